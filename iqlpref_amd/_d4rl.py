"""What the gym < 0.26 D4RL baselines (``awac``, ``offline_bc``) spell the same way: the evaluation rollout, the
device, environment and dataset defaults of ``train()`` and the command line.  ``finetune.train`` takes its device
default from here.  gym and d4rl are imported only where a default needs them."""
import os
from typing import Callable, Optional

import numpy as np
import torch

from . import distributed as D


@torch.no_grad()
def eval_actor(env, actor, device: str, n_episodes: int, seed: int) -> np.ndarray:
    """``env.seed(seed)`` once, then ``n_episodes`` chained episodes of a gym < 0.26 environment (``reset() ->
    obs``, ``step() -> (obs, reward, done, info)``) on ``actor.act`` in eval mode, returns accumulated from the
    Python float 0.0.  The actor is handed back in train mode."""
    env.seed(seed)
    actor.eval()
    episode_rewards = []
    try:
        for _ in range(n_episodes):
            state, done = env.reset(), False
            episode_reward = 0.0
            while not done:
                action = actor.act(state, device)
                state, reward, done, _ = env.step(action)
                episode_reward += reward
            episode_rewards.append(episode_reward)
    finally:
        actor.train()
    return np.asarray(episode_rewards)


def default_device(config, device: Optional[str] = None) -> str:
    """``device`` as given; None: the rank's GPU, else ``config.device`` ("cuda" is "cuda:0")."""
    return device or D.local_device() or ("cuda:0" if config.device == "cuda" else config.device)


def default_env(env_name: str, env=None, dataset=None):
    """``env`` as given; None: ``gym.make(env_name)``, d4rl first registering its environments if it is to be used."""
    if env is None:
        import gym
        if dataset is None:
            import d4rl  # noqa: F401
        env = gym.make(env_name)
    return env


def default_dataset(env, dataset=None):
    """``dataset`` as given; None: ``d4rl.qlearning_dataset(env)``."""
    if dataset is None:
        import d4rl
        dataset = d4rl.qlearning_dataset(env)
    return dataset


def cli(prog: str, load_config: Callable, train: Callable, argv=None) -> None:
    """``python -m <prog> --config_path file.yaml --field value ... [--seeds_per_gpu K]`` (pyrallis.wrap there)."""
    import argparse
    from .train import parse_overrides
    ap = argparse.ArgumentParser(prog=f"python -m {prog}")
    ap.add_argument("--config_path", default=None)
    ap.add_argument("--seeds_per_gpu", type=int, default=int(os.environ.get("AGENTS_PER_GPU", "1")),
                    help="independent seeds trained side by side on each GPU")
    args, rest = ap.parse_known_args(argv)
    train(load_config(args.config_path, **parse_overrides(rest)), seeds_per_gpu=args.seeds_per_gpu)
