"""``algorithms/minari/iql.py`` ("mref"): IQL on the task rewards of a Minari dataset -- the pen counterpart
of the antmaze ``tr_sweeps`` oracle baseline, whose checkpoints ``iqlpref_amd.posthoc`` evaluates
(``human_pen_models/iql-D4RL/...``, ``evaluation/minari/iql_stats.py``).

mref is ``algorithms/custom_offline/iql.py`` with the reward model taken out: ``qlearning_dataset`` keeps
``episode.rewards`` as they are stored (mref:147-165) and everything behind it is the same program.  So is this
module: ``train()`` is ``custom_offline._train`` with that function as the relabel -- ``modify_reward``, the state
normalisation, ``NumpyIndexStream``, the fused fp32 step with the convex Polyak form, ``_offline_loop.run`` with
its best-model rule, ``seeds_per_gpu`` and ``resume``.  Checkpoints carry the custom flavour's keys.
"""
import os
import uuid
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Optional

import numpy as np

from . import custom_offline as _co
from .custom_offline import ImplicitQLearning, ReplayBuffer, evaluate, modify_reward  # noqa: F401  (mref's names)


@dataclass
class TrainConfig:
    """mref:36-70, same fields and defaults (``custom_offline.TrainConfig`` without the reward model)."""
    project: str = "IQL-pref"
    group: str = "IQL-Minari"
    name: str = "iql"
    gamma: float = 0.99
    tau: float = 0.005
    beta: float = 3.0
    iql_tau: float = 0.7
    iql_deterministic: bool = False
    vf_lr: float = 3e-4
    qf_lr: float = 3e-4
    actor_lr: float = 3e-4
    actor_dropout: Optional[float] = None
    dataset_id: str = "D4RL/pen/human-v2"
    update_steps: int = int(1e6)
    buffer_size: int = 2_000_000
    batch_size: int = 256
    normalize_state: bool = True
    normalize_reward: bool = False
    eval_every: int = int(5e3)
    eval_episodes: int = 10
    train_seed: int = 0
    eval_seed: int = 0
    checkpoints_path: Optional[str] = None

    def __post_init__(self):
        self.name = f"{self.name}-{self.dataset_id}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)


def qlearning_dataset(dataset: Iterable) -> Dict[str, np.ndarray]:
    """mref:147-165.  ``dataset`` iterates episodes (Minari ``EpisodeData`` or dicts) with ``observations``
    [L+1, S], ``actions`` [L, A], ``rewards`` [L], ``terminations`` [L]; the rewards keep their stored dtype."""
    episodes = list(dataset)
    obs, act, nxt, dones, _ = _co._concat_episodes(episodes)
    rewards = np.concatenate([np.asarray(ep["rewards"] if isinstance(ep, dict) else ep.rewards) for ep in episodes])
    return {"observations": obs, "actions": act, "next_observations": nxt, "rewards": rewards, "terminals": dones}


def train(config: TrainConfig, dataset=None, eval_env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None,
          normalized_score: Optional[Callable] = None, seeds_per_gpu: int = 1, sampler: str = "device",
          device: Optional[str] = None, chunk: int = 2000, resume: bool = False):
    """mref:535-690 on the fused HIP step: ``custom_offline.train`` without ``reward_model`` -- the arguments, the
    records, the files, ``seeds_per_gpu`` and ``resume`` are described there."""
    return _co._train(config, dataset, eval_env, qlearning_dataset, False, logger=logger,
                      normalized_score=normalized_score, seeds_per_gpu=seeds_per_gpu, sampler=sampler, device=device,
                      chunk=chunk, resume=resume, where="minari_iql.train")
