#!/usr/bin/env python3
"""Generate tests/golden/finetune_run.npz by RUNNING the reference's offline-to-online ``train()``
(algorithms/finetune/iql.py:566-767, "fref") on the CPU.

Run where the reference is at hand (it never travels to the GPU machine):

    python tests/golden/make_finetune_fixture.py [--ref /root/reference]

fref is imported with inert stubs for the packages it names (gym, d4rl, pyrallis, wandb); ``train`` then
runs as written against stand-ins: ``gym.make`` gives a recording ``tests/finetune_env.py`` environment,
``d4rl.qlearning_dataset`` a small rolled-out dataset, ``wandb.log`` records every call.  Two runs: a
Gaussian actor on a locomotion-named environment with ``normalize_reward`` (the scaled rewards and the
full ``reward_mod_dict``), and a deterministic actor on a goal environment (success and regret records,
antmaze's ``- 1``).  ``buffer_size`` is smaller than dataset + online steps: the ring wraps.

Only inputs and outputs are stored: the dataset, every step's index batch, the exploration noise of every
tick (the samplers are wrapped: ``Normal.sample`` becomes ``loc + scale * eps`` with the recorded eps,
``torch.randn_like`` hands out the recorded eps), what both environments handed out and were given, the
per-step losses and actor learning rates, every log record, the buffer at the end, and of the initial parameters
and of every checkpoint each tensor whole (up to 4096 elements) or every 61st element of it.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import fake_envs  # noqa: E402
from tests import finetune_env as fe  # noqa: E402

COMMON = dict(offline_iterations=30, online_iterations=60, batch_size=16, eval_freq=30, n_episodes=2, buffer_size=80,
              n_dataset=50, data_seed=21, eval_seed=4)
# name -> (env name, seed, iql_deterministic, normalize_reward)
RUNS = {"gauss": ("halfcheetah-standin-v0", 3, False, True), "det": ("antmaze-standin-v0", 7, True, True)}
WHOLE, EVERY = 4096, 61  # tensors of up to WHOLE elements are stored whole, of larger ones every EVERY-th element


def import_finetune_reference(ref_root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("d4rl")
    stub("gym", Env=object, wrappers=types.SimpleNamespace(TransformObservation=fake_envs.TransformObservation,
                                                           TransformReward=fake_envs.TransformReward))
    stub("wandb")
    stub("pyrallis", wrap=lambda *a, **k: (lambda f: f))
    path = os.path.join(ref_root, "algorithms", "finetune", "iql.py")
    spec = importlib.util.spec_from_file_location("ref_finetune_iql", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def sample_of(v):
    """What the fixture keeps of one parameter tensor (tests/test_gpu_finetune.py takes the same elements)."""
    flat = v.detach().reshape(-1).numpy()
    return flat.copy() if flat.size <= WHOLE else flat[::EVERY].copy()


def net_arrays(prefix, sd):
    return {f"{prefix}/{net}/{k}": sample_of(v) for net in ("qf", "vf", "actor") for k, v in sd[net].items()}


def run(fref, name, env_name, seed, deterministic, normalize_reward):
    c = COMMON
    envs, records, saves, idx, eps, losses, lrs, out = [], [], [], [], [], [], [], {}
    raw = fe.make_dataset(env_name, c["n_dataset"], c["data_seed"])

    def make(env_id):
        envs.append(fe.RecordingEnv(fe.FinetuneEnv(env_id)))
        return envs[-1]

    def log(d, step=None):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    fref.gym.make = make
    fref.d4rl.qlearning_dataset = lambda env: {k: v.copy() for k, v in raw.items()}
    fref.wandb.init = lambda **kw: None
    fref.wandb.run = types.SimpleNamespace(save=lambda: None)
    fref.wandb.log = log
    fref.pyrallis.dump = lambda cfg, f: f.write("# written by the pyrallis stand-in\n")

    real_normal, real_sample, real_train, real_init = fref.Normal, fref.ReplayBuffer.sample, fref.ImplicitQLearning.train, \
        fref.ImplicitQLearning.__init__
    real_modify, real_add = fref.modify_reward, fref.ReplayBuffer.add_transition
    real_randn_like, real_save = torch.randn_like, torch.save
    added = []

    class RecordedNormal(real_normal):
        def sample(self, sample_shape=torch.Size()):
            e = torch.randn(self._extended_shape(sample_shape))
            eps.append(e.numpy().reshape(-1).copy())
            return self.loc + self.scale * e

    def randn_like(x, **kw):
        e = real_randn_like(x, **kw)
        eps.append(e.numpy().reshape(-1).copy())
        return e

    def sample(self, batch_size):
        st = np.random.get_state()
        batch = real_sample(self, batch_size)
        np.random.set_state(st)
        idx.append(np.random.randint(0, self._size, size=batch_size))  # the same draw again: the indices it used
        out.setdefault("buffer", self)
        return batch

    def train_step(self, batch):
        lrs.append(self.actor_optimizer.param_groups[0]["lr"])
        d = real_train(self, batch)
        losses.append([d["value_loss"], d["q_loss"], d["actor_loss"]])
        return d

    def init(self, **kw):
        real_init(self, **kw)
        out.update(net_arrays(f"{name}/init", {"qf": self.qf.state_dict(), "vf": self.vf.state_dict(),
                                               "actor": self.actor.state_dict()}))

    def modify(dataset, env_id, max_episode_steps=1000):
        d = real_modify(dataset, env_id, max_episode_steps)
        out[f"{name}/reward_mod_keys"] = np.asarray(sorted(d), dtype=str)
        out[f"{name}/reward_mod_values"] = np.asarray([d[k] for k in sorted(d)], np.float64)
        out[f"{name}/dataset_rewards_modified"] = dataset["rewards"].copy()
        return d

    def add(self, state, action, reward, next_state, done):
        added.append((float(reward), bool(done)))
        real_add(self, state, action, reward, next_state, done)

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        out.update(net_arrays(f"{name}/ckpt/{os.path.basename(path)}", obj))
        out[f"{name}/ckpt/{os.path.basename(path)}/total_it"] = np.int64(obj["total_it"])
        out[f"{name}/ckpt/{os.path.basename(path)}/last_epoch"] = np.int64(obj["actor_lr_schedule"]["last_epoch"])
        real_save(obj, path)

    fref.Normal, fref.ReplayBuffer.sample, fref.ImplicitQLearning.train = RecordedNormal, sample, train_step
    fref.ImplicitQLearning.__init__, fref.modify_reward, fref.ReplayBuffer.add_transition = init, modify, add
    torch.randn_like, torch.save = randn_like, save
    try:
        with tempfile.TemporaryDirectory() as tmp:
            config = fref.TrainConfig(device="cpu", env=env_name, seed=seed, eval_seed=c["eval_seed"],
                                      eval_freq=c["eval_freq"], n_episodes=c["n_episodes"],
                                      offline_iterations=c["offline_iterations"],
                                      online_iterations=c["online_iterations"], checkpoints_path=tmp,
                                      buffer_size=c["buffer_size"], batch_size=c["batch_size"],
                                      iql_deterministic=deterministic, normalize_reward=normalize_reward)
            out[f"{name}/config_name_prefix"] = np.asarray(config.name[:-8])
            out[f"{name}/config_path_tail"] = np.asarray(os.path.relpath(config.checkpoints_path, tmp)[:-8])
            fref.train(config)
    finally:
        fref.Normal, fref.ReplayBuffer.sample, fref.ImplicitQLearning.train = real_normal, real_sample, real_train
        fref.ImplicitQLearning.__init__, fref.modify_reward, fref.ReplayBuffer.add_transition = real_init, real_modify, real_add
        torch.randn_like, torch.save = real_randn_like, real_save
    buf = out.pop("buffer")
    state = np.random.get_state()
    out.update({f"{name}/env_name": np.asarray(env_name), f"{name}/seed": np.int64(seed),
                f"{name}/deterministic": np.bool_(deterministic), f"{name}/normalize_reward": np.bool_(normalize_reward),
                f"{name}/expl_noise": np.float64(config.expl_noise), f"{name}/noise_clip": np.float64(config.noise_clip),
                f"{name}/rec_step": np.asarray([r[0] for r in records], np.int64),
                f"{name}/rec_key": np.asarray([r[1] for r in records]),
                f"{name}/rec_value": np.asarray([r[2] for r in records], np.float64),
                f"{name}/save_step": np.asarray([s[0] for s in saves], np.int64),
                f"{name}/save_name": np.asarray([s[1] for s in saves]),
                f"{name}/idx": np.asarray(idx, np.int64), f"{name}/eps": np.asarray(eps, np.float32),
                f"{name}/losses": np.asarray(losses, np.float64), f"{name}/actor_lr": np.asarray(lrs, np.float64),
                f"{name}/added_reward": np.asarray([a[0] for a in added], np.float64),
                f"{name}/added_done": np.asarray([a[1] for a in added], bool),
                f"{name}/np_key": np.asarray(state[1], np.uint32), f"{name}/np_pos": np.int64(state[2]),
                f"{name}/buf_pointer": np.int64(buf._pointer), f"{name}/buf_size": np.int64(buf._size),
                f"{name}/buf_states": buf._states.numpy().copy(), f"{name}/buf_actions": buf._actions.numpy().copy(),
                f"{name}/buf_rewards": buf._rewards.numpy().copy(),
                f"{name}/buf_next_states": buf._next_states.numpy().copy(), f"{name}/buf_dones": buf._dones.numpy().copy()})
    for k, v in raw.items():
        out[f"{name}/dataset/{k}"] = v
    out.update(envs[0].tape(f"{name}/env"))
    out.update(envs[1].tape(f"{name}/eval_env"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    fref = import_finetune_reference(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    out = {f"common/{k}": np.asarray(v) for k, v in COMMON.items()}
    d = fref.TrainConfig()
    names = sorted(k for k in vars(d) if k not in ("name", "checkpoints_path"))
    out["defaults/keys"] = np.asarray(names)
    out["defaults/values"] = np.asarray([repr(getattr(d, k)) for k in names])
    for name, spec in RUNS.items():
        out.update(run(fref, name, *spec))
    path = os.path.join(HERE, "finetune_run.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
