#!/usr/bin/env python3
"""Generate tests/golden/custom_train_run.npz by RUNNING the reference's custom-flavour ``train()``
(algorithms/custom_offline/iql.py:597-749, "cref") on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_custom_train_fixture.py [--ref /root/reference]

cref is imported with ``make_fixtures.import_custom_reference`` (inert stubs for the absent
packages); ``train`` then runs as written against stand-ins: a fake Minari dataset of a few episodes
of a gymnasium-API environment (tests/custom_train_env.py), ``load_QMLP`` returning a numpy reward
MLP whose parameters are regenerated from a seed, ``wandb.log`` recording every call, and
``minari.get_normalized_score`` raising ``ValueError`` in run "raw" and affine in run "norm" (the two
best-score branches of cref:711-735).  Only inputs and outputs are stored: the log records, the
checkpoint files written at each step, per-tensor sums and a few full tensors of ``best_model.pt``
and the last checkpoint, and the final ``np.random.get_state()``.
"""
import argparse
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
from tests import custom_train_env as cte  # noqa: E402
from tests.golden import make_fixtures  # noqa: E402

# one entry per run: (train_seed, normalized score: None = raises ValueError, else (a, b): a + b * returns)
RUNS = {"raw": (3, None), "norm": (7, (2.0, 0.5))}
# 60 steps, as the offline flavour's train_runs replay: on this 287-row stand-in the CPU and GPU fp32
# trajectories part by more than 2e-5 after ~55 steps (rounding amplified by Adam), 3e-2 by step 300
COMMON = dict(update_steps=60, eval_every=20, batch_size=64, eval_episodes=2, eval_seed=4,
              data_seed=11, reward_seed=5, lengths=(40, 55, 33, 60, 47, 52))
FULL = {"actor": "net.net.4.weight", "vf": "v.net.4.weight", "qf": "q1.net.4.weight"}  # stored whole


def checkpoint_arrays(prefix, sd):
    out = {}
    for net in ("qf", "vf", "actor"):
        for k, v in sd[net].items():
            out[f"{prefix}/{net}/{k}/sum"] = np.float64(v.double().sum().item())
        out[f"{prefix}/{net}/{FULL[net]}"] = sd[net][FULL[net]].numpy()
    for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
        for i, st in sd[opt]["state"].items():
            for k in ("exp_avg", "exp_avg_sq"):
                out[f"{prefix}/{opt}/{i}/{k}/sum"] = np.float64(st[k].double().sum().item())
            out[f"{prefix}/{opt}/{i}/step"] = np.float64(float(st["step"]))
    out[f"{prefix}/actor_lr_scheduler/last_epoch"] = np.int64(sd["actor_lr_scheduler"]["last_epoch"])
    out[f"{prefix}/actor_lr_scheduler/last_lr"] = np.float64(sd["actor_lr_scheduler"]["_last_lr"][0])
    return out


def run(cref, name, train_seed, affine):
    c = COMMON
    dataset = cte.MinariDataset(c["data_seed"], c["lengths"])
    S, A = dataset.recover_environment().S, dataset.recover_environment().A
    layers = cte.reward_layers(c["reward_seed"], S, A)
    records, saves = [], []

    def log(d, step):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    def normalized(ds, returns):
        if affine is None:
            raise ValueError("no reference scores for this dataset")
        return affine[0] + affine[1] * np.asarray(returns)

    cref.wandb = types.SimpleNamespace(init=lambda **kw: None, log=log)
    cref.minari = types.SimpleNamespace(download_dataset=lambda i: None, load_dataset=lambda i: dataset,
                                        get_normalized_score=normalized)
    cref.ocp = types.SimpleNamespace(Checkpointer=lambda h: types.SimpleNamespace(close=lambda: None),
                                     CompositeCheckpointHandler=lambda: None)
    cref.load_QMLP = lambda path, checkpointer, on_cpu=True: cte.numpy_reward(layers)
    cref.nnx = types.SimpleNamespace(jit=lambda f, **kw: f)
    cref.pyrallis = types.SimpleNamespace(dump=lambda cfg, f: f.write(repr(cfg)))
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    with tempfile.TemporaryDirectory() as tmp:
        config = cref.TrainConfig(update_steps=c["update_steps"], eval_every=c["eval_every"],
                                  batch_size=c["batch_size"], eval_episodes=c["eval_episodes"],
                                  eval_seed=c["eval_seed"], train_seed=train_seed, checkpoints_path=tmp)
        torch.save = save
        try:
            cref.train(config)
        finally:
            torch.save = real_save
        state = np.random.get_state()
        last = max((s for s in saves if s[1].startswith("checkpoint_")), key=lambda s: s[0])[1]
        best = torch.load(os.path.join(config.checkpoints_path, "best_model.pt"), weights_only=True)
        final = torch.load(os.path.join(config.checkpoints_path, last), weights_only=True)
    out = {f"{name}/train_seed": np.int64(train_seed),
           f"{name}/affine": np.asarray(affine if affine is not None else (np.nan, np.nan), np.float64),
           f"{name}/rec_step": np.asarray([r[0] for r in records], np.int64),
           f"{name}/rec_key": np.asarray([r[1] for r in records]),
           f"{name}/rec_value": np.asarray([r[2] for r in records], np.float64),
           f"{name}/save_step": np.asarray([s[0] for s in saves], np.int64),
           f"{name}/save_name": np.asarray([s[1] for s in saves]),
           f"{name}/np_key": np.asarray(state[1], np.uint32), f"{name}/np_pos": np.int64(state[2]),
           f"{name}/np_has_gauss": np.int64(state[3]), f"{name}/np_cached": np.float64(state[4])}
    out.update(checkpoint_arrays(f"{name}/best", best))
    out.update(checkpoint_arrays(f"{name}/last", final))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    cref = make_fixtures.import_custom_reference(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    out = {f"common/{k}": np.asarray(v) for k, v in COMMON.items()}
    for name, (seed, affine) in RUNS.items():
        out.update(run(cref, name, seed, affine))
    path = os.path.join(HERE, "custom_train_run.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
