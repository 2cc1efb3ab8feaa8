"""Phase 2a of PIPELINE.md on one MI355X: the normalize_reward selection sweep (indices 0..7, seed 0)
as one process, against the seeds-per-GPU yardstick and a single run.

    python tools/sweep_run.py [--steps 20000] [--rows 1000000] [--only train_runs,group,seeds,solo]

Synthetic antmaze-shaped data (S 29, A 8, B 256, bf16): ``--rows`` transitions in 1000-step episodes
with sparse rewards, so that indices 2-7 see a return range.  No evaluation.  One JSON line per
variant:
  train_runs        8 configs (normalize_reward 0..7) through sweep.train_runs, default group mode
  train_runs_group  the same with group_mode="group" (one launch sequence for all 8)
  seeds_per_gpu     train(config, seeds_per_gpu=8): 8 seeds of ONE config (the yardstick)
  solo              train(config): one run
``steps_per_s`` = runs x steps per second of training, timed between the first and the last logging
window (the logger is called after each window's one host sync); ``prep_s`` = seconds spent in
dataset preparation (build_dataset + the device buffers), ``wall_s`` = the whole call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iqlpref_amd as ia  # noqa: E402
from iqlpref_amd import _lib  # noqa: E402

T = sys.modules["iqlpref_amd.train"]
DEV = "cuda:0"
S, A = 29, 8
ENV = "antmaze-medium-diverse-v2"


class Env:
    def __init__(self):
        self.observation_space = type("Box", (), {"shape": (S,)})()
        self.action_space = type("Box", (), {"shape": (A,), "high": np.ones(A, np.float32)})()


def dataset(rows):
    rng = np.random.default_rng(0)
    ep = np.arange(rows) // 1000  # 1000-step episodes (no terminals: each ends on the step limit)
    p = 0.002 + 0.02 * rng.uniform(size=ep.max() + 1)  # per-episode success rate: returns differ
    return {"observations": rng.standard_normal((rows, S), dtype=np.float32),
            "actions": rng.uniform(-1, 1, (rows, A)).astype(np.float32),
            "rewards": (rng.uniform(size=rows) < p[ep]).astype(np.float32),
            "next_observations": rng.standard_normal((rows, S), dtype=np.float32),
            "terminals": np.zeros(rows, np.float32)}


def config(nr, steps):
    return ia.TrainConfig(env=ENV, normalize_reward=nr, seed=0, max_timesteps=steps, log_freq=250,
                          eval_freq=10 ** 9, batch_size=256, device=DEV, buffer_size=10_000_000)


class Timer:
    """Seconds spent in dataset preparation, and the time of every logging window."""

    def __init__(self):
        self.prep = 0.0
        self.stamps = []
        self._saved = {}

    def wrap(self, name):
        real = getattr(T, name)

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **kw)
            torch.cuda.synchronize()
            self.prep += time.perf_counter() - t0
            return out
        self._saved[name] = real
        setattr(T, name, timed)

    def __enter__(self):
        self.wrap("build_dataset")
        self.wrap("_prepare_replay")
        return self

    def __exit__(self, *exc):
        for name, real in self._saved.items():
            setattr(T, name, real)

    def log(self, rec, step):
        self.stamps.append((step, time.perf_counter()))


def measure(name, n_runs, steps, fn):
    torch.cuda.synchronize()
    with Timer() as tm:
        t0 = time.perf_counter()
        fn(tm.log)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    first = {}
    for st, t in tm.stamps:  # one stamp per run and window; the first of each step counts
        first.setdefault(st, t)
    steps_list = sorted(first)
    s0, s1 = steps_list[0], steps_list[-1]
    rate = n_runs * (s1 - s0) / (first[s1] - first[s0])
    rec = {"variant": name, "runs": n_runs, "steps": steps, "steps_per_s": round(rate), "prep_s": round(tm.prep, 2),
           "wall_s": round(wall, 2), "build": _lib.build_tag()}
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--only", default="train_runs,train_runs_group,seeds_per_gpu,solo")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args(argv)
    data, env, n = dataset(args.rows), Env(), args.steps
    quiet = lambda d, step: None
    variants = {
        "train_runs": (8, lambda log: ia.train_runs([config(nr, n) for nr in range(8)], env, data, logger=log)),
        "train_runs_group": (8, lambda log: ia.train_runs([config(nr, n) for nr in range(8)], env, data,
                                                          logger=log, group_mode="group")),
        "seeds_per_gpu": (8, lambda log: ia.train(config(1, n), env, data, logger=log, seeds_per_gpu=8)),
        "solo": (1, lambda log: ia.train(config(1, n), env, data, logger=log)),
    }
    recs = []
    ia.train(config(1, 500), env, data, logger=quiet)  # warm-up: library load, first graphs
    for name in args.only.split(","):
        k, fn = variants[name]
        recs.append(measure(name, k, n, fn))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
