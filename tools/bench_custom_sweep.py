"""A pen sweep grid as one launch batch against the same runs one after another, at pen shape (S 45 / A 24 /
H 256 / B 256, fp32, actor dropout 0.1): ten runs that differ in the reward model (ten QMLPs, so ten relabels
and ten 5,000-row buffers), evaluation off, three legs alternated within every repetition:

  batch    custom_offline.train_runs(configs, runs_per_gpu=10): one seed group of ten;
  single   custom_offline.train_runs(configs, runs_per_gpu=1): ten batches of one, each stepping its trainer
           directly;
  solo     custom_offline.train(config) ten times, one after another.

Every leg is timed as a whole call (host clock, ending in a device synchronise) at two lengths, ``--short`` and
``--long`` steps per run.  ``call`` is the rate of the long call, set-up included (relabels, buffers, nets, device
handles, the first graph capture); ``steady`` is (long - short) steps over (long - short) seconds, in which the
set-up cancels.  Rates are run-steps/s: ten runs of n steps count 10 n.  The loggers are no-ops, but every step
still makes its record, as in a real run.  The last line is one JSON object with the median of the repetitions.

    python tools/bench_custom_sweep.py [--runs 10] [--short 4000] [--long 24000] [--reps 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iqlpref_amd import _lib  # noqa: E402
from iqlpref_amd import custom_offline as co  # noqa: E402

DEV, S, A, B, ROWS, EP_LEN, DROPOUT = "cuda:0", 45, 24, 256, 5000, 100, 0.1


class _Box:
    def __init__(self, n, high):
        self.shape, self.high = (n,), np.full(n, high)


class _Env:
    """The spaces train() reads; never stepped (evaluation is off)."""
    observation_space, action_space = _Box(S, np.inf), _Box(A, 1.0)


def episodes(seed):
    rng = np.random.default_rng(seed)
    return [{"observations": rng.standard_normal((EP_LEN + 1, S)), "actions": rng.uniform(-1, 1, (EP_LEN, A)),
             "terminations": np.arange(EP_LEN) == EP_LEN - 1} for _ in range(ROWS // EP_LEN)]


def reward_model(seed):
    rng = np.random.default_rng(seed)
    dims = (S + A, 256, 256, 1)
    layers = [{"kernel": (rng.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32),
               "bias": (0.1 * rng.standard_normal(o)).astype(np.float32)} for i, o in zip(dims[:-1], dims[1:])]
    return co.QMLP(S, A, (256, 256), "relu", "none").load_flax_params(layers).to(DEV)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--short", type=int, default=4000, help="steps per run of the short call")
    ap.add_argument("--long", type=int, default=24000, help="steps per run of the long call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args(argv)
    if not 1 <= args.runs <= _lib.MAX_GROUP or not 0 < args.short < args.long:
        ap.error(f"--runs in 1..{_lib.MAX_GROUP} and 0 < --short < --long")
    _lib.require_gpu(DEV)
    data = episodes(0)
    models = {f"model_{k}": reward_model(100 + k) for k in range(args.runs)}
    quiet = lambda record, step: None
    score = lambda ds, returns: np.asarray(returns)

    def configs(n):
        return [co.TrainConfig(reward_model_path=path, dataset_id="bench/pen-shape-v0", train_seed=0, batch_size=B,
                               actor_dropout=DROPOUT, buffer_size=ROWS, update_steps=n, eval_every=n + 1)
                for path in models]

    def batch(n):
        co.train_runs(configs(n), data, models, _Env(), runs_per_gpu=args.runs, logger=quiet, normalized_score=score)

    def single(n):
        co.train_runs(configs(n), data, models, _Env(), runs_per_gpu=1, logger=quiet, normalized_score=score)

    def solo(n):
        for cfg in configs(n):
            co.train(cfg, data, models[cfg.reward_model_path], _Env(), logger=quiet, normalized_score=score, device=DEV)

    legs = {"batch": batch, "single": single, "solo": solo}

    def timed(leg, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for leg in legs.values():  # warm-up: code objects, allocator, every path once
        leg(min(args.short, 2000))
    rates = {name: {"call": [], "steady": []} for name in legs}
    for rep in range(args.reps):
        for name, leg in legs.items():
            t_short, t_long = timed(leg, args.short), timed(leg, args.long)
            call = args.runs * args.long / t_long
            steady = args.runs * (args.long - args.short) / (t_long - t_short)
            rates[name]["call"].append(call), rates[name]["steady"].append(steady)
            print(f"rep {rep} {name:>6}: short {t_short:7.3f} s  long {t_long:7.3f} s  call {call:9.0f}  "
                  f"steady {steady:9.0f} run-steps/s", flush=True)
    summary = lambda r: {"median": statistics.median(r), "min": min(r), "max": max(r)}
    result = {"build_tag": _lib.build_tag(),
              "shape": {"S": S, "A": A, "H": 256, "B": B, "rows_per_run": ROWS, "precision": "fp32", "dropout": DROPOUT},
              "runs": args.runs, "short": args.short, "long": args.long, "reps": args.reps,
              "run_steps_per_s": {name: {k: summary(v) for k, v in r.items()} for name, r in rates.items()}}
    med = lambda name, k: result["run_steps_per_s"][name][k]["median"]
    result["batch_over_solo"] = {k: med("batch", k) / med("solo", k) for k in ("call", "steady")}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
