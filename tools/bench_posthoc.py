"""One lock step of the post-hoc evaluation at pen shape (S 45, A 24, 2 x 256), two ways: grouped
(``posthoc.policy_actions_many`` on an MlpSet: one launch for M actors x R rows) and as M ``policy_actions``
calls (the path the sequential programs take, R rows at a time).  Both include what a step of the evaluation
pays besides the kernel: the observations' copy to the device, the clamp and the actions' copy back, which is
the host wait.

    python tools/bench_posthoc.py [--windows 5] [--seconds 0.4]

Per case the two variants alternate in windows of at least ``--seconds`` each after a warm-up of every shape;
the figure is the median window's time per step, with the spread (min .. max) beside it.  The outputs of the
two variants are compared bit for bit before anything is timed.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ((8, 16), (64, 2), (200, 1))  # (M checkpoints, R environments each)
S, A, WIDTH, DEV = 45, 24, 256, "cuda:0"


def window(fn, seconds):
    """Seconds per call over a window of at least ``seconds`` (every call ends in a device-to-host copy)."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.4)
    args = ap.parse_args(argv)
    import iqlpref_amd as ia
    from iqlpref_amd import posthoc
    if not torch.cuda.is_available():
        raise SystemExit("bench_posthoc needs the GPU: a host timing says nothing about it")
    for M, R in CASES:
        actors = []
        for m in range(M):
            torch.manual_seed(m)
            actors.append(ia.GaussianPolicy(S, A, 1.0, hidden_dim=WIDTH, n_hidden=2, dropout=0.1).to(DEV).eval())
        obs = np.random.default_rng(M).standard_normal((M, R, S))
        actor_set = posthoc.MlpSet([a.net for a in actors], DEV)

        def grouped():
            return posthoc.policy_actions_many(actor_set, obs, 1.0)

        def solo():
            return np.stack([ia.policy_actions(a, obs[m], 1.0, DEV) for m, a in enumerate(actors)])
        same = bool(np.array_equal(grouped().view(np.uint32), solo().view(np.uint32)))
        for _ in range(3):  # warm-up of both shapes
            grouped(), solo()
        torch.cuda.synchronize()
        tg, ts = [], []
        for _ in range(args.windows):
            tg.append(window(grouped, args.seconds))
            ts.append(window(solo, args.seconds))
        g, s = statistics.median(tg), statistics.median(ts)
        print(json.dumps({"M": M, "R": R, "bits_equal": same,
                          "grouped_ms": round(g * 1e3, 4), "grouped_ms_min_max": [round(min(tg) * 1e3, 4),
                                                                                  round(max(tg) * 1e3, 4)],
                          "solo_ms": round(s * 1e3, 4), "solo_ms_min_max": [round(min(ts) * 1e3, 4),
                                                                            round(max(ts) * 1e3, 4)],
                          "speedup": round(s / g, 2)}), flush=True)
        actor_set.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
