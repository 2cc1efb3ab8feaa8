#!/usr/bin/env python3
"""Time the Bayesian-reward relabel (custom_offline_br) piece by piece on one GPU:

    python tools/bench_br_relabel.py [--N 1000000] [--S 500] [--n 100] [--reps 5] [--host-rows 20000]

  predictions   S exact-fp32 MLP forwards into the device [S, N] matrix (PosteriorRewardNet.predictions)
  choice        iqlhip_posterior_choice end to end (draw + gather-reduce overlapped), MEAN and MEDIAN,
                and n = 1 (reward_type 0); state upload / download included
  np_randint    iqlhip_np_randint for the same N * n values at the same hi: the draw alone, as the
                existing kernel does it (it materialises the int64 indices: 8 N n bytes)
  host          the reference's loop (np.random.choice per row) on --host-rows rows of the CPU of this
                machine, scaled to N: a CPU figure

Medians of --reps runs after one warm-up, one JSON line.  The split of `choice` into its kernels
(k_choice_draw / k_choice_reduce) comes from a kernel trace of this script, not from here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iqlpref_amd import _lib  # noqa: E402
from iqlpref_amd import custom_offline_br as br  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--S", type=int, default=500)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=20_000)
    ap.add_argument("--in-dim", type=int, default=69)  # pen: 45 + 24
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--depth", type=int, default=3)
    a = ap.parse_args()
    lib = _lib.load()
    rng = np.random.default_rng(0)
    dims = [a.in_dim] + [a.width] * a.depth + [1]
    sets = [[x for i, o in zip(dims[:-1], dims[1:])
             for x in ((rng.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32),
                       (0.1 * rng.standard_normal(o)).astype(np.float32))] for _ in range(a.S)]
    model = br.PosteriorRewardNet(sets, None, "relu", DEV)
    x = torch.from_numpy(rng.standard_normal((a.N, a.in_dim)).astype(np.float32)).to(DEV)
    res = {"N": a.N, "S": a.S, "n_samps": a.n, "reps": a.reps, "build_tag": _lib.build_tag(),
           "device": torch.cuda.get_device_name(0)}
    res["predictions_s"] = timed(lambda: model.predictions(x), a.reps)
    preds = model.predictions(x)
    rs = np.random.RandomState(0)
    res["choice_mean_s"] = timed(lambda: br.posterior_choice(preds, a.n, br.MEAN, rs), a.reps)
    res["choice_median_s"] = timed(lambda: br.posterior_choice(preds, a.n, br.MEDIAN, rs), a.reps)
    res["choice_first_s"] = timed(lambda: br.posterior_choice(preds, 1, br.MEAN, rs), a.reps)
    # the draw alone by the existing kernel, same hi, same number of values
    state = torch.from_numpy(br.pack_np_state(rs.get_state()).view(np.int32)[None].copy()).to(DEV)
    idx = torch.empty((a.N, a.n), dtype=torch.int64, device=DEV)

    def randint():
        with torch.cuda.device(DEV):
            _lib.check(lib.iqlhip_np_randint(_lib.ptr(state), (C.c_int64 * 1)(a.S), 1, a.n, a.N,
                                             (C.c_void_p * 1)(idx.data_ptr()), _lib.stream_ptr()))
    res["np_randint_s"] = timed(randint, a.reps)
    total = a.N * a.n
    res["values_per_s"] = {"choice_mean": total / res["choice_mean_s"][0], "choice_median": total / res["choice_median_s"][0],
                           "np_randint": total / res["np_randint_s"][0]}
    res["choice_over_randint"] = res["choice_mean_s"][0] / res["np_randint_s"][0]
    res["relabel_over_predictions"] = {m: (res["predictions_s"][0] + res[f"choice_{m}_s"][0]) / res["predictions_s"][0]
                                       for m in ("mean", "median", "first")}
    # the reference's host loop on a slice of the rows (CPU of this machine)
    rows = min(a.host_rows, a.N)
    if rows > 0:
        host = np.ascontiguousarray(preds[:, :rows].t().cpu().numpy())
        t0 = time.perf_counter()
        for row in host:
            np.random.choice(row, a.n)
        dt = time.perf_counter() - t0
        res["host_cpu_loop"] = {"rows": rows, "seconds": dt, "us_per_row": 1e6 * dt / rows,
                                "scaled_to_N_s": dt / rows * a.N}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
