#!/usr/bin/env python3
"""Time of the any-percent selection (algorithms/offline/any_percent_bc.py:206-239 keep_best_trajectories) at an
antmaze-like size -- n = 1,000,000 rows, trajectories of up to 1000 rows, frac 0.1, S 29 / A 8 -- three ways:

  device_path offline_bc.select_best_trajectories on arrays that already lie on the GPU: the trajectory walk, the
              copy of the returns to the host, the host argsort and the five gathers, to a device synchronise;
  host_restatement  offline_bc.keep_best_trajectories, the vectorised host restatement, on a fresh copy of the dict;
  python_loop the reference's loop, restated here, on the first ``--loop_rows`` rows (default 100,000), with the
              fancy-index copies of that slice; the figure printed is that time SCALED by n / loop_rows and
              labelled so.

    python tools/bench_offline_bc.py [--repeats 5] [--rows 1000000] [--loop_rows 100000] [--json out.json]

Each leg runs once unmeasured, then ``--repeats`` times: median [min .. max] seconds.  The upload of the dataset
(one PCIe crossing, which training needs anyway) is timed separately and reported as ``upload``.  There is no CPU
path for the device leg: without a GPU the script fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S, A, DEV, FRAC, DISCOUNT, MAX_LEN = 29, 8, "cuda:0", 0.1, 0.99, 1000


def data(n):
    """Sparse 0 / 1 rewards and goal-reached terminals as antmaze has them: many returns tie."""
    rng = np.random.default_rng(0)
    term = rng.uniform(size=n) < 1.0 / 400  # with the cut at 1000 rows: trajectories of 1 .. 1000 rows
    rew = np.where(term, 1.0, 0.0).astype(np.float32)
    return {"observations": rng.standard_normal((n, S), dtype=np.float32),
            "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "next_observations": rng.standard_normal((n, S), dtype=np.float32), "rewards": rew, "terminals": term}


def python_loop(dataset, frac, discount, max_episode_steps=1000):
    """The reference's loop and copies, restated (what the other two legs replace)."""
    ids_by_trajectories, returns, cur_ids, cur_return, reward_scale = [], [], [], 0, 1.0
    for i, (reward, done) in enumerate(zip(dataset["rewards"], dataset["terminals"])):
        cur_return += reward_scale * reward
        cur_ids.append(i)
        reward_scale *= discount
        if done == 1.0 or len(cur_ids) == max_episode_steps:
            ids_by_trajectories.append(list(cur_ids))
            returns.append(cur_return)
            cur_ids, cur_return, reward_scale = [], 0, 1.0
    sort_ord = np.argsort(returns, axis=0)[::-1].reshape(-1)
    order = []
    for i in sort_ord[: max(1, int(frac * len(sort_ord)))]:
        order += ids_by_trajectories[i]
    order = np.array(order)
    return {k: v[order] for k, v in dataset.items()}


def timed(run, repeats):
    run()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--loop_rows", type=int, default=100_000)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_offline_bc.py measures on a ROCm GPU; none is visible")
    from iqlpref_amd import _lib, offline_bc
    d = data(args.rows)
    legs = {}

    def upload():
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
        torch.cuda.synchronize()
        return dev
    legs["upload"] = timed(upload, args.repeats)
    dev = upload()
    kept = {}

    def device():
        sel, chosen = offline_bc.select_best_trajectories(*[dev[k] for k in offline_bc.ARRAYS], FRAC, DISCOUNT, MAX_LEN,
                                                          device=DEV)
        torch.cuda.synchronize()
        kept["device"] = (sel["rewards"].shape[0], len(chosen))
    legs["device_path"] = timed(device, args.repeats)

    def host():
        c = dict(d)
        offline_bc.keep_best_trajectories(c, FRAC, DISCOUNT, MAX_LEN)
        kept["host"] = (c["rewards"].shape[0],)
    legs["host_restatement"] = timed(host, args.repeats)

    part = {k: v[:args.loop_rows] for k, v in d.items()}
    scale = args.rows / args.loop_rows
    legs[f"python_loop_scaled_from_{args.loop_rows}_rows"] = [t * scale for t in timed(lambda: python_loop(part, FRAC, DISCOUNT),
                                                                                     args.repeats)]
    assert kept["device"][0] == kept["host"][0], kept
    out = {"rows": args.rows, "S": S, "A": A, "frac": FRAC, "max_len": MAX_LEN, "kept_rows": kept["device"][0],
           "kept_trajectories": kept["device"][1], "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "build_tag": _lib.build_tag()}
    for name, r in legs.items():
        out[name] = {"median_s": float(np.median(r)), "min_s": float(min(r)), "max_s": float(max(r))}
        print(f"{name:40s} {np.median(r) * 1e3:10.2f} ms  [{min(r) * 1e3:.2f} .. {max(r) * 1e3:.2f}]")
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
