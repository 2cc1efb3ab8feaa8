#!/usr/bin/env python3
"""The BB flavour's evaluation: the numpy simulator (bb_run_eval_IQL) against the device rollout
(bb_run_eval_device, a launch pair per step) and the fused rollout (bb_run_eval_fused, one launch per episode),
same actor, same preference transformer, same seed; and ``--group`` K actors evaluated side by side
(bb_run_eval_fused_group) against the same K evaluated one after the other (K bb_run_eval_fused calls).

    python tools/bench_bb_eval.py [--episodes 10] [--horizon 500] [--hidden 256] [--repeats 5] [--warmup 1]
                                  [--group 8] [--no-host]

Synthetic BB shapes: state 26, action 2, a fresh Gaussian actor of ``--hidden`` units (its tanh output keeps the
heading within +-1 degree and the speed under the clamp: it does not reach a goal 30 away within the horizon
unless that lies due east), the default preference transformer (embd 64, one block, 4 heads, MLP 256),
context 100.  One evaluation = ``--episodes`` episodes.  Every timed evaluation ends in a device
synchronisation; ``--warmup`` untimed evaluations of each path come first, then ``--repeats`` timed ones of
each path, alternated.  Prints one JSON line: median (and min / max) seconds per evaluation and microseconds
per simulated step for both paths, the ratio of the medians, and the device path's split into set-up and
upload / step loop / reward call from a further run that synchronises between the phases (so the split adds
up to a slightly longer evaluation than the unsplit one); the same for the fused path.  ``fused_beats_device``:
the fused median lies below the device median by more than the min-max spread of either path in this run;
``group_beats_serial``: the group median lies below K times the solo fused median by more than the spread of the
group leg or K times that of the solo leg.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iqlpref_amd import _lib, custom_offline_bb as bb  # noqa: E402
from iqlpref_amd.relabel import RewardPT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--context", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--group", type=int, default=8, help="members of the group leg (0: no group leg)")
    ap.add_argument("--no-host", action="store_true", help="leave the numpy path out")
    args = ap.parse_args()
    dev, S, A = "cuda:0", 26, 2
    _lib.require_gpu(dev)
    torch.manual_seed(0)
    hi, lo = torch.tensor([0.8, 180.0], device=dev), torch.tensor([0.0, -180.0], device=dev)
    actor = bb.GaussianPolicy(S, A, hi, lo, hidden_dim=args.hidden).to(dev)
    pt = RewardPT(S, A, args.horizon).to(dev)
    ctx = bb.RewardPTContext(pt, args.context)
    rng = np.random.default_rng(0)
    mean = np.concatenate([rng.uniform(-5, 5, S - 4), np.zeros(4)])
    std = np.concatenate([rng.uniform(20, 35, S - 4), np.ones(4)])
    move_stats = (0.9, 0.2, 0.35, 0.1)
    kw = dict(num_episodes=args.episodes, move_stats=move_stats, state_mean=mean, state_std=std,
              max_horizon=args.horizon, context_length=args.context, seed=args.seed, device=dev)

    def host():
        return bb.bb_run_eval_IQL(actor, r_model=ctx, **kw)

    def device(record=None):
        return bb.bb_run_eval_device(actor, r_model=ctx, chunk=args.chunk, record=record, **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def fused(record=None):
        return bb.bb_run_eval_fused(actor, r_model=ctx, record=record, **kw)

    K = args.group
    members = [actor] + [bb.GaussianPolicy(S, A, hi, lo, hidden_dim=args.hidden).to(dev) for _ in range(K - 1)]
    gkw = {k: v for k, v in kw.items() if k != "seed"}

    def group(record=None):
        return bb.bb_run_eval_fused_group(members, r_model=ctx, seeds=[args.seed + k for k in range(K)],
                                          record=record, **gkw)

    def serial():
        return [bb.bb_run_eval_fused(m, r_model=ctx, **dict(kw, seed=args.seed + k)) for k, m in enumerate(members)]

    paths = {"device": device, "fused": fused}
    if not args.no_host:
        paths["host"] = host
    if K:
        paths.update(group=group, serial=serial)
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    times, last = {name: [] for name in paths}, {}
    for _ in range(args.repeats):
        for name, fn in paths.items():
            t, last[name] = timed(fn)
            times[name].append(t)
    rh, rd = last.get("host", last["device"]), last["device"]
    rec, frec = {"timing": {}}, {"timing": {}}
    device(rec)
    fused(frec)
    steps = sum(e["length"] for e in rec["episodes"])
    split = {k: rec["timing"].get(k, 0.0) for k in ("setup", "steps", "reward")}
    fsplit = {k: frec["timing"].get(k, 0.0) for k in ("setup", "steps", "reward")}

    def stats(xs):
        return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs),
                "us_per_step": statistics.median(xs) / steps * 1e6}

    med = lambda name: statistics.median(times[name])
    spread = lambda name: max(times[name]) - min(times[name])
    out = {"episodes": args.episodes, "horizon": args.horizon, "hidden": args.hidden, "context": args.context,
           "chunk": args.chunk, "simulated_steps": steps, "repeats": args.repeats,
           "device": stats(times["device"]), "fused": stats(times["fused"]),
           "device_over_fused": med("device") / med("fused"),
           "fused_beats_device": bool(med("device") - med("fused") > max(spread("device"), spread("fused"))),
           "fused_equals_device": bool(last["fused"].tobytes() == rd.tobytes()),
           "device_split_s": split, "device_split_us_per_step": {k: v / steps * 1e6 for k, v in split.items()},
           "fused_split_s": fsplit, "fused_split_us_per_step": {k: v / steps * 1e6 for k, v in fsplit.items()},
           "max_return_difference": float(np.abs(rh - rd).max()),
           "build_tag": _lib.build_tag(), "gpu": torch.cuda.get_device_name(0)}
    if "host" in times:
        out.update(host=stats(times["host"]), host_over_device=med("host") / med("device"))
    if K:
        grec = {"timing": {}}
        group(grec)
        gsteps = sum(e["length"] for m in grec["members"] for e in m["episodes"])
        gstats = lambda xs: {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs),
                             "us_per_step": statistics.median(xs) / gsteps * 1e6}
        out.update(group_members=K, group_simulated_steps=gsteps, group=gstats(times["group"]),
                   serial=gstats(times["serial"]), k_times_solo_fused_s=K * med("fused"),
                   k_solo_over_group=K * med("fused") / med("group"), serial_over_group=med("serial") / med("group"),
                   group_beats_serial=bool(K * med("fused") - med("group") > max(spread("group"), K * spread("fused"))),
                   group_equals_serial=bool(all(a.tobytes() == b.tobytes() for a, b in zip(last["group"], last["serial"]))),
                   group_split_s={k: grec["timing"].get(k, 0.0) for k in ("setup", "steps", "reward")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
