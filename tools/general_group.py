"""Aggregate throughput of K general-step trainers in a SeedGroup, one JSON line per (shape, K, variant):

    python tools/general_group.py --shapes 3x256,1x256 --ks 1,2,4,8 --variants streams,general:0,general:50
    python tools/general_group.py H N_HIDDEN B K [--variants ...]        (one shape, one K)

A variant is MODE[:GRAPH_UNROLL]: a SeedGroup mode ("streams", "general"; graph_unroll default: the
mode's own) or "solo" (the first trainer alone, K ignored).  Per variant: a warm-up, then --repeats
timed regions of at least --min_seconds each (host clock around work that ends in a device
synchronise); the line holds the median, minimum and maximum of total steps/s and, where the build
has them, launch_counts().  --root DIR imports iqlpref_amd from another checkout (the parent commit's
export with its own library: the baseline of an A/B) -- such a build may lack the newer modes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("dims", nargs="*", type=int, help="H N_HIDDEN B K")
ap.add_argument("--shapes", default=None, help="comma-separated N_HIDDENxH, e.g. 3x256,2x512")
ap.add_argument("--ks", default=None, help="comma-separated group sizes")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--variants", default="streams,general:0,general:50")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.25)
ap.add_argument("--root", default=None)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import bench  # noqa: E402
if args.root:
    sys.path.insert(0, os.path.abspath(args.root))
import iqlpref_amd as ia  # noqa: E402

if args.dims:
    H, NH, B, K = args.dims
    shapes, ks = [(NH, H)], [K]
else:
    B = args.batch
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
dev = "cuda:0"
buf = ia.ReplayBuffer(bench.S_DIM, bench.A_DIM, 200_000, dev)
buf.load_d4rl_dataset(bench.synth_dataset(1, 200_000))
tag = ia._lib.build_tag()


def timed(step, sync, n):
    t0 = time.perf_counter()
    step(n)
    sync()
    return time.perf_counter() - t0


for NH, H in shapes:
    for K in ks:
        for variant in args.variants.split(","):
            mode, _, unroll = variant.partition(":")
            unroll = int(unroll) if unroll else None
            if mode == "solo" and K != ks[0]:
                continue
            trs = [bench.build_trainer(ia, torch, dev, 1 + k, "bf16", hidden_dim=H, n_hidden=NH)
                   for k in range(1 if mode == "solo" else K)]
            if mode == "solo":
                g, n_tr = trs[0], 1
                step = lambda n: g.train_steps(buf, n, B, return_losses=False, graph_unroll=unroll)
                sync = torch.cuda.synchronize
            else:
                g, n_tr = ia.SeedGroup(trs, mode=mode), K
                step = lambda n: g.train_steps(buf, n, B, return_losses=False, graph_unroll=unroll)
                sync = g.synchronize
            timed(step, sync, 300)  # warm-up: code objects, graph capture, pinned slots
            n = 300
            while True:  # steps per region: at least min_seconds of work
                dt = timed(step, sync, n)
                if dt >= args.min_seconds:
                    break
                n = int(n * max(1.5, 1.2 * args.min_seconds / dt)) + 1
            rates = [n_tr * n / timed(step, sync, n) for _ in range(args.repeats)]
            rec = {"tag": args.tag, "build": tag, "variant": variant, "mode": getattr(g, "mode", "solo"),
                   "kind": trs[0].step_kind(B), "n_hidden": NH, "H": H, "B": B, "K": n_tr, "steps_per_region": n,
                   "steps_per_s_total": statistics.median(rates), "min": min(rates), "max": max(rates)}
            if hasattr(g, "launch_counts") and mode != "streams":
                rec["launch_counts"] = list(g.launch_counts())
            print(json.dumps(rec), flush=True)
            if mode != "solo":
                g.close()
            del g, trs
