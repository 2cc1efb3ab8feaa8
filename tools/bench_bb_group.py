"""Seed groups on the BB flavour's shape (S 26 / A 2 / H 256 / B 256, fp32, convex Polyak): seed-steps/s of the
epoch walk of a 100,000-row dataset (390 whole blocks and a tail of 160 rows per epoch) for K = 1, 2, 4, 8, 16
seeds on one GPU, three legs per K, alternated within every repetition:

  lone     ONE trainer's train_epoch_steps (the same leg for every K: the spread of the run);
  counted  a SeedGroup of K stepped with the K index arrays and the shared count array of
           BlockEpochSamplerGroup (what custom_offline_bb.train(seeds_per_gpu=K) queues);
  plain    the same group, the same index arrays, no counts (plain SeedGroup.train_steps).

Host clock around synchronised runs of 5 chunks of 2000 steps; every leg is warmed up first.  The last line is
one JSON object with the median of the repetitions per (K, leg) and the library's build tag.

    python tools/bench_bb_group.py [--mode group|split|streams] [--reps 3] [--out FILE.json]
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
import iqlpref_amd as ia  # noqa: E402
from iqlpref_amd import _lib  # noqa: E402
from iqlpref_amd import custom_offline_bb as bb  # noqa: E402

DEV, S, A, B, N, CHUNK, CHUNKS = "cuda:0", 26, 2, 256, 100_000, 2000, 5


def make_trainer(seed):
    torch.manual_seed(seed)
    hi, lo = torch.tensor([1.0, 180.0], device=DEV), torch.tensor([0.0, -180.0], device=DEV)
    q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), bb.GaussianPolicy(S, A, hi, lo).to(DEV)
    ao = torch.optim.Adam(actor.parameters(), lr=3e-4)
    return bb.ImplicitQLearning(hi, lo, actor, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 10 ** 6), q,
                                torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                                device=DEV, seed=seed)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", default=None, choices=("group", "split", "streams"),
                    help="SeedGroup mode (default: the SeedGroup default, as train() uses)")
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args(argv)
    _lib.require_gpu(DEV)

    rng = np.random.default_rng(0)
    buf = bb.ReplayBuffer(S, A, N, DEV)
    buf.load_dataset({"observations": rng.standard_normal((N, S)).astype(np.float32),
                      "actions": rng.uniform(-1, 1, (N, A)).astype(np.float32),
                      "rewards": rng.standard_normal(N).astype(np.float32),
                      "next_observations": rng.standard_normal((N, S)).astype(np.float32),
                      "terminals": (rng.uniform(size=N) < 0.02).astype(np.float32)})
    lone, lone_sampler = make_trainer(1000), bb.BlockEpochSampler(N, B, generator=torch.Generator().manual_seed(1000))
    result = {"build_tag": _lib.build_tag(), "shape": {"S": S, "A": A, "H": 256, "B": B, "rows": N, "precision": "fp32"},
              "steps_per_leg": CHUNK * CHUNKS, "reps": args.reps, "seed_steps_per_s": {}}
    for K in args.seeds:
        trainers = [make_trainer(k) for k in range(K)]
        group = ia.SeedGroup(trainers, mode=args.mode)
        samplers = bb.BlockEpochSamplerGroup.draw(N, B, K)

        def counted(t):
            idx, valid = samplers.device_indices(t, CHUNK, DEV)
            group.train_steps(buf, CHUNK, B, indices=idx, n_valid=valid)

        def plain(t):
            idx, _ = samplers.device_indices(t, CHUNK, DEV)
            group.train_steps(buf, CHUNK, B, indices=idx)

        legs = {"lone": (1, lambda t: lone.train_epoch_steps(buf, lone_sampler, t, CHUNK)),
                "counted": (K, counted), "plain": (K, plain)}
        for _, leg in legs.values():  # warm-up: every path once (graphs are captured here)
            leg(0)
        group.synchronize()
        rates = {name: [] for name in legs}
        for rep in range(args.reps):
            for name, (width, leg) in legs.items():
                t0 = time.perf_counter()
                for c in range(CHUNKS):
                    leg(c * CHUNK)
                group.synchronize()
                dt = time.perf_counter() - t0
                rates[name].append(width * CHUNKS * CHUNK / dt)
                print(f"K {K:2d} ({group.mode}) rep {rep} {name:>8}: {rates[name][-1]:9.0f} seed-steps/s  "
                      f"{dt / (CHUNKS * CHUNK) * 1e6:7.2f} us/launch sequence", flush=True)
        result["seed_steps_per_s"][str(K)] = {
            "mode": group.mode,
            **{name: {"median": statistics.median(r), "min": min(r), "max": max(r)} for name, r in rates.items()}}
        group.close()
        del group, trainers
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
