"""Host vs device numpy index sampling for the custom flavour's fp32 step (pen shape: S 45, A 24, H 256,
B 256), in chunks of 2000 steps, at K = 1 (one trainer) and K = 8 (one SeedGroup).

    python tools/custom_sampler_bench.py [--K 1 8] [--chunks 5] [--samplers host device]

"host": every chunk draws K x [2000][256] indices with numpy's legacy randint and uploads them
(ReplayBuffer.draw_indices); "device": one NumpyIndexStream launch draws all K streams.  One JSON
line per (K, sampler) with steps/s (summed over the K seeds).  The draw kernel's own time comes from a
run of its own under rocprofv3, e.g.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/custom_sampler_bench.py --K 8 --samplers device --chunks 3
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
from iqlpref_amd import custom_offline as co  # noqa: E402
from iqlpref_amd.multi import SeedGroup  # noqa: E402

DEV = "cuda:0"
S, A, B = 45, 24, 256


def make_buffer(n_rows):
    rng = np.random.default_rng(0)
    buf = co.ReplayBuffer(S, A, n_rows, DEV)
    buf.load_dataset({"observations": rng.standard_normal((n_rows, S), dtype=np.float32),
                      "actions": rng.uniform(-1, 1, (n_rows, A)).astype(np.float32),
                      "rewards": rng.standard_normal(n_rows, dtype=np.float32),
                      "next_observations": rng.standard_normal((n_rows, S), dtype=np.float32),
                      "terminals": (rng.uniform(size=n_rows) < 0.01).astype(np.float32)})
    return buf


def make_trainer(seed):
    torch.manual_seed(seed)
    q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), ia.GaussianPolicy(S, A, 1.0).to(DEV)
    ao = torch.optim.Adam(actor.parameters(), lr=3e-4)
    return co.ImplicitQLearning(1.0, actor, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 10 ** 6), q,
                                torch.optim.Adam(q.parameters(), lr=3e-4), v,
                                torch.optim.Adam(v.parameters(), lr=3e-4), device=DEV, seed=seed)


def run(buf, K, sampler, chunks, chunk, warmup):
    trainers = [make_trainer(k) for k in range(K)]
    group = SeedGroup(trainers) if K > 1 else None
    gens = [np.random.RandomState(100 + k) for k in range(K)]
    stream = co.NumpyIndexStream(DEV)
    pending = []

    def one():
        if sampler == "host":
            idx = [torch.from_numpy(buf.draw_indices(B, chunk, rng=g)).to(DEV) for g in gens]
        else:
            idx = stream.draw(buf.index_bound(), chunk, B, gens)
        if group is None:
            losses = [trainers[0].train_steps(buf, chunk, B, indices=idx[0])]
        else:
            losses = group.train_steps(buf, chunk, B, indices=idx, return_losses=True)
        if pending:  # the previous chunk's losses come back once it is done, as in custom_offline.train
            [l.cpu() for l in pending.pop()]
        pending.append(losses)

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(chunks):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if group is not None:
        group.close()
    return K * chunks * chunk / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--samplers", nargs="+", default=["host", "device"])
    ap.add_argument("--chunks", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=496113)
    args = ap.parse_args()
    buf = make_buffer(args.rows)
    # the host draw alone, for scale (no GPU involved)
    t0 = time.perf_counter()
    buf.draw_indices(B, args.chunk, rng=np.random.RandomState(0))
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"host_draw_ms_per_chunk": round(host_ms, 2), "chunk": args.chunk, "batch": B,
                      "rows": args.rows}), flush=True)
    for K in args.K:
        for sampler in args.samplers:
            sps = run(buf, K, sampler, args.chunks, args.chunk, args.warmup)
            print(json.dumps({"K": K, "sampler": sampler, "steps_per_s": round(sps, 1),
                              "chunks": args.chunks, "chunk": args.chunk}), flush=True)


if __name__ == "__main__":
    main()
