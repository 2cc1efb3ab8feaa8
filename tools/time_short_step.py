"""What a per-step valid-row count costs on the BB flavour's shape (S 26 / A 2 / H 256 / B 256, fp32, convex
Polyak): steps/s of 2000-step chunks with injected indices, (a) no counts, (b) counts all equal to the
batch, (c) every step short (100 of 256 rows), (d) the epoch walk of a 100,000-row dataset (390 whole
blocks and a tail of 160 rows per epoch) through train_epoch_steps.  Host clock around synchronised chunks."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iqlpref_amd as ia  # noqa: E402
from iqlpref_amd import custom_offline_bb as bb  # noqa: E402

DEV, S, A, B, N, CHUNK = "cuda:0", 26, 2, 256, 100_000, 2000
rng = np.random.default_rng(0)
data = {"observations": rng.standard_normal((N, S)).astype(np.float32),
        "actions": rng.uniform(-1, 1, (N, A)).astype(np.float32),
        "rewards": rng.standard_normal(N).astype(np.float32),
        "next_observations": rng.standard_normal((N, S)).astype(np.float32),
        "terminals": (rng.uniform(size=N) < 0.02).astype(np.float32)}
buf = bb.ReplayBuffer(S, A, N, DEV)
buf.load_dataset(data)
torch.manual_seed(0)
hi, lo = torch.tensor([1.0, 180.0], device=DEV), torch.tensor([0.0, -180.0], device=DEV)
q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), bb.GaussianPolicy(S, A, hi, lo).to(DEV)
ao = torch.optim.Adam(actor.parameters(), lr=3e-4)
tr = bb.ImplicitQLearning(hi, lo, actor, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 10 ** 6), q,
                          torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                          device=DEV, seed=0)
idx = torch.from_numpy(rng.integers(0, N, (CHUNK, B))).to(DEV)
full = torch.full((CHUNK,), B, dtype=torch.int32, device=DEV)
short = torch.full((CHUNK,), 100, dtype=torch.int32, device=DEV)
sampler = bb.BlockEpochSampler(N, B)
legs = {"no counts": lambda t: tr.train_steps(buf, CHUNK, B, indices=idx, return_losses=False),
        "counts == batch": lambda t: tr.train_steps(buf, CHUNK, B, indices=idx, n_valid=full, return_losses=False),
        "every step 100 rows": lambda t: tr.train_steps(buf, CHUNK, B, indices=idx, n_valid=short, return_losses=False),
        "epoch walk": lambda t: tr.train_epoch_steps(buf, sampler, t, CHUNK)}
for leg in legs.values():  # warm-up: every path once
    leg(0)
torch.cuda.synchronize()
for rep in range(3):
    for name, leg in legs.items():
        t0 = time.perf_counter()
        for c in range(5):
            leg(c * CHUNK)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"rep {rep} {name:>20}: {5 * CHUNK / dt:9.0f} steps/s  {dt / (5 * CHUNK) * 1e6:6.2f} us/step", flush=True)
