#!/usr/bin/env python3
"""Steps per second of the behaviour-cloning step (csrc/bc_step.hip) at the pen shape -- S 45, A 24, batch 256 --
for one seed and for a group of 8, and in the same run, on the same GPU and the same data: an eager torch-ROCm
restatement of the reference's step (algorithms/minari/any_percent_bc.py:230-243: Actor, F.mse_loss, Adam; one
loss.item() per step as there) and the IQL fp32 step at the same shape (``custom_offline.ImplicitQLearning``).

    python tools/bench_bc.py [--steps 4000] [--warmup 500] [--repeats 5] [--json out.json]

Every figure is a host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps of
the same shape; the indices are drawn and uploaded before the clock starts.  Each leg is repeated ``--repeats`` times
and printed as median [min .. max].  A group's rate is steps of ONE member times members (seed-steps per second).
There is no CPU path: without a GPU the script fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S, A, B, N_ROWS, DEV = 45, 24, 256, 5000, "cuda:0"


def data():
    rng = np.random.default_rng(0)
    return {"observations": rng.standard_normal((N_ROWS, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (N_ROWS, A)).astype(np.float32),
            "rewards": rng.standard_normal(N_ROWS).astype(np.float32),
            "next_observations": rng.standard_normal((N_ROWS, S)).astype(np.float32),
            "terminals": (rng.uniform(size=N_ROWS) < 0.05).astype(np.float32)}


def timed(run, steps, warmup, repeats):
    run(warmup)
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bc.py measures on a ROCm GPU; none is visible")
    import iqlpref_amd as ia
    from iqlpref_amd import custom_offline as co, minari_bc
    buf = co.ReplayBuffer(S, A, N_ROWS, DEV)
    buf.load_dataset(data())
    n_idx = max(args.steps, args.warmup)
    idx = [torch.from_numpy(np.random.RandomState(k).randint(0, N_ROWS, size=(n_idx, B))).to(DEV) for k in range(8)]

    def bc_trainer(seed):
        torch.manual_seed(seed)
        actor = minari_bc.Actor(S, A, 1.0).to(DEV)
        return minari_bc.BC(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), DEV)

    legs = {}
    one = bc_trainer(0)
    legs["bc_one_seed"] = timed(lambda n: one.train_steps(buf, n, B, indices=idx[0][:n], return_losses=False),
                                args.steps, args.warmup, args.repeats)
    group = minari_bc.BCGroup([bc_trainer(k) for k in range(8)])
    rates = timed(lambda n: group.train_steps(buf, n, B, indices=[i[:n] for i in idx]), args.steps, args.warmup,
                  args.repeats)
    legs["bc_eight_seeds"] = [8 * r for r in rates]
    group.close()

    # the reference's step, eager: the same modules and optimiser on the GPU, rows gathered by the same indices
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(S, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, A), torch.nn.Tanh()).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)

    def eager(n):
        for i in range(n):
            rows = idx[0][i]
            loss = torch.nn.functional.mse_loss(1.0 * net(buf._states[rows]), buf._actions[rows])
            loss.item()  # (the reference logs every step's loss)
            opt.zero_grad()
            loss.backward()
            opt.step()
    legs["eager_torch_reference_step"] = timed(eager, args.steps, args.warmup, args.repeats)

    torch.manual_seed(0)
    q, v, pol = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), ia.GaussianPolicy(S, A, 1.0).to(DEV)
    ao = torch.optim.Adam(pol.parameters(), lr=3e-4)
    iql = co.ImplicitQLearning(1.0, pol, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 10 ** 6), q,
                               torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                               device=DEV, seed=0)
    legs["iql_fp32_one_seed"] = timed(lambda n: iql.train_steps(buf, n, B, indices=idx[0][:n], return_losses=False),
                                      args.steps, args.warmup, args.repeats)

    out = {"shape": {"S": S, "A": A, "B": B}, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0)}
    for name, r in legs.items():
        out[name] = {"median": float(np.median(r)), "min": float(min(r)), "max": float(max(r))}
        print(f"{name:28s} {np.median(r):10.0f} steps/s  [{min(r):.0f} .. {max(r):.0f}]")
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
