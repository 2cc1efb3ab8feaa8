#!/usr/bin/env python3
"""Cost of one online fine-tuning tick (iqlpref_amd.finetune) with a null environment.

    python tools/bench_finetune.py [--ticks 2000] [--warmup 200] [--batch 256] [--rows 100000] [--seeds K]

A tick is what ``finetune.train`` does per online step: ``explore_action`` and its copy to the host (the
environment needs the action), ``add_transition``, one ``train_steps(n_steps=1)`` on pre-drawn indices.  The
environment is null: the next state is a fixed array.  Prints one JSON line: microseconds per tick, its split
into act / append / step (each timed on the host around its own call, with a device synchronisation after the
step so that the three add up to the tick), and beside them the microseconds of a bare ``train_steps(n_steps=1)``
call in a loop on the same trainer -- the floor the tick cannot go under.

``--seeds K`` (K > 1) times the tick of ``finetune.train(seeds_per_gpu=K)`` instead: ``explore_actions`` and its
one copy to the host, ``add_transitions``, one ``SeedGroup.train_steps(n_steps=1)`` on K rings -- the same three
parts, each once for all K members.  ``seed_ticks_per_s`` = K / tick.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import iqlpref_amd as ia  # noqa: E402
from iqlpref_amd import _lib, finetune as ft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--state-dim", type=int, default=17)
    ap.add_argument("--action-dim", type=int, default=6)
    ap.add_argument("--seeds", type=int, default=1)
    args = ap.parse_args()
    dev, S, A, B, K = "cuda:0", args.state_dim, args.action_dim, args.batch, args.seeds
    total = args.warmup + args.ticks
    rng = np.random.default_rng(0)
    data = {"observations": rng.standard_normal((args.rows, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (args.rows, A)).astype(np.float32),
            "rewards": rng.standard_normal(args.rows).astype(np.float32),
            "next_observations": rng.standard_normal((args.rows, S)).astype(np.float32),
            "terminals": (rng.uniform(size=args.rows) < 0.01).astype(np.float32)}
    trs, bufs = [], []
    for k in range(K):
        torch.manual_seed(k)
        q, v, actor = ia.TwinQ(S, A).to(dev), ia.ValueFunction(S).to(dev), ia.GaussianPolicy(S, A, 1.0).to(dev)
        trs.append(ft.ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), q,
                                        torch.optim.Adam(q.parameters(), lr=3e-4), v,
                                        torch.optim.Adam(v.parameters(), lr=3e-4), max_steps=10 ** 6, device=dev, seed=k))
        bufs.append(ft.ReplayBuffer(S, A, args.rows + total // 2, dev))  # (the ring fills half way through: both regimes)
        bufs[k].load_d4rl_dataset(data)
    # the three calls of a tick, as finetune.train picks them: one seed on its own entry points, K > 1 grouped
    if K == 1:
        np.random.seed(0)
        gens, group = None, None
        act = lambda states: trs[0].explore_action(states, None, batch_size=B).cpu().numpy()
        append = lambda s, a, r, s2, d: bufs[0].add_transition(s[0], a[0], r[0], s2[0], d[0])
        step = lambda indices: trs[0].train_steps(bufs[0], 1, B, indices=indices[0], return_losses=False)
    else:
        from iqlpref_amd.multi import SeedGroup
        gens = [np.random.RandomState(k) for k in range(K)]
        group = SeedGroup(trs, mode="group")  # (what finetune.train steps its members with)
        act = lambda states: ft.explore_actions(trs, states, None, expl_noise=0.03, noise_clip=0.5,
                                                batch_size=B).cpu().numpy()
        append = lambda *transitions: ft.add_transitions(bufs, *transitions)
        step = lambda indices: group.train_steps(bufs, 1, B, indices=indices, return_losses=False)
    cap = bufs[0]._buffer_size
    idx = ft.GrowingIndexStream(dev).draw(min(bufs[0].index_bound() + 1, cap), cap, total, B, generators=gens)
    states = rng.standard_normal((K, S))
    nxt = list(rng.standard_normal((K, S)))
    rewards, dones = [0.5] * K, [False] * K
    t_act = t_app = t_step = 0.0
    for i in range(total):
        if i == args.warmup:
            torch.cuda.synchronize()
            t_act = t_app = t_step = 0.0
        t0 = time.perf_counter()
        actions = act(states)
        t1 = time.perf_counter()
        append(states, actions, rewards, nxt, dones)
        t2 = time.perf_counter()
        step([x[i:i + 1] for x in idx])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_act, t_app, t_step = t_act + t1 - t0, t_app + t2 - t1, t_step + t3 - t2
    # the floor: the same call with nothing around it (the device queue never runs dry: no sync inside)
    floor_idx = [x[:1] for x in idx]
    for _ in range(args.warmup):
        step(floor_idx)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.ticks):
        step(floor_idx)
    torch.cuda.synchronize()
    floor = (time.perf_counter() - t0) / args.ticks
    us = lambda x: round(1e6 * x / args.ticks, 2)
    tick = (t_act + t_app + t_step) / args.ticks
    print(json.dumps({"tool": "bench_finetune", "build_tag": _lib.build_tag(), "seeds": K, "ticks": args.ticks, "batch": B,
                      "state_dim": S, "action_dim": A, "tick_us": us(t_act + t_app + t_step), "act_us": us(t_act),
                      "append_us": us(t_app), "step_us": us(t_step), "bare_train_step_us": round(1e6 * floor, 2),
                      "seed_ticks_per_s": round(K / tick, 1)}))
    if group is not None:
        group.close()


if __name__ == "__main__":
    main()
