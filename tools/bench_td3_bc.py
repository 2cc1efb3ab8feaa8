#!/usr/bin/env python3
"""Steps per second of the TD3+BC step (csrc/td3_bc_step.hip) at the halfcheetah shape -- S 17, A 6, batch 256,
hidden 256, policy_freq 2 -- for one seed and for groups of 8 and 16, and in the same run, on the same GPU and the
same data: an eager torch-ROCm run of the tests/td3_bc_cases.py restatement of the reference's ``train``
(algorithms/offline/td3_bc.py:324-380: its ``_net`` on device-resident parameters, F.mse_loss, three Adams, the target
formula) -- once with one ``.item()`` per logged loss as the reference logs them, once without any host sync, as the
TD3+BC legs run.

    python tools/bench_td3_bc.py [--steps 2000] [--warmup 300] [--repeats 5] [--only LEG] [--json out.json]

Every figure is a host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps of
the same shape; the indices are drawn and uploaded before the clock starts, the TD3+BC legs draw their noise on the
device.  Each leg is repeated ``--repeats`` times and printed as median [min .. max].  A group's rate is steps of ONE
member times members (seed-steps per second).  ``--only td3bc_one_seed`` runs that leg alone (for a kernel trace of
the launches).  There is no CPU path: without a GPU the script fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S, A, B, H, N_ROWS, DEV = 17, 6, 256, 256, 5000, "cuda:0"
DISCOUNT, TAU, ALPHA, POLICY_NOISE, NOISE_CLIP, POLICY_FREQ, MAX_ACTION = 0.99, 5e-3, 2.5, 0.2, 0.5, 2, 1.0


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


class Eager:
    """tdbc:285-380 in eager torch on the GPU with the arithmetic of tests/td3_bc_cases.py: its ``_net`` on parameter
    dicts that live on the device, ``F.mse_loss``, three ``torch.optim.Adam``, the target formula.  ``items``: one
    ``.item()`` per logged loss, as the reference logs them."""

    def __init__(self, items):
        from tests import td3_bc_cases as tc
        self.tc, self.items, self.total_it = tc, items, 0
        torch.manual_seed(0)
        named = lambda m: {"net." + k: torch.nn.Parameter(v.detach().clone().to(DEV)) for k, v in m.state_dict().items()}
        self.actor, self.c1, self.c2 = named(tc.mlp(S, H, A)), named(tc.mlp(S + A, H, 1)), named(tc.mlp(S + A, H, 1))
        self.targets = [({k: v.detach().clone() for k, v in n.items()}, n) for n in (self.actor, self.c1, self.c2)]
        adam = lambda p: torch.optim.Adam(list(p.values()), lr=3e-4)
        self.oa, self.o1, self.o2 = adam(self.actor), adam(self.c1), adam(self.c2)

    def train(self, s, a, r, s2, d):
        tc, F = self.tc, torch.nn.functional
        self.total_it += 1
        (at, _), (t1, _), (t2, _) = self.targets
        with torch.no_grad():
            noise = (torch.randn_like(a) * POLICY_NOISE).clamp(-NOISE_CLIP, NOISE_CLIP)
            a2 = (MAX_ACTION * torch.tanh(tc._net(at, s2)) + noise).clamp(-MAX_ACTION, MAX_ACTION)
            x2 = torch.cat([s2, a2], 1)
            y = r + (1 - d) * DISCOUNT * torch.min(tc._net(t1, x2), tc._net(t2, x2))
        x = torch.cat([s, a], 1)
        loss = F.mse_loss(tc._net(self.c1, x), y) + F.mse_loss(tc._net(self.c2, x), y)
        if self.items:
            loss.item()
        self.o1.zero_grad(), self.o2.zero_grad()
        loss.backward()
        self.o1.step(), self.o2.step()
        if self.total_it % POLICY_FREQ == 0:
            pi = MAX_ACTION * torch.tanh(tc._net(self.actor, s))
            q = tc._net(self.c1, torch.cat([s, pi], 1))
            lmbda = ALPHA / q.abs().mean().detach()
            loss = -lmbda * q.mean() + F.mse_loss(pi, a)
            if self.items:
                loss.item()
            self.oa.zero_grad()
            loss.backward()
            self.oa.step()
            with torch.no_grad():
                for t, n in self.targets:
                    for k in t:
                        t[k].copy_((1 - TAU) * t[k] + TAU * n[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="run this leg alone")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_td3_bc.py measures on a ROCm GPU; none is visible")
    from iqlpref_amd import td3_bc
    buf = td3_bc.ReplayBuffer(S, A, N_ROWS, DEV)
    buf.load_d4rl_dataset(data())
    n_idx = max(args.steps, args.warmup)
    idx = [torch.from_numpy(np.random.RandomState(k).randint(0, N_ROWS, size=(n_idx, B))).to(DEV) for k in range(16)]
    want = lambda leg: args.only in (None, leg)

    def trainer(seed):
        torch.manual_seed(seed)
        actor = td3_bc.Actor(S, A, MAX_ACTION, H).to(DEV)
        c1, c2 = td3_bc.Critic(S, A, H).to(DEV), td3_bc.Critic(S, A, H).to(DEV)
        adam = lambda m: torch.optim.Adam(m.parameters(), lr=3e-4)
        return td3_bc.TD3_BC(MAX_ACTION, actor, adam(actor), c1, adam(c1), c2, adam(c2), discount=DISCOUNT, tau=TAU,
                             policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, policy_freq=POLICY_FREQ, alpha=ALPHA,
                             device=DEV, seed=seed)

    legs = {}
    if want("td3bc_one_seed"):
        one = trainer(0)
        legs["td3bc_one_seed"] = timed(lambda n: one.train_steps(buf, n, B, indices=idx[0][:n], return_losses=False),
                                       args.steps, args.warmup, args.repeats)
    for K in (8, 16):
        if want(f"td3bc_{K}_seeds"):
            group = td3_bc.TD3BCGroup([trainer(k) for k in range(K)])
            rates = timed(lambda n: group.train_steps(buf, n, B, indices=[i[:n] for i in idx[:K]]), args.steps,
                          args.warmup, args.repeats)
            legs[f"td3bc_{K}_seeds"] = [K * r for r in rates]
            group.close()

    # the reference's train, eager, with and without the host syncs that its logging costs
    for leg, items in (("eager_torch_reference_train", True), ("eager_torch_no_item", False)):
        if want(leg):
            eager = Eager(items)

            def run_eager(n, eager=eager):
                for i in range(n):
                    rows = idx[0][i]
                    eager.train(buf._states[rows], buf._actions[rows], buf._rewards[rows], buf._next_states[rows],
                                buf._dones[rows])
            legs[leg] = timed(run_eager, args.steps, args.warmup, args.repeats)

    out = {"shape": {"S": S, "A": A, "B": B, "H": H, "policy_freq": POLICY_FREQ}, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for name, r in legs.items():
        out[name] = {"median": float(np.median(r)), "min": float(min(r)), "max": float(max(r))}
        print(f"{name:30s} {np.median(r):10.0f} steps/s  [{min(r):.0f} .. {max(r):.0f}]")
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
