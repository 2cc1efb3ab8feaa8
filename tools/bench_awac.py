#!/usr/bin/env python3
"""Steps per second of the AWAC step (csrc/awac_step.hip) at the halfcheetah shape -- S 17, A 6, batch 256, hidden
256 -- for one seed and for groups of 8 and 16, and in the same run, on the same GPU and the same data: an eager
torch-ROCm run of the tests/awac_cases.py restatement of the reference's update (algorithms/offline/awac.py:248-310:
its ``_net`` / ``_sample`` on device-resident parameters, F.mse_loss, torch.distributions.Normal, three Adams, the
target formula) -- once with one ``.item()`` per loss as the reference logs them, once without any host sync, as
the AWAC legs run -- and, for scale, this package's general IQL fp32 step at ``n_hidden=3``.

    python tools/bench_awac.py [--steps 2000] [--warmup 300] [--repeats 5] [--only LEG] [--json out.json]

Every figure is a host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps of
the same shape; the indices are drawn and uploaded before the clock starts, the AWAC legs draw their noise on the
device.  Each leg is repeated ``--repeats`` times and printed as median [min .. max].  A group's rate is steps of
ONE member times members (seed-steps per second).  ``--only awac_one_seed`` runs that leg alone (for a kernel
trace of the four launches).  There is no CPU path: without a GPU the script fails.
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
GAMMA, TAU, LAMBDA, EXP_ADV_MAX = 0.99, 5e-3, 1.0, 100.0


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
    """awac:218-310 in eager torch on the GPU with the arithmetic of tests/awac_cases.py: its ``_net`` and
    ``_sample`` on parameter dicts that live on the device, ``F.mse_loss``, ``Normal.log_prob``, three
    ``torch.optim.Adam``, the target formula.  ``items``: one ``.item()`` per loss, as the reference logs them."""

    def __init__(self, items):
        from tests import awac_cases as ac
        self.ac, self.items = ac, items
        torch.manual_seed(0)
        named = lambda m: {"_mlp." + k: torch.nn.Parameter(v.detach().clone().to(DEV)) for k, v in m.state_dict().items()}
        self.actor, self.c1, self.c2 = named(ac.mlp(S, H, A)), named(ac.mlp(S + A, H, 1)), named(ac.mlp(S + A, H, 1))
        self.actor["_log_std"] = torch.nn.Parameter(torch.zeros(A, device=DEV))
        self.t1 = {k: v.detach().clone() for k, v in self.c1.items()}
        self.t2 = {k: v.detach().clone() for k, v in self.c2.items()}
        adam = lambda p: torch.optim.Adam(list(p.values()), lr=3e-4)
        self.oa, self.o1, self.o2 = adam(self.actor), adam(self.c1), adam(self.c2)

    def update(self, s, a, r, s2, d):
        ac, F = self.ac, torch.nn.functional
        with torch.no_grad():
            a2, _ = ac._sample(self.actor, s2, torch.randn((B, A), device=DEV))
            x2 = torch.cat([s2, a2], -1)
            y = r + GAMMA * (1.0 - d) * torch.min(ac._net(self.t1, x2), ac._net(self.t2, x2))
        x = torch.cat([s, a], -1)
        loss = F.mse_loss(ac._net(self.c1, x), y) + F.mse_loss(ac._net(self.c2, x), y)
        self.o1.zero_grad(), self.o2.zero_grad()
        loss.backward()
        self.o1.step(), self.o2.step()
        if self.items:
            loss.item()
        with torch.no_grad():
            pi, _ = ac._sample(self.actor, s, torch.randn((B, A), device=DEV))
            xp = torch.cat([s, pi], -1)
            adv = torch.min(ac._net(self.c1, x), ac._net(self.c2, x)) - torch.min(ac._net(self.c1, xp), ac._net(self.c2, xp))
            w = torch.clamp_max(torch.exp(adv / LAMBDA), EXP_ADV_MAX)
        policy = torch.distributions.Normal(ac._net(self.actor, s), self.actor["_log_std"].clamp(-20.0, 2.0).exp())
        loss = (-policy.log_prob(a).sum(-1, keepdim=True) * w).mean()
        self.oa.zero_grad()
        loss.backward()
        self.oa.step()
        if self.items:
            loss.item()
        with torch.no_grad():
            for t, c in ((self.t1, self.c1), (self.t2, self.c2)):
                for k in t:
                    t[k].copy_((1 - TAU) * t[k] + TAU * c[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="run this leg alone")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_awac.py measures on a ROCm GPU; none is visible")
    import iqlpref_amd as ia
    from iqlpref_amd import awac, custom_offline as co
    buf = awac.ReplayBuffer(S, A, N_ROWS, DEV)
    buf.load_d4rl_dataset(data())
    n_idx = max(args.steps, args.warmup)
    idx = [torch.from_numpy(np.random.RandomState(k).randint(0, N_ROWS, size=(n_idx, B))).to(DEV) for k in range(16)]
    want = lambda leg: args.only in (None, leg)

    def trainer(seed):
        torch.manual_seed(seed)
        actor, c1, c2 = awac.Actor(S, A, H).to(DEV), awac.Critic(S, A, H).to(DEV), awac.Critic(S, A, H).to(DEV)
        adam = lambda m: torch.optim.Adam(m.parameters(), lr=3e-4)
        return awac.AdvantageWeightedActorCritic(actor, adam(actor), c1, adam(c1), c2, adam(c2), gamma=GAMMA, tau=TAU,
                                                 awac_lambda=LAMBDA, seed=seed)

    legs = {}
    if want("awac_one_seed"):
        one = trainer(0)
        legs["awac_one_seed"] = timed(lambda n: one.train_steps(buf, n, B, indices=idx[0][:n], return_losses=False),
                                      args.steps, args.warmup, args.repeats)
    for K in (8, 16):
        if want(f"awac_{K}_seeds"):
            group = awac.AWACGroup([trainer(k) for k in range(K)])
            rates = timed(lambda n: group.train_steps(buf, n, B, indices=[i[:n] for i in idx[:K]]), args.steps,
                          args.warmup, args.repeats)
            legs[f"awac_{K}_seeds"] = [K * r for r in rates]
            group.close()

    # the reference's update, eager, with and without the two host syncs per update that its logging costs
    for leg, items in (("eager_torch_reference_update", True), ("eager_torch_no_item", False)):
        if want(leg):
            eager = Eager(items)

            def run_eager(n, eager=eager):
                for i in range(n):
                    rows = idx[0][i]
                    eager.update(buf._states[rows], buf._actions[rows], buf._rewards[rows], buf._next_states[rows],
                                 buf._dones[rows])
            legs[leg] = timed(run_eager, args.steps, args.warmup, args.repeats)

    if want("iql_fp32_n_hidden_3_one_seed"):
        torch.manual_seed(0)
        q, v = ia.TwinQ(S, A, H, n_hidden=3).to(DEV), ia.ValueFunction(S, H, n_hidden=3).to(DEV)
        pol = ia.GaussianPolicy(S, A, 1.0, hidden_dim=H, n_hidden=3).to(DEV)
        ao = torch.optim.Adam(pol.parameters(), lr=3e-4)
        iql = co.ImplicitQLearning(1.0, pol, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 10 ** 6), q,
                                   torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                                   device=DEV, seed=0)
        legs["iql_fp32_n_hidden_3_one_seed"] = timed(
            lambda n: iql.train_steps(buf, n, B, indices=idx[0][:n], return_losses=False), args.steps, args.warmup,
            args.repeats)

    out = {"shape": {"S": S, "A": A, "B": B, "H": H}, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0)}
    for name, r in legs.items():
        out[name] = {"median": float(np.median(r)), "min": float(min(r)), "max": float(max(r))}
        print(f"{name:30s} {np.median(r):10.0f} steps/s  [{min(r):.0f} .. {max(r):.0f}]")
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
