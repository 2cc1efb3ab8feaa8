"""Stand-ins and restatements shared by tests/golden/make_bb_fixture.py and the BB-flavour tests
(tests/test_bb_host.py, tests/test_gpu_bb.py): the synthetic dataset, a numpy reward callable with
the reference's call shape, an actor that replays recorded actions, and a float64 torch restatement of
one IQL step of algorithms/custom_offline/iql_bb.py on an explicit batch.  No GPU, no reference."""
import math

import numpy as np
import torch

N_ROWS, BATCH, STATE_DIM, ACTION_DIM = 167, 32, 26, 2  # 5 whole blocks and a tail of 7
MOVE_STATS = (0.9, 0.2, 0.35, 0.1)  # (agent mean, std, obstacle mean, std): the simulator reads [2], [3]
HYPER = dict(gamma=0.99, tau=0.005, beta=3.0, iql_tau=0.7, lr=3e-4, betas=(0.9, 0.999), eps=1e-8)


def synth_dataset(seed: int = 21, n: int = N_ROWS):
    """Arrays of the HDF5 layout: simulator-shaped states (2 + 6 * 3 + 2 + 4 columns), (speed, angle)
    actions with speeds in [0, 0.8] (so the 99th percentile sits below 1 and tanh can exceed it), raw and
    normalised rewards, attn_mask with a few zeros."""
    rng = np.random.default_rng(seed)
    states = rng.uniform(-50, 50, (n, STATE_DIM))
    states[:, 4:20:3] = rng.uniform(0, 360, (n, 6))  # obstacle headings
    tail = np.stack([rng.choice([9, 10, 11], n), rng.choice([1, 2, 3, 4], n), rng.choice(4, n), rng.choice(181, n)], 1)
    states[:, -4:] = tail
    nxt = states.copy()
    nxt[:, :20] += rng.normal(0, 0.5, (n, 20))
    actions = np.stack([rng.uniform(0, 0.8, n), rng.uniform(-2, 2, n)], 1)
    rewards = rng.normal(0, 1, n)
    mask = np.ones(n)
    mask[rng.choice(n, 9, replace=False)] = 0.0
    mask[n - 3] = 0.0  # one of them inside the short last batch
    f = lambda x: x.astype(np.float32)
    return {"states": f(states), "actions": f(actions), "rewards": f(rewards),
            "n_rewards": f((rewards - rewards.mean()) / rewards.std()), "next_states": f(nxt), "attn_mask": f(mask)}


def numpy_reward(states, actions, timesteps, attn_mask, training=False):
    """A reward with the call shape of the reference's model: float64 numpy over the whole context."""
    assert states.shape[1] == actions.shape[1] == timesteps.shape[1] == attn_mask.shape[1] and not training
    v = np.tanh(0.01 * states[..., :2].sum(-1) + 0.5 * actions[..., 0] - 0.002 * actions[..., 1]) \
        + 0.01 * np.sin(timesteps) + 0.001 * np.cumsum(actions[..., 0], axis=1)
    return {"value": v[:, None, :]}, None


class ReplayActor:
    """Hands out recorded actions in order and keeps the states it is asked about."""

    def __init__(self, actions):
        self.actions, self.states, self.mode = list(actions), [], []

    def eval(self):
        self.mode.append("eval")

    def train(self):
        self.mode.append("train")

    def act(self, state, device="cpu"):
        self.states.append(np.array(state))
        return np.array(self.actions[len(self.states) - 1])


# --------------------------------------------------------------------------- #
# one IQL step in float64 torch on the CPU (iql_bb.py: _update_v, _update_q, _update_policy, train)
# --------------------------------------------------------------------------- #
NETS = ("q1", "q2", "v", "actor")


class StepRestatement:
    """``params``: {net: [W1, b1, W2, b2, W3, b3]} (torch layouts) and ``log_std``; float64 copies are
    trained with plain Adam, the convex Polyak form and the cosine actor schedule.  ``train(batch)``
    takes ONLY the rows that count: every mean is over them."""

    def __init__(self, params, log_std, t_max, hyper=HYPER):
        d = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
        self.p = {n: [d(x) for x in params[n]] for n in NETS}
        self.log_std = d(log_std)
        self.target = {n: [x.detach().clone() for x in self.p[n]] for n in ("q1", "q2")}
        self.h, self.t_max, self.it = hyper, t_max, 0
        leaves = [x for n in NETS for x in self.p[n]] + [self.log_std]
        self.m = {id(x): torch.zeros_like(x) for x in leaves}
        self.v = {id(x): torch.zeros_like(x) for x in leaves}

    @staticmethod
    def mlp(w, x, tanh=False):
        x = torch.relu(x @ w[0].T + w[1])
        x = torch.relu(x @ w[2].T + w[3])
        x = x @ w[4].T + w[5]
        return torch.tanh(x) if tanh else x

    def _adam(self, leaves, loss, lr):
        b1, b2 = self.h["betas"]
        grads = torch.autograd.grad(loss, leaves)
        t = self.it + 1
        with torch.no_grad():
            for x, g in zip(leaves, grads):
                m, v = self.m[id(x)], self.v[id(x)]
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                x -= (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + self.h["eps"])

    def train(self, s, a, r, s2, mask):
        f = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
        s, a, r, s2, mask = f(s), f(a), f(r).reshape(-1), f(s2), f(mask).reshape(-1)
        h, sa = self.h, torch.cat([s, a], 1)
        with torch.no_grad():
            next_v = self.mlp(self.p["v"], s2)[:, 0]
            target_q = torch.min(self.mlp(self.target["q1"], sa)[:, 0], self.mlp(self.target["q2"], sa)[:, 0])
        adv = target_q - self.mlp(self.p["v"], s)[:, 0]
        v_loss = torch.mean(torch.abs(h["iql_tau"] - (adv < 0).double()) * adv ** 2)
        self._adam(self.p["v"], v_loss, h["lr"])
        targets = r + mask * h["gamma"] * next_v
        q_loss = sum(torch.mean((self.mlp(self.p[n], sa)[:, 0] - targets) ** 2) for n in ("q1", "q2")) / 2
        self._adam(self.p["q1"] + self.p["q2"], q_loss, h["lr"])
        with torch.no_grad():
            for n in ("q1", "q2"):
                for tp, sp in zip(self.target[n], self.p[n]):
                    tp.copy_((1 - h["tau"]) * tp + h["tau"] * sp)
        exp_adv = torch.exp(h["beta"] * adv.detach()).clamp(max=100.0)
        dist = torch.distributions.Normal(self.mlp(self.p["actor"], s, tanh=True),
                                          torch.exp(self.log_std.clamp(-20.0, 2.0)))
        a_loss = torch.mean(exp_adv * -dist.log_prob(a).sum(-1))
        lr_a = h["lr"] * (1 + math.cos(math.pi * self.it / self.t_max)) / 2
        self._adam(self.p["actor"] + [self.log_std], a_loss, lr_a)
        self.it += 1
        return [v_loss.item(), q_loss.item(), a_loss.item()]

    def moments(self, net):
        leaves = self.p[net] + ([self.log_std] if net == "actor" else [])
        return [self.m[id(x)].numpy() for x in leaves], [self.v[id(x)].numpy() for x in leaves]
