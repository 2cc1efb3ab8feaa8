"""What the tests of ``iqlpref_amd.td3_bc`` share (test infrastructure, our own code; nothing of the library
but in ``build_trainer``, the one function here that needs a GPU):
the inputs of the step cases and a torch-autograd restatement of one ``TD3_BC.train`` (tdbc:324-380: the modules'
arithmetic, ``F.mse_loss``, ``torch.optim.Adam``, the target formula) that runs in float32 or float64 from given
parameters, batch and standard normals.

The step is restated in its two halves, because the second reads what the first wrote: ``critic_half`` gives the
critic loss and the gradients of both critics at (actor target, critics, critic targets); ``actor_half`` gives the
actor loss and the actor's gradients at (actor, critic 1 AFTER its Adam step).  The networks that are differentiated
have relu kinks that matter: both critics at (s, a) in the first half; the actor at s and critic 1 at (s, pi) -- the
gradient reaches the actor through critic 1's input -- in the second.  Everything else runs under no-grad.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.awac_cases import batch_of, judge_gap, polyak32  # noqa: F401
from tests.minari_cases import KINK, KINK_CAP, POISON, adam_step, judge, near_kink, ulp32  # noqa: F401

LR, DISCOUNT, TAU, ALPHA = 3e-4, 0.99, 5e-3, 2.5
# (tdbc's 0.2 / 0.5 clip one entry in eighty; these clip |eps| > 0.8, four in ten, and reach +-max_action)
POLICY_NOISE, NOISE_CLIP = 1.0, 0.8
LAYERS = ("net.0", "net.2", "net.4")
NAMES = tuple(f"{l}.{w}" for l in LAYERS for w in ("weight", "bias"))
TRAINED = ("actor", "critic_1", "critic_2")
TARGETS = ("actor_target", "critic_1_target", "critic_2_target")

# case -> (S, A, B, H, max_action, policy_freq, seed): the issue's five cases.  The seed of a case is the first at
# which the float64 restatement alone keeps the kink cap in every step and the conditions on the noise and on
# mean|q| hold (tests/test_td3_bc_host.py).
CASES = {"s3_a1_b1_h16": (3, 1, 1, 16, 1.0, 2, 3), "s17_a6_b17_h256": (17, 6, 17, 256, 1.0, 2, 0),
         "s128_a32_b48_h128": (128, 32, 48, 128, 2.0, 2, 0), "s45_a24_b64_h64_pf3": (45, 24, 64, 64, 1.0, 3, 0),
         "s29_a8_b256_h256_pf1": (29, 8, 256, 256, 1.0, 1, 0)}
NOISE_CASE = "s29_a8_b256_h256_pf1"


def n_steps(case):
    """2 x policy_freq steps, at least 3: every case sees two actor steps."""
    return max(3, 2 * CASES[case][5])


def hyper(case):
    """The trainer's constants of a case; policy_noise and noise_clip already times max_action (tdbc:473-474)."""
    mx, pf = CASES[case][4], CASES[case][5]
    return {"max_action": mx, "policy_freq": pf, "policy_noise": POLICY_NOISE * mx, "noise_clip": NOISE_CLIP * mx,
            "discount": DISCOUNT, "alpha": ALPHA, "tau": TAU}


def mlp(in_dim, hidden, out_dim):
    return torch.nn.Sequential(torch.nn.Linear(in_dim, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden),
                               torch.nn.ReLU(), torch.nn.Linear(hidden, out_dim))


def case_inputs(case):
    """(S, A, B, H, params, data, idx, eps, poison rows).

    ``params``: net name -> {tensor name: fp32 array} for the three trained networks and their three targets: torch's
    default Linear initialisation under the case's seed; the targets are the networks times (1 + 0.05 noise), so that
    reading a network for its target shows, and the actor target's last Linear is three times as large, so that some
    a' reach +-max_action.  The dataset has STEPS B + 8 rows; the first two and the last two, and every row that no
    step's indices name, hold POISON in every column.  ``idx`` is int64 [STEPS, B16]: columns [0, B) are the step's
    indices, columns [B, B16) name poisoned rows.  ``eps`` is float32 [STEPS, B, A].  Some terminals are 1."""
    S, A, B, H, mx, pf, seed = CASES[case]
    steps = n_steps(case)
    torch.manual_seed(3000 + seed)
    named = lambda m: {"net." + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(300 + seed)
    params = {"actor": named(mlp(S, H, A)), "critic_1": named(mlp(S + A, H, 1)), "critic_2": named(mlp(S + A, H, 1))}
    for n, t in zip(TRAINED, TARGETS):
        params[t] = {k: (v * (1 + 0.05 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in params[n].items()}
    params["actor_target"]["net.4.weight"] *= np.float32(3.0)
    n = steps * B + 8
    obs = rng.standard_normal((n, S)).astype(np.float32)
    nxt = rng.standard_normal((n, S)).astype(np.float32)
    act = rng.uniform(-mx, mx, (n, A)).astype(np.float32)
    rew = rng.standard_normal(n).astype(np.float32)
    done = (rng.uniform(size=n) < 0.2).astype(np.float32)
    B16 = -(-B // 16) * 16
    good = np.arange(2, n - 2)
    idx = np.empty((steps, B16), np.int64)
    for t in range(steps):
        idx[t, :B] = rng.choice(good, size=B, replace=B > len(good))
    poison = np.setdiff1d(np.arange(n), idx[:, :B].reshape(-1))
    idx[:, B:] = rng.choice(poison, size=(steps, B16 - B))
    obs[poison], nxt[poison], act[poison], rew[poison] = POISON, POISON, POISON, POISON
    data = {"observations": obs, "actions": act, "rewards": rew, "next_observations": nxt, "terminals": done}
    eps = rng.standard_normal((steps, B, A)).astype(np.float32)
    return S, A, B, H, params, data, idx, eps, poison


# --------------------------------------------------------------------------- #
# the step, restated
# --------------------------------------------------------------------------- #
def _tensors(p, dtype, grad):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad) for k, v in p.items()}


def _net(p, x, zs=None, force=None, slot=0):
    """``net(x)`` up to the last Linear (an actor's Tanh is the caller's).  ``zs``: a list that takes the two hidden
    pre-activations; ``force`` = (masks, value): relu' of the masked pairs of hidden layer i is ``value`` instead of
    [z > 0] (masks[slot + i]); forward values stay."""
    h = x
    for i, l in enumerate(LAYERS[:2]):
        z = F.linear(h, p[l + ".weight"], p[l + ".bias"])
        if zs is not None:
            zs.append(z.detach().numpy().copy())
        if force is None:
            h = torch.relu(z)
        else:
            near, value = torch.from_numpy(force[0][slot + i]), force[1]
            slope = torch.where(near, torch.full_like(z, float(value)), (z > 0).to(z.dtype)).detach()
            h = torch.relu(z).detach() + (z - z.detach()) * slope
    return F.linear(h, p[LAYERS[2] + ".weight"], p[LAYERS[2] + ".bias"])


def critic_half(actor_t, critic_1, critic_2, target_1, target_2, batch, eps, hp, dtype, force=None):
    """tdbc:331-352 at these parameters.  Returns (critic_loss, {"critic_1.<name>": gradient, "critic_2...."}, the
    four hidden pre-activations (critic 1's two, critic 2's two), extras: the unclipped noise, the clipped noise
    and a')."""
    s, a, r, s2, d = (torch.tensor(np.asarray(x), dtype=dtype) for x in batch)
    r, d = r.reshape(-1, 1), d.reshape(-1, 1)
    at, t1, t2 = (_tensors(p, dtype, False) for p in (actor_t, target_1, target_2))
    c1, c2 = _tensors(critic_1, dtype, True), _tensors(critic_2, dtype, True)
    mx = hp["max_action"]
    with torch.no_grad():
        raw = torch.tensor(np.asarray(eps), dtype=dtype) * hp["policy_noise"]
        noise = raw.clamp(-hp["noise_clip"], hp["noise_clip"])
        a2 = (mx * torch.tanh(_net(at, s2)) + noise).clamp(-mx, mx)
        x2 = torch.cat([s2, a2], 1)
        target_q = torch.min(_net(t1, x2), _net(t2, x2))
        target_q = r + (1 - d) * hp["discount"] * target_q
    zs, x = [], torch.cat([s, a], 1)
    q1 = _net(c1, x, zs, force, 0)
    q2 = _net(c2, x, zs, force, 2)
    loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
    loss.backward()
    grads = {f"{n}.{k}": v.grad.numpy().copy() for n, c in (("critic_1", c1), ("critic_2", c2)) for k, v in c.items()}
    return loss.item(), grads, tuple(zs), {"raw": raw.numpy().copy(), "noise": noise.numpy().copy(), "next_action": a2.numpy().copy()}


def actor_half(actor, critic_1, batch, hp, dtype, force=None):
    """tdbc:364-372 at these parameters (critic 1 as updated).  Returns (actor_loss, {"actor.<name>": gradient}, the
    four hidden pre-activations (the actor's two at s, critic 1's two at (s, pi)), extras: mean|q| and lmbda)."""
    s, a = (torch.tensor(np.asarray(x), dtype=dtype) for x in batch[:2])
    ap, c1 = _tensors(actor, dtype, True), _tensors(critic_1, dtype, False)
    zs = []
    pi = hp["max_action"] * torch.tanh(_net(ap, s, zs, force, 0))
    q = _net(c1, torch.cat([s, pi], 1), zs, force, 2)
    lmbda = hp["alpha"] / q.abs().mean().detach()
    loss = -lmbda * q.mean() + F.mse_loss(pi, a)
    loss.backward()
    grads = {f"actor.{k}": v.grad.numpy().copy() for k, v in ap.items()}
    return loss.item(), grads, tuple(zs), {"mean_abs_q": float(q.detach().abs().mean()), "lmbda": float(lmbda)}


# --------------------------------------------------------------------------- #
# the fp32 side of the bound, over several summation orders
# --------------------------------------------------------------------------- #
ORDERS = 8  # fp32 evaluations per bound: the restatement as it stands and seven permutations of its hidden units


def permute_hidden(p, perms):
    """``awac_cases.permute_hidden`` for these networks' names and depth: the same function of the input, every dot
    product summed in another order."""
    q = dict(p)
    for i, pi in enumerate(perms):
        a, b = LAYERS[i], LAYERS[i + 1]
        q[a + ".weight"], q[a + ".bias"] = q[a + ".weight"][pi], q[a + ".bias"][pi]
        q[b + ".weight"] = q[b + ".weight"][:, pi]
    return {k: np.ascontiguousarray(v) for k, v in q.items()}


def unpermute_grads(g, perms):
    """The gradients of ``permute_hidden(p, perms)`` in the order of ``p``'s entries ({tensor name: array})."""
    g = dict(g)
    for i, pi in enumerate(perms):
        a, b = LAYERS[i], LAYERS[i + 1]
        inv = np.argsort(pi)
        g[a + ".weight"], g[a + ".bias"] = g[a + ".weight"][inv], g[a + ".bias"][inv]
        g[b + ".weight"] = g[b + ".weight"][:, inv]
    return g


def fp32_gap(half, nets, rest, trained, l64, g64, orders=ORDERS, seed=0):
    """``awac_cases.fp32_gap`` (its docstring has the reason for several orders) for these networks: |fp32 torch -
    float64 torch| of one half over ``orders`` summation orders.  Returns (largest loss gap, {gradient name: largest
    gap per entry})."""
    rng = np.random.default_rng(seed)
    lgap, ggap = 0.0, {k: np.zeros_like(v) for k, v in g64.items()}
    for o in range(orders):
        perms = [[np.arange(n[LAYERS[i] + ".bias"].shape[0]) if o == 0 else rng.permutation(n[LAYERS[i] + ".bias"].shape[0])
                  for i in range(2)] for n in nets]
        l32, g32 = half(*[permute_hidden(n, pm) for n, pm in zip(nets, perms)], *rest, torch.float32)[:2]
        lgap = max(lgap, abs(l32 - l64))
        for prefix, i in trained.items():
            own = {k[len(prefix) + 1:]: v for k, v in g32.items() if k.startswith(prefix + ".")}
            for k, v in unpermute_grads(own, perms[i]).items():
                name = f"{prefix}.{k}"
                ggap[name] = np.maximum(ggap[name], np.abs(v.astype(np.float64) - g64[name]))
    return lgap, ggap


def is_actor_step(total_it, policy_freq):
    """tdbc:362 at the one-based ``total_it``."""
    return total_it % policy_freq == 0


def f64_trajectory(case):
    """The float64 restatement on its own: the case's steps from its initial parameters.  Returns per step the share
    of (row, hidden unit) pairs of the differentiated networks within KINK of zero, the losses (actor_loss None
    without an actor step) and the extras of the halves."""
    S, A, B, H, params, data, idx, eps, _ = case_inputs(case)
    hp = hyper(case)
    p = {n: {k: v.astype(np.float64) for k, v in params[n].items()} for n in params}
    m = {n: {k: np.zeros_like(v) for k, v in p[n].items()} for n in TRAINED}
    v = {n: {k: np.zeros_like(x) for k, x in p[n].items()} for n in TRAINED}
    out, actor_it = [], 0

    def adam(n, grads, t1):
        for k in p[n]:
            p[n][k], m[n][k], v[n][k] = adam_step(p[n][k], m[n][k], v[n][k], grads[f"{n}.{k}"], t1, torch.float64, lr=LR)

    for t in range(n_steps(case)):
        batch = batch_of(data, idx[t, :B])
        lc, gc, zc, xc = critic_half(p["actor_target"], p["critic_1"], p["critic_2"], p["critic_1_target"],
                                     p["critic_2_target"], batch, eps[t], hp, torch.float64)
        adam("critic_1", gc, t + 1), adam("critic_2", gc, t + 1)
        la, za, xa = None, (), None
        if is_actor_step(t + 1, hp["policy_freq"]):
            la, ga, za, xa = actor_half(p["actor"], p["critic_1"], batch, hp, torch.float64)
            actor_it += 1
            adam("actor", ga, actor_it)
            for n, tg in zip(TRAINED, TARGETS):
                p[tg] = {k: (1 - TAU) * p[tg][k] + TAU * p[n][k] for k in p[tg]}
        near = near_kink(zc + za)
        out.append({"share": sum(int(x.sum()) for x in near) / sum(x.size for x in near), "critic_loss": lc,
                    "actor_loss": la, "critic": xc, "actor": xa})
    return out


# --------------------------------------------------------------------------- #
# what the GPU tests of the family share
# --------------------------------------------------------------------------- #
DEV = "cuda:0"


def build_trainer(S, A, H, params, hp, seed=0, keep_grads=True, **over):
    """A ``td3_bc.TD3_BC`` on ``DEV`` from parameter arrays (``params``: net name -> {tensor name: array}; targets where
    given) and the constants ``hp`` (``hyper``), ``over`` replacing entries of it.  Needs the GPU."""
    from iqlpref_amd import td3_bc
    hp = dict(hp, **over)
    actor, c1, c2 = td3_bc.Actor(S, A, hp["max_action"], H), td3_bc.Critic(S, A, H), td3_bc.Critic(S, A, H)
    for m, n in ((actor, "actor"), (c1, "critic_1"), (c2, "critic_2")):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        m.to(DEV)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=LR)
    tr = td3_bc.TD3_BC(hp["max_action"], actor, adam(actor), c1, adam(c1), c2, adam(c2), discount=hp["discount"],
                       tau=hp["tau"], policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"],
                       policy_freq=hp["policy_freq"], alpha=hp["alpha"], device=DEV, seed=seed, keep_grads=keep_grads)
    with torch.no_grad():
        for n in TARGETS:
            if n in params:
                for k, p in getattr(tr, n).named_parameters():
                    p.copy_(torch.from_numpy(params[n][k]))
    return tr


def box_muller(seed, step, B, A, stream):
    """include/iqlhip.h, iqlhip_awac_train_steps / iqlhip_td3bc_train_steps: float64 Box-Muller on Philox block (row * 8
    + column / 4, step lo, step hi, stream), words (x, y) / (z, w) one pair each.  [B, A] float64."""
    from oracle import philox
    nq = (A + 3) // 4
    rows = np.repeat(np.arange(B, dtype=np.uint32), nq)
    quads = np.tile(np.arange(nq, dtype=np.uint32), B)
    x, y, z, w = philox.philox4x32_10(rows * np.uint32(8) + quads, np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32),
                                      np.uint32(stream), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((B, nq, 4), np.float64)
    for pair, (ua, ub) in enumerate(((x, y), (z, w))):
        u1 = (ua.astype(np.float64) + 1.0) / 4294967296.0
        u2 = ub.astype(np.float64) / 4294967296.0
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        out[:, :, 2 * pair] = (rad * np.cos(ang)).reshape(B, nq)
        out[:, :, 2 * pair + 1] = (rad * np.sin(ang)).reshape(B, nq)
    return out.reshape(B, 4 * nq)[:, :A]
