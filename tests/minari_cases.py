"""What the tests of ``minari_bc`` / ``minari_iql`` share (test infrastructure, our own code; no GPU, nothing of the
library): the fixtures' readers, the inputs of the behaviour-cloning step cases, and a torch-autograd restatement
of the BC step (bcref:230-243: Actor, ``F.mse_loss``, ``torch.optim.Adam``) that runs in float32 or float64.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

H = 256
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8  # bcref:330: torch.optim.Adam defaults at lr 3e-4
KINK = 1e-5      # a pre-activation closer to zero than this may fall on either side of relu' in fp32
KINK_CAP = 1e-3  # at most this share of the (row, hidden unit) pairs of the steps compared may be that close
STEPS = 3
POISON = 1e30

# case -> (S, A, B, max_action, seed): the issue's five shapes.  64 = whole slabs; 17 = one row into the second
# slab; 48 with the widest layers of the envelope's middle (S 96, A 32 = two output tiles); 1 = a single row, a
# single output; 256 = the pen batch, 16 slabs.  max_action differs from 1 where a missing factor would hide.
# The seed of a case is the first at which the float64 restatement alone keeps the kink cap in all three steps
# (tests/test_bc_step_host.py; at one row a single pair of the 512 is already twice the cap: seed 0 has one).
CASES = {"s45_a24_b64": (45, 24, 64, 1.0, 0), "s17_a6_b17": (17, 6, 17, 2.0, 0), "s96_a32_b48": (96, 32, 48, 1.0, 0),
         "s3_a1_b1": (3, 1, 1, 0.5, 1), "s45_a24_b256": (45, 24, 256, 1.0, 0)}


def load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


def run_of(golden, name):
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}


def from_planes(planes, shape):
    """make_minari_fixture.byte_planes undone: uint8 [4, n] -> fp32 tensor of ``shape``."""
    return torch.from_numpy(np.ascontiguousarray(planes.T).reshape(-1).view(np.float32).reshape(tuple(shape)).copy())


def bc_state_dict(run):
    """The reference's state dict that the fixture keeps whole (run "raw"): (file name, state dict)."""
    fname = str(run["whole"])
    pre = f"whole/{fname}"
    actor = {k: from_planes(run[f"{pre}/actor/{k}/planes"], run[f"{pre}/actor/{k}/shape"]) for k in NAMES}
    state = {}
    for i, k in enumerate(NAMES):
        shape = actor[k].shape
        state[i] = {"step": torch.tensor(float(run[f"{pre}/actor_optimizer/{i}/step"])),
                    "exp_avg": from_planes(run[f"{pre}/actor_optimizer/{i}/exp_avg/planes"], shape),
                    "exp_avg_sq": from_planes(run[f"{pre}/actor_optimizer/{i}/exp_avg_sq/planes"], shape)}
    ref_opt = torch.optim.Adam([torch.nn.Parameter(v.clone()) for v in actor.values()], lr=LR)
    groups = ref_opt.state_dict()["param_groups"]  # (torch's own group of this version, with the run's values)
    groups[0].update(lr=float(run[f"{pre}/actor_optimizer/lr"]), betas=tuple(run[f"{pre}/actor_optimizer/betas"]),
                     eps=float(run[f"{pre}/actor_optimizer/eps"]), params=[int(i) for i in run[f"{pre}/actor_optimizer/params"]])
    return fname, {"actor": actor, "actor_optimizer": {"state": state, "param_groups": groups}}


# --------------------------------------------------------------------------- #
# the step, restated
# --------------------------------------------------------------------------- #
def bc_forward_backward(params, s, a, max_action, dtype, force=None):
    """Loss and gradients of one BC step at ``params`` (name -> array) on the batch (s, a) in ``dtype``.
    Returns (loss, {name: gradient array}, (z1, z2) pre-activations as arrays).  ``force``: None, or (near1,
    near2, value) -- boolean masks [B, 256] of the hidden pre-activations whose relu' is set to ``value`` (0 or
    1) instead of [z > 0]; the forward values are untouched."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    x, act = torch.tensor(np.asarray(s), dtype=dtype), torch.tensor(np.asarray(a), dtype=dtype)
    zs = []

    def relu(z, i):
        zs.append(z.detach().numpy().copy())
        if force is None:
            return torch.relu(z)
        near, value = torch.from_numpy(force[i]), force[2]
        slope = torch.where(near, torch.full_like(z, float(value)), (z > 0).to(dtype)).detach()
        return torch.relu(z).detach() + (z - z.detach()) * slope

    h = relu(F.linear(x, p["net.0.weight"], p["net.0.bias"]), 0)
    h = relu(F.linear(h, p["net.2.weight"], p["net.2.bias"]), 1)
    pi = max_action * torch.tanh(F.linear(h, p["net.4.weight"], p["net.4.bias"]))
    loss = F.mse_loss(pi, act)
    loss.backward()
    return loss.item(), {k: v.grad.numpy().copy() for k, v in p.items()}, tuple(zs)


def adam_step(p0, m0, v0, g, t, dtype, lr=LR):
    """torch.optim.Adam's step number ``t`` (1-based) from parameter p0, moments m0 / v0 and gradient g, in
    ``dtype``: (p1, m1, v1) as arrays."""
    mk = lambda x: torch.tensor(np.asarray(x), dtype=dtype)
    p = torch.nn.Parameter(mk(p0))
    opt = torch.optim.Adam([p], lr=lr, betas=BETAS, eps=EPS, foreach=False)
    if t > 1:
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": mk(m0), "exp_avg_sq": mk(v0)}
    p.grad = mk(g)
    opt.step()
    st = opt.state[p]
    return p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()


def ulp32(x):
    """The fp32 rounding unit at the largest entry of x."""
    m = np.float32(np.max(np.abs(x))) if np.size(x) else np.float32(0)
    return float(np.spacing(m)) if m > 0 else float(np.finfo(np.float32).tiny)


# --------------------------------------------------------------------------- #
# the step cases
# --------------------------------------------------------------------------- #
def bc_case_inputs(case):
    """(S, A, B, max_action, initial parameters {name: fp32 array}, dataset dict, idx, poison rows).

    The parameters are torch's default Linear initialisation under the case's seed.  The dataset has 3 B + 8
    rows; the first two and the last two, and every row that no step's indices name, hold POISON in every state
    and action column.  ``idx`` is int64 [STEPS, B16] (B16 = B rounded up to 16): columns [0, B) are the step's
    indices, columns [B, B16) -- the memory right behind them, where a kernel that padded the batch by reading on
    would look -- name poisoned rows."""
    S, A, B, max_action, seed = CASES[case]
    torch.manual_seed(1000 + seed)
    net = torch.nn.Sequential(torch.nn.Linear(S, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
                              torch.nn.Linear(H, A), torch.nn.Tanh())
    params = {"net." + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    rng = np.random.default_rng(seed)
    n = 3 * B + 8
    obs = rng.standard_normal((n, S)).astype(np.float32)
    act = (max_action * rng.uniform(-1, 1, (n, A))).astype(np.float32)
    B16 = -(-B // 16) * 16
    good = np.arange(2, n - 2)
    idx = np.empty((STEPS, B16), np.int64)
    for t in range(STEPS):
        idx[t, :B] = rng.choice(good, size=B, replace=B > len(good))
    poison = np.setdiff1d(np.arange(n), idx[:, :B].reshape(-1))
    idx[:, B:] = rng.choice(poison, size=(STEPS, B16 - B))
    obs[poison], act[poison] = POISON, POISON
    data = {"observations": obs, "actions": act, "rewards": np.zeros(n, np.float32),
            "next_observations": obs.copy(), "terminals": np.zeros(n, np.float32)}
    return S, A, B, max_action, params, data, idx, poison


def near_kink(zs):
    """The (row, unit) pairs of the two hidden layers whose pre-activation is within KINK of zero."""
    return tuple(np.abs(z) < KINK for z in zs)


def bc_f64_trajectory(case):
    """The float64 restatement on its own: STEPS steps from the case's initial parameters.  Returns per step the
    share of (row, hidden unit) pairs within KINK of zero, and the losses."""
    S, A, B, max_action, params, data, idx, _ = bc_case_inputs(case)
    p = {k: v.astype(np.float64) for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    shares, losses = [], []
    for t in range(STEPS):
        rows = idx[t, :B]
        loss, g, zs = bc_forward_backward(p, data["observations"][rows], data["actions"][rows], max_action, torch.float64)
        near = near_kink(zs)
        shares.append(sum(int(x.sum()) for x in near) / sum(x.size for x in near))
        losses.append(loss)
        for k in p:
            p[k], m[k], v[k] = adam_step(p[k], m[k], v[k], g[k], t + 1, torch.float64)
    return shares, losses


def judge(got, want64, got32):
    """|got - want64| against the issue's bound for one tensor: 4 x the largest |fp32 torch - float64 torch| of
    that tensor, floored at the tensor's fp32 rounding unit at its largest entry.  Returns (error / bound, bound)."""
    want64 = np.asarray(want64, np.float64)
    bound = max(4.0 * float(np.max(np.abs(np.asarray(got32, np.float64) - want64))), ulp32(want64))
    return float(np.max(np.abs(np.asarray(got, np.float64) - want64))) / bound, bound
