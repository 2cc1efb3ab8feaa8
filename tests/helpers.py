"""Shared helpers for the parity tests (oracle side + golden-file access)."""
import os

import numpy as np

from oracle import iql_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TRAJ = ["traj_antmaze", "traj_cheetah_det", "traj_pen_dropout", "traj_antmaze_h256"]
# BASELINE configs 1 / 3 and config 5's batch at H = 256 (initial parameters and data rebuilt from the seed)
TRAJ_BIG = ["traj_cheetah_h256", "traj_pen_h256", "traj_antmaze_b1024"]
# depths / widths away from the default (make_fixtures.SHAPES): the general layer-wise step
TRAJ_SHAPES = ["traj_deep3_w96", "traj_shallow1_w40_drop", "traj_deep4_w72_det"]


def synth_dataset(rng, n, s_dim, a_dim, reward="normal"):
    """Seeded synthetic transitions (shared with tests/golden/make_fixtures.py, which feeds the
    same arrays to the reference)."""
    obs = rng.standard_normal((n, s_dim)).astype(np.float32)
    nxt = rng.standard_normal((n, s_dim)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, a_dim)).astype(np.float32)
    if reward == "normal":
        rew = rng.standard_normal(n).astype(np.float32)
    else:  # antmaze-like sparse, then -1 (normalize_reward=1)
        rew = (rng.uniform(size=n) < 0.05).astype(np.float32) - 1.0
    term = (rng.uniform(size=n) < 0.02)
    return {
        "observations": obs,
        "actions": act,
        "rewards": rew,
        "next_observations": nxt,
        "terminals": term,
    }


def tensor_checks(v):
    """[sum, sum of magnitudes, sum of index-weighted values] in float64: identifies a tensor."""
    x = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.asarray([x.sum(), np.abs(x).sum(), (x * (np.arange(x.size) % 997 + 1)).sum()])


def regen_inputs(d):
    """Initial parameters and data of a seed-regenerated golden trajectory: the dataset from
    numpy's default_rng(seed), the networks from torch.manual_seed(seed) and OUR module
    constructors in the reference's order (q, v, actor; make_fixtures.run_trajectory) -- the same
    torch calls in the same order give the reference's initial weights, which is itself part of the
    drop-in contract.  Verified against the checksums the fixture holds of the reference's own
    arrays: a mismatch raises, nothing is compared on other inputs."""
    import torch
    import iqlpref_amd as ia
    h = d["hyper"]
    S, A, H, n = int(h[0]), int(h[1]), int(h[2]), int(h[4])
    det, drop = bool(h[10]), (None if h[11] < 0 else float(h[11]))
    seed = int(d["regen_seed"])
    data = synth_dataset(np.random.default_rng(seed), n, S, A, str(d["reward_kind"]))
    data["terminals"] = data["terminals"].astype(np.float32)
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(seed)
        q = ia.TwinQ(S, A, hidden_dim=H)
        v = ia.ValueFunction(S, hidden_dim=H)
        actor = (ia.DeterministicPolicy if det else ia.GaussianPolicy)(S, A, 1.0, hidden_dim=H, dropout=drop)
    finally:
        torch.random.set_rng_state(state)
    if not det:
        with torch.no_grad():
            actor.log_std.copy_(torch.linspace(-0.5, 0.3, A))
    nets = tuple({k: t.detach().numpy().copy() for k, t in m.state_dict().items()} for m in (q, v, actor))
    for k, arr in data.items():
        if not np.array_equal(tensor_checks(arr), d[f"check/data/{k}"]):
            raise AssertionError(f"regenerated data/{k} is not what the reference was given")
    for pre, net in zip(("qf", "vf", "actor"), nets):
        for k, arr in net.items():
            if not np.array_equal(tensor_checks(arr), d[f"check/init/{pre}/{k}"]):
                raise AssertionError(f"regenerated init/{pre}/{k} differs from the reference's initial weights")
    return data, nets


def regen_indices(d):
    """The index stream of a seed-regenerated trajectory: make_fixtures.run_trajectory draws
    torch.randint(0, n_rows, (batch,)) from torch.Generator().manual_seed(seed + 1) per step."""
    import torch
    h = d["hyper"]
    B, n, K = int(h[3]), int(h[4]), int(h[5])
    g = torch.Generator().manual_seed(int(d["regen_seed"]) + 1)
    idx = np.stack([torch.randint(0, n, (B,), generator=g).numpy() for _ in range(K)])
    if "check/indices" in getattr(d, "files", d) and not np.array_equal(tensor_checks(idx), d["check/indices"]):
        raise AssertionError("regenerated index stream is not the one the reference run drew")
    return idx


def load_traj(name, mode):
    d = np.load(os.path.join(GOLDEN, f"{name}_{mode}.npz"))
    common = d
    if "h256" in name and "regen_seed" not in d.files:
        common = np.load(os.path.join(GOLDEN, f"{name}_common.npz"))
    h = d["hyper"]
    hyper = dict(
        s_dim=int(h[0]), a_dim=int(h[1]), hidden=int(h[2]), batch=int(h[3]),
        n_rows=int(h[4]), k_steps=int(h[5]), beta=float(h[6]), iql_tau=float(h[7]),
        discount=float(h[8]), tau=float(h[9]), deterministic=bool(h[10]),
        dropout=None if h[11] < 0 else float(h[11]), max_steps=int(h[12]),
        n_hidden=int(h[13]) if len(h) > 13 else 2)
    if "regen_seed" in d.files:
        data, nets = regen_inputs(d)
        return d, hyper, data, nets
    data = {k.split("/")[1]: common[k] for k in common.files if k.startswith("data/")}
    qf, vf, actor = orc.split_init(common)
    return d, hyper, data, (qf, vf, actor)


def keep_masks(d, hyper, t):
    if hyper["dropout"] is None:
        return None
    m = np.unpackbits(d["dropout_keep"][t], axis=-1)[..., :hyper["hidden"]].astype(bool)
    return [m[l] for l in range(m.shape[0])]


def make_oracle(hyper, nets, mode):
    qf, vf, actor = nets
    return orc.IQLOracle(qf, vf, actor, iql_tau=hyper["iql_tau"], beta=hyper["beta"],
                         max_steps=hyper["max_steps"], discount=hyper["discount"],
                         tau=hyper["tau"], mode=mode, dropout=hyper["dropout"])


def golden_param(d, key, arr):
    """Compare ``arr`` against golden entry ``key`` (full or strided summary)."""
    if key in d.files:
        return d[key], arr
    if key + "#stride37" in d.files:
        return d[key + "#stride37"], np.asarray(arr).reshape(-1)[::37]
    return None, None


def resume_state(d):
    """The reference's checkpoint after `ckpt/total_it` steps out of a traj_resume_* fixture:
    (qf, vf, actor, q_target) parameter dicts, {group: {param name: (exp_avg, exp_avg_sq)}} with the
    parameter names in the reference's optimizer order, the step count."""
    pick = lambda pre: {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
    nets = (pick("ckpt/qf/"), pick("ckpt/vf/"), pick("ckpt/actor/"))
    target = pick("ckpt/q_target/")
    moments = {}
    for group, opt, net in (("q", "q_optimizer", nets[0]), ("v", "v_optimizer", nets[1]),
                            ("actor", "actor_optimizer", nets[2])):
        names = list(net.keys())  # state_dict order = named_parameters order = the optimizer's index order
        if group == "actor" and "log_std" in names:  # (registered first in GaussianPolicy: index 0 either way)
            assert names[0] == "log_std" or names[-1] == "log_std"
        assert int(d[f"ckpt/{opt}/n_params"]) == len(names)
        moments[group] = {n: (d[f"ckpt/{opt}/{i}/exp_avg"], d[f"ckpt/{opt}/{i}/exp_avg_sq"])
                          for i, n in enumerate(names)}
        for i, n in enumerate(names):
            assert d[f"ckpt/{opt}/{i}/exp_avg"].shape == net[n].shape, (opt, i, n)
            assert float(d[f"ckpt/{opt}/{i}/step"]) == float(d["ckpt/total_it"])
    return nets, target, moments, int(d["ckpt/total_it"])


# ---------------------------------------------------------------------------------------------
# Envelope tests of the stand-alone relabel kernels (iqlhip_mlp_forward, iqlhip_cvar_tail_mean):
# plain numpy references and input generators, shared by the GPU tests and the host test that
# checks the generators themselves (tests/test_relabel_oracle.py).
# ---------------------------------------------------------------------------------------------
# reward_models/q_mlp.py:121-130 in table order: activation code 8 + i of iqlhip_mlp_desc is entry i
FLAX_ACTIVATIONS = {"cos": np.cos, "tanh": np.tanh, "relu": lambda v: np.maximum(v, 0),
                    "softplus": lambda v: np.logaddexp(v, 0), "sin": np.sin,
                    "leaky_relu": lambda v: np.where(v >= 0, v, 0.01 * v), "swish": lambda v: v / (1 + np.exp(-v)),
                    "none": lambda v: v}
ACT_FLAX_BASE = 8


def mlp_act(code, hidden):
    """The function behind an activation code of iqlhip_mlp_desc (hidden: 0 relu, 1 tanh; output:
    0 none, 1 tanh; 8 + i: entry i of the table, either place)."""
    if code >= ACT_FLAX_BASE:
        return list(FLAX_ACTIVATIONS.values())[code - ACT_FLAX_BASE]
    if code == 1:
        return np.tanh
    return FLAX_ACTIVATIONS["relu"] if hidden else FLAX_ACTIVATIONS["none"]


def mlp_weights_for(rng, dims):
    """fp32 ([in, out] weights standard_normal / sqrt(fan_in), biases 0.1 standard_normal): O(1) activations."""
    ws = [rng.standard_normal((dims[i], dims[i + 1])).astype(np.float32) / np.float32(np.sqrt(dims[i]))
          for i in range(len(dims) - 1)]
    bs = [rng.standard_normal(dims[i + 1]).astype(np.float32) * np.float32(0.1) for i in range(len(dims) - 1)]
    return ws, bs


def mlp_forward_ref(ws, bs, x, hidden_act=0, out_act=0, dtype=np.float64, keeps=None, scale=None):
    """x @ W + b per layer in ``dtype`` (fp64: the reference; fp32: the yardstick of what fp32 can
    give), ws [in, out].  keeps: one boolean mask [n, width] per hidden layer, kept values times scale."""
    h = np.asarray(x, dtype=dtype)
    n = len(ws)
    for l in range(n):
        h = (h @ ws[l].astype(dtype) + bs[l].astype(dtype)).astype(dtype)
        h = np.asarray(mlp_act(hidden_act if l < n - 1 else out_act, l < n - 1)(h), dtype=dtype)
        if keeps is not None and l < n - 1:
            h = (h * keeps[l] * dtype(scale)).astype(dtype)
    return h


# iqlhip_cvar_tail_mean: L lanes share a column (about one per 16 rows), COLS columns per work-group;
# beyond S = 1248 the 32-column LDS image no longer fits and a work-group takes 16 columns
CVAR_S_MAX = 2400


def cvar_launch_config(S):
    """(columns per work-group, lanes per column) the launcher picks for S rows."""
    L = 2
    while L < 32 and L * 16 < S:
        L *= 2
    if L < 32:
        return {2: 128, 4: 64, 8: 32, 16: 32}[L], L
    return (32 if S <= 1248 else 16), 32


CVAR_FAMILIES = ("normal", "ties", "constant", "two_half", "two_tail", "wide", "negative", "ulps",
                 "zeros_denormals", "ascending", "descending")


def cvar_column(rng, family, S, n_tail):
    """One fp32 column of S finite values of a named family (row order shuffled unless it is the point)."""
    f64 = rng.standard_normal(S)
    if family == "normal":
        col = f64
    elif family == "ties":  # one decimal: many equal values
        col = np.round(f64, 1)
    elif family == "constant":
        col = np.full(S, f64[0])
    elif family in ("two_half", "two_tail"):  # exactly k copies of the smaller value
        k = S // 2 if family == "two_half" else n_tail
        col = np.where(rng.permutation(S) < k, -1.5, 0.75)
    elif family in ("wide", "negative"):  # ~26 decades each side of 1: where a value-interpolated probe is worst
        mag = np.clip(np.exp(30.0 * f64), 1e-30, 1e30)  # (strictly negative stays strictly negative in fp32)
        col = -mag if family == "negative" else np.where(rng.uniform(size=S) < 0.5, -mag, mag)
    elif family == "ulps":
        # neighbouring floats 1 + k 2^-23, each repeated: from S = 32 on every value is there more
        # than 8 times (S // 12 distinct values, at most 16), the threshold's multiplicity included
        nd = min(16, max(1, S // 12))
        col = 1.0 + (rng.permutation(S) % nd) * 2.0 ** -23
    elif family == "zeros_denormals":
        # +0, -0, fp32 denormals of both signs and normals of the smallest binades.  The column's minimum is
        # a normal number (~ -1e-30) and in every tail: tail means stay where a rounding is relative, which
        # is what the tests' bound models (below 2^-126 fp32 is spaced 2^-149 whatever the magnitude)
        j = rng.integers(1, 1 << 23, S).astype(np.float64) * 2.0 ** -149
        kind = rng.permutation(S) % 6
        col = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                        [0.0, -0.0, j, -j, f64 * 1e-30], f64 * 4e-38)
        col[rng.integers(S)] = -(1.0 + abs(f64[0])) * 1e-30
    elif family in ("ascending", "descending"):
        col = np.sort(f64)
        return (col if family == "ascending" else col[::-1]).astype(np.float32)
    else:
        raise KeyError(family)
    return np.asarray(col, dtype=np.float32)


def cvar_matrix(rng, S, N, n_tail, first=0):
    """fp32 [S, N]: the families round-robin over the columns, starting at family ``first``."""
    names = [CVAR_FAMILIES[(first + c) % len(CVAR_FAMILIES)] for c in range(N)]
    return np.stack([cvar_column(rng, f, S, n_tail) for f in names], axis=1), names


def cvar_int_matrix(rng, S, N):
    """Integer-valued fp32 entries in [-1000, 1000] with ties: every fp32 partial sum is exact."""
    return rng.integers(-1000, 1001, (S, N)).astype(np.float32)


def cvar_n_tails(S):
    from oracle import relabel_oracle as ro
    cand = [1, 2, 8, 9, S // 20 or 1, S // 2, S - 1, S] + [ro.n_tail_of(a, S) for a in (0.5, 0.9, 0.95)]
    return sorted({min(max(t, 1), S) for t in cand})


def cvar_ref(preds, n_tail):
    """(fp64 mean of the n_tail smallest per column, per-column bound for an fp32 kernel that selects
    exactly: n_tail 2^-24 mean|tail| for the fp32 sum in any order, 2^-24 |mean| for the division)."""
    tail = np.sort(preds.astype(np.float64), axis=0)[:n_tail]
    want = tail.mean(axis=0)
    tol = n_tail * 2.0 ** -24 * np.abs(tail).mean(axis=0) + 2.0 ** -24 * np.abs(want)
    return want, tol


# ---------------------------------------------------------------------------------------------
# Envelope tests of the trainer's forward entry point (iqlhip_forward, tests/test_gpu_forward_envelope.py):
# random networks under the trainer's state_dict names, a second bf16 restatement that accumulates in
# fp64 (the yardstick of what two correct bf16 forwards may differ by) and bf16 ulps.
# ---------------------------------------------------------------------------------------------
def forward_nets(rng, S, A, H, n_hidden=2, n_critics=2, deterministic=False, dropout=None):
    """(qf, vf, actor) fp32 parameter dicts under the state_dict names of TwinQ / EnsembleQ, ValueFunction
    and the policies, from mlp_weights_for (O(1) activations), nn.Linear's [out, in] layout; every critic
    is its own draw.  A Sequential with Dropout layers counts them in its indices (0, 3, 6 for 0, 2, 4)."""
    def mlp(prefix, dims, step):
        ws, bs = mlp_weights_for(rng, dims)
        out = {}
        for l, (w, b) in enumerate(zip(ws, bs)):
            out[f"{prefix}{step * l}.weight"] = np.ascontiguousarray(w.T)
            out[f"{prefix}{step * l}.bias"] = b
        return out
    hid = [H] * n_hidden
    qf = {}
    for e in range(n_critics):
        qf.update(mlp(f"q{e + 1}.net.", [S + A] + hid + [1], 2))
    vf = mlp("v.net.", [S] + hid + [1], 2)
    actor = {} if deterministic else {"log_std": np.linspace(-0.5, 0.3, A).astype(np.float32)}
    actor.update(mlp("net.net.", [S] + hid + [A], 2 if dropout is None else 3))
    return qf, vf, actor


def net_layers(params, prefix):
    """([in, out] weights, biases) of the Linear layers under ``prefix``, as mlp_forward_ref takes them."""
    keys = orc.linear_keys(params, prefix)
    return [np.ascontiguousarray(params[w].T) for w, _ in keys], [params[b] for _, b in keys]


def bf16_from_f64(y):
    """fp64 -> bfloat16 in ONE nearest-even rounding (8 significant bits), returned as fp64.  (Through
    fp32 it would be two roundings.)  Normal numbers only: nothing here comes near 2^-126."""
    m, e = np.frexp(np.asarray(y, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def mlp_forward_bf16_f64(x, params, prefix, out_act=None):
    """The autocast MLP forward of oracle/iql_oracle.py:mlp_forward (eval mode) with the same operands
    rounded to bf16, every sum in fp64 and each Linear's result rounded to bf16 once: a second correct
    bf16 forward.  Where it and the oracle (fp32 sums) differ, a rounding tie fell the other way."""
    h = orc.bf16(np.asarray(x, dtype=np.float32)).astype(np.float64)
    keys = orc.linear_keys(params, prefix)
    for l, (wk, bk) in enumerate(keys):
        z = bf16_from_f64(h @ orc.bf16(params[wk]).astype(np.float64).T + orc.bf16(params[bk]).astype(np.float64))
        h = np.maximum(z, 0.0) if l < len(keys) - 1 else z
    return bf16_from_f64(np.tanh(h)) if out_act == "tanh" else h


def bf16_ulp(x):
    """Spacing of bfloat16 at |x|: 2^-7 of its binade."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, e - 1 - 7)
