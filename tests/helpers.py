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


FWD_TOL = 2e-5  # the project's rtol = atol for fp32 forwards of up to four Linear layers, width <= 256


def forward_reference(params, mode, s, a):
    """which -> (reference [n, width] in fp64, |second CPU forward - reference| per element) of the four
    forwards "q" | "v" | "actor" | "q_target" on ``params`` = (qf, vf, actor, q_target) parameter dicts.
    fp32: mlp_forward_ref in fp64, the second forward the same in fp32 numpy; bf16: the oracle's autocast
    restatement, the second forward mlp_forward_bf16_f64."""
    qf, vf, actor, qt = params
    sa = np.concatenate([s, a], axis=1)
    out = {}
    if mode == "fp32":
        def pair(p, prefix, x, out_act):
            ws, bs = net_layers(p, prefix)
            want = mlp_forward_ref(ws, bs, x, 0, out_act)
            return want, np.abs(mlp_forward_ref(ws, bs, x, 0, out_act, dtype=np.float32).astype(np.float64) - want)
        for which, q in (("q", qf), ("q_target", qt)):
            cols = [pair(q, f"q{e + 1}.net.", sa, 0) for e in range(orc.n_critics(q))]
            out[which] = tuple(np.concatenate(c, axis=1) for c in zip(*cols))
        out["v"] = pair(vf, "v.net.", s, 0)
        out["actor"] = pair(actor, "net.net.", s, 1)
        return out
    for which, q in (("q", qf), ("q_target", qt)):
        want = np.stack(orc.critics_all(q, s, a, "bf16")[0], axis=1).astype(np.float64)
        other = np.concatenate([mlp_forward_bf16_f64(sa, q, f"q{e + 1}.net.") for e in range(orc.n_critics(q))], axis=1)
        out[which] = (want, np.abs(other - want))
    want = orc.value_forward(vf, s, "bf16")[0][:, None].astype(np.float64)
    out["v"] = (want, np.abs(mlp_forward_bf16_f64(s, vf, "v.net.") - want))
    want = orc.policy_forward(actor, s, "bf16")[0].astype(np.float64)
    out["actor"] = (want, np.abs(mlp_forward_bf16_f64(s, actor, "net.net.", "tanh") - want))
    return out


def forward_judge(mode, got, want, gap, n_lin, width):
    """(within the bounds of tests/test_gpu_forward_envelope.py's docstring?, the figures as text)."""
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    if mode == "fp32":
        if n_lin <= 4 and width <= 256:
            bound, lim = f"rtol = atol = {FWD_TOL:.0e}", FWD_TOL + FWD_TOL * np.abs(want)
        else:
            atol = max(4 * float(gap.max()), FWD_TOL)
            bound, lim = f"atol {atol:.2e}", atol
        return bool(np.all(err <= lim)), f"max |err| {err.max():.3e} ({bound}; fp32 numpy vs fp64: gap {gap.max():.3e})"
    max_b = max(4 * float(gap.max()), 2 * float(bf16_ulp(np.abs(want).max())))
    med_b = max(4 * float(np.median(gap)), 0.25 * float(bf16_ulp(np.median(np.abs(want)))))
    ok = err.max() <= max_b and np.median(err) <= med_b
    return bool(ok), (f"max |err| {err.max():.3e} (bound {max_b:.3e}), median {np.median(err):.3e} (bound {med_b:.3e}), "
                      f"bit-identical {np.mean(err == 0):.3f}; the CPU pair: max gap {gap.max():.3e}, median {np.median(gap):.3e}")


# ---------------------------------------------------------------------------------------------
# Preference-transformer relabel (tests/test_gpu_relabel.py, test_gpu_pt_general.py,
# test_gpu_pt_envelope.py): windows, their oracle values, the two bounds, and the cases of the
# envelope tests with their inputs -- numpy only, so that tests/test_relabel_oracle.py can show on
# the host that the reference alone stays inside the bounds.
# ---------------------------------------------------------------------------------------------
PT_TOL = 5e-3            # absorbs bf16 rounding flips of a q.k logit
PT_TIGHT_MEDIAN = 1e-5   # on short windows: a wrong tile or head split errs by the size of the values


def oracle_windows(p, obs, act, starts, lens, t0, QL, heads, dtype=np.float32, trim=False):
    """pt_value_last of right-aligned windows (start, len, t0), batched.  dtype=np.float64: the
    high-precision mode of the oracle, returned as float64.  trim=True (the long cases: the cost of a
    forward grows with the square of its padded length): the windows go in order of length and a
    batch is padded to ITS longest window instead of to QL -- a pad key weighs exp(-1e4 - max) = 0
    exactly, so the number of pads moves a value by the order of a float sum of zeros at most
    (tests/test_relabel_oracle.py holds the float64 mode to 1e-12 on this)."""
    from oracle import relabel_oracle as ro
    n, S, A = len(lens), obs.shape[1], act.shape[1]
    order = np.argsort(lens, kind="stable") if trim else np.arange(n)
    out = np.empty(n, dtype)
    for b in range(0, n, 32 if trim else 64):
        idx = order[b:b + (32 if trim else 64)]
        pad = int(max(lens[i] for i in idx)) if trim else QL
        sts = np.zeros((len(idx), pad, S), np.float32); acs = np.zeros((len(idx), pad, A), np.float32)
        ts = np.zeros((len(idx), pad), np.int64); am = np.zeros((len(idx), pad), np.float32)
        for r, i in enumerate(idx):
            s0, l0 = int(starts[i]), int(lens[i])
            sts[r, pad - l0:] = obs[s0:s0 + l0]; acs[r, pad - l0:] = act[s0:s0 + l0]
            ts[r, pad - l0:] = (0 if t0 is None else int(t0[i])) + np.arange(l0); am[r, pad - l0:] = 1
        out[idx] = ro.pt_value_last(p, sts, acs, ts, am, num_heads=heads, dtype=dtype)
    return out


def oracle_prefixes(p, obs, act, start, n, t0, heads, dtype=np.float32):
    """ONE forward over the n transitions from row ``start`` (timesteps t0 ..), values at every
    position: because attention is causal, entry l - 1 is the value of the window (start, l, t0)
    (include/iqlhip.h; the pads of the shorter window weigh exactly 0)."""
    from oracle import relabel_oracle as ro
    ts = (t0 + np.arange(n))[None]
    return ro.pt_value_last(p, obs[None, start:start + n], act[None, start:start + n], ts,
                            np.ones((1, n), np.float32), num_heads=heads, all_positions=True, dtype=dtype)[0]


def random_windows(rng, n_rows, max_ep, QL, n_extra, lengths=None):
    """Every length 1..QL once (or each of ``lengths``), then random ones, then windows sharing rows
    with earlier ones."""
    first = np.arange(1, QL + 1) if lengths is None else np.asarray(lengths)
    lens = np.concatenate([first, rng.integers(1, QL + 1, n_extra)]).astype(np.int32)
    starts = np.array([rng.integers(0, n_rows - l + 1) for l in lens], np.int64)
    t0 = np.array([rng.integers(0, max_ep + 2 - l) for l in lens], np.int32)
    # the same rows again under other lengths / timesteps
    k = min(16, len(lens))
    lens2 = rng.integers(1, QL + 1, k).astype(np.int32)
    starts2 = np.minimum(starts[:k], n_rows - lens2)
    t02 = np.array([rng.integers(0, max_ep + 2 - l) for l in lens2], np.int32)
    return (np.concatenate([lens, lens2]), np.concatenate([starts, starts2]), np.concatenate([t0, t02]))


def check_close(got, want, short=None):
    """Loose bound everywhere; the tight median bound on all windows, or on `short` (a mask)."""
    d = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=PT_TOL, atol=PT_TOL)
    sel = d if short is None else d[short]
    assert np.median(sel) <= PT_TIGHT_MEDIAN, (float(d.max()), float(np.median(sel)))
    return float(d.max()), float(np.median(d))


# The envelope cases, every one as (L, E, heads, I, S, A, QL).  Tuned kernel (k_pt_relabel: one block,
# embd 64): nks = 16-deep k-steps of the embedding GEMM, walked in chunks of KCH = 3; nmt = 16-token
# tiles per kind, 2 nmt jobs on 8 waves; nkq = k-steps per K half of the MLP out projection.
PT_TUNED_CASES = [
    (1, 64, 1, 256, 1, 1, 1),        # smallest: one token pair, one job
    (1, 64, 4, 256, 49, 3, 6),       # first second chunk, state: nks_s = 4 = one chunk + a partial one
    (1, 64, 4, 256, 3, 49, 6),       # the same on the side prepare_query uses
    (1, 64, 2, 1024, 96, 96, 20),    # whole chunks, S + A = 192, no padding column, LDS > 80 KiB
    (1, 64, 8, 768, 191, 1, 12),     # twelve k-steps, the last padded by one input; nkq = 24
    (1, 64, 16, 1024, 29, 8, 20),    # widest MLP (nkq = 32), most heads (head_dim 4)
    (1, 64, 4, 256, 5, 3, 129),      # three job rounds: nmt = 9
    (1, 64, 1, 512, 5, 3, 300),      # many job rounds: nmt = 19
]
PT_TUNED_WIDEST = PT_TUNED_CASES[3]
# General path (k_lin, k_attn, k_last_rows, k_value_head): head_dim HD = E / heads over HDL lanes,
# DPL = HD / HDL features per lane, G = 64 / HDL key groups; tp = row pitch of a window, 32-row tiles.
PT_GENERAL_CASES = [
    (2, 256, 1, 64, 5, 3, 9),        # HD 256: HDL 64, DPL 4, G 1
    (2, 128, 1, 128, 5, 3, 9),       # HD 128: 64, 2, 1
    (2, 256, 2, 256, 5, 3, 9),       # HD 128: 64, 2, 1
    (2, 192, 1, 192, 5, 3, 9),       # HD 192: 64, 3, 1
    (2, 192, 2, 192, 5, 3, 9),       # HD 96: 32, 3, 2
    (2, 192, 4, 192, 5, 3, 9),       # HD 48: 16, 3, 4
    (2, 192, 16, 192, 5, 3, 9),      # HD 12: 4, 3, 16
    (2, 192, 32, 192, 5, 3, 9),      # HD 6: 2, 3, 32
    (2, 64, 8, 64, 5, 3, 9),         # HD 8: 8, 1, 8
    (2, 128, 32, 128, 5, 3, 9),      # HD 4: 4, 1, 16
    (2, 256, 64, 1024, 5, 3, 9),     # HD 4, most heads, widest MLP
    (2, 64, 4, 64, 255, 1, 6),       # widest input, the split at the state end
    (2, 64, 4, 64, 1, 255, 6),       # widest input, the split at the action end
    (1, 128, 4, 256, 128, 128, 6),   # widest input, even
    (2, 64, 4, 64, 5, 3, 1),         # one transition: tp = 32, two real tokens
    (2, 64, 4, 64, 5, 3, 16),        # full tile: 2 QL = 32 rows exactly
    (2, 64, 4, 64, 5, 3, 17),        # one past the tile: tp = 64, short windows skip tile 2
]
# Long windows of the general path: prefixes of ONE stretch of rows (oracle_prefixes).
PT_GENERAL_LONG = (2, 64, 4, 64, 5, 3, 1024)
PT_GENERAL_TOP = (2, 64, 1, 64, 5, 3, 4096)
# Seeds: the shape itself unless a case is listed here.  (A listed case did not pass the float32 vs
# float64 check of tests/test_relabel_oracle.py with its own seed: a bf16 flip of a logit that weighs.)
PT_CASE_SEEDS = {}


def pt_case_id(case):
    return "L%d-E%d-h%d-I%d-S%d-A%d-QL%d" % case


def pt_case_rng(case):
    return np.random.default_rng(PT_CASE_SEEDS.get(case, list(case)))


def pt_case_lengths(QL, rng):
    """Every length 1..QL up to 129; beyond, about 120 of them: both neighbours of every multiple of
    16 (a token tile) up to 64, of every multiple of 64 (a job round of the tuned kernel: 8 jobs of
    16 tokens of one kind), the ends, and random ones."""
    if QL <= 129:
        return None
    edges = {1, 2, QL - 1, QL}
    for m in list(range(16, 65, 16)) + list(range(64, QL, 64)):
        edges |= {m - 1, m, m + 1}
    edges = {l for l in edges if 1 <= l <= QL}
    rest = np.setdiff1d(np.arange(1, QL + 1), sorted(edges))
    return np.sort(np.concatenate([sorted(edges), rng.choice(rest, 118 - len(edges), replace=False)]))


def pt_case_inputs(case):
    """(p, obs, act, lens, starts, t0, max_ep) of one envelope case: seeded random weights
    (oracle.relabel_oracle.make_pt_params), a few hundred dataset rows, every length 1..QL once plus 16
    random windows plus 16 that share rows with earlier ones (random_windows)."""
    from oracle import relabel_oracle as ro
    L, E, heads, I, S, A, QL = case
    rng = pt_case_rng(case)
    max_ep = max(150, QL + 20)
    p = ro.make_pt_params(rng, S, A, max_ep, embd=E, pref=8, inter=I, layers=L)
    n_rows = max(300, QL + 200)
    obs = rng.standard_normal((n_rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    lens, starts, t0 = random_windows(rng, n_rows, max_ep, QL, 16, lengths=pt_case_lengths(QL, rng))
    return p, obs, act, lens, starts, t0, max_ep


def pt_prefix_inputs(case, n, lengths, n_random):
    """(p, obs, act, start, t0, lens, max_ep) of a long case: the windows are the prefixes ``lengths``,
    and ``n_random`` more, of the n transitions from row ``start``, first timestep t0."""
    from oracle import relabel_oracle as ro
    L, E, heads, I, S, A, QL = case
    rng = pt_case_rng(case)
    max_ep = QL + 50
    p = ro.make_pt_params(rng, S, A, max_ep, embd=E, pref=8, inter=I, layers=L)
    n_rows = n + 64
    obs = rng.standard_normal((n_rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    start, t0 = int(rng.integers(1, n_rows - n)), int(rng.integers(1, max_ep + 2 - n))
    lens = np.concatenate([lengths, rng.integers(1, n + 1, n_random)]).astype(np.int32)
    return p, obs, act, start, t0, lens, max_ep


def pt_clamp_windows(starts, lens, t0, n_rows, n_temb, QL):
    """The rule of include/iqlhip.h as both load_window functions implement it: the length into
    [1, min(QL, n_rows, n_temb)], then the start into [0, n_rows - len] and the first timestep into
    [0, n_temb - len]."""
    lens = np.maximum(np.minimum(np.asarray(lens, np.int64), min(QL, n_rows, n_temb)), 1)
    starts = np.clip(np.asarray(starts, np.int64), 0, n_rows - lens)
    t0 = np.clip(np.asarray(t0, np.int64), 0, n_temb - lens)
    return starts.astype(np.int64), lens.astype(np.int32), t0.astype(np.int32)


# ---------------------------------------------------------------------------------------------
# Envelope tests of the general layer-wise training step (csrc/iql_deep.hip: kd_backward / kd_update;
# tests/test_gpu_general_step_envelope.py and, on the host, tests/test_general_step_envelope_host.py).
# Every step is judged at the parameters the GPU held BEFORE it: the references below take a state
# (qf, vf, actor, q_target) and one batch, and return that single step's losses and gradients.
# ---------------------------------------------------------------------------------------------
GS_LR = 1e-2          # one sign-like Adam step moves every weight by several bf16 ulps (largest ulp ~1e-3 at fan-in 17)
GS_ROWS = 200
GS_STEPS = 2          # step 1 on kd_sync's copies, step 2 on the copies kd_update wrote
GS_MARGIN = 1e-5      # the project's kink threshold (_shape_case)
GS_GRAD_TOL = 5e-5    # fp32 gradients, of the largest reference entry (_shape_case)
GS_BF16_FLOOR = 2e-2  # bf16 gradients: the project's 2e-2 of the largest entry (_shape_case)
GS_LOSS_RTOL = {"fp32": 3e-5, "bf16": 6e-3}
GS_HYPER = dict(iql_tau=0.8, beta=3.0, max_steps=1000, discount=0.99, tau=0.005)
GS_ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)  # torch.optim.Adam's defaults

# id -> (S, A, n_hidden, H, B, E, deterministic, dropout, offset biases, numpy seed, tq, orientation of the hidden
# and output layers).  seed: the first that gs_pick_seed accepts (the reference's own two steps keep every net
# 2e-5 from a kink and its bf16 restatements agree within the test's bounds; B >= 1024 cannot avoid a kink, any seed).  tq / orientation: what the case is meant to reach, checked
# against gs_update_plan, the rule of deep_create restated.
GS_CASES = {
    # hidden width not a multiple of 4: dW = dZ^T X on hidden and output layers
    "1x1": (12, 5, 1, 1, 16, 2, False, None, False, 0, 1, "dzT_x"),
    "2x3_det": (11, 5, 2, 3, 16, 2, True, None, False, 0, 1, "dzT_x"),
    "3x17_b17": (12, 5, 3, 17, 17, 2, False, None, False, 1, 1, "dzT_x"),
    "6x33_det": (11, 5, 6, 33, 16, 2, True, None, False, 10, 1, "dzT_x"),
    "2x65_b32_e3": (17, 6, 2, 65, 32, 3, False, None, False, 0, 1, "dzT_x"),
    "3x129": (17, 6, 3, 129, 16, 2, False, None, False, 10, 1, "dzT_x"),
    "2x257_det": (17, 6, 2, 257, 16, 2, True, None, False, 15, 1, "dzT_x"),
    "1x1023_offset": (17, 6, 1, 1023, 16, 2, False, None, True, 1, 1, "dzT_x"),
    "2x765_offset": (17, 6, 2, 765, 16, 2, False, None, True, 2, 4, "dzT_x"),
    # multiples of 4 at the boundaries: dW^T = X^T dZ
    "2x4": (17, 6, 2, 4, 16, 2, False, None, False, 0, 1, "xT_dz"),
    "3x36_det": (17, 6, 3, 36, 16, 2, True, None, False, 4, 1, "xT_dz"),
    "2x68_b48": (17, 6, 2, 68, 48, 2, False, None, False, 3, 1, "xT_dz"),
    "2x768_offset": (17, 6, 2, 768, 16, 2, False, None, True, 0, 4, "xT_dz"),
    "6x1024_offset": (17, 6, 6, 1024, 16, 2, False, None, True, 28, 4, "xT_dz"),
    # tq = 4 reached by batch size, and just under the rule
    "2x129_b1024_e8": (12, 5, 2, 129, 1024, 8, False, None, False, 0, 4, "dzT_x"),
    "2x192_b1024_e8": (12, 5, 2, 192, 1024, 8, False, None, False, 0, 4, "xT_dz"),
    "2x129_b1024_e7": (12, 5, 2, 129, 1024, 7, False, None, False, 0, 1, "dzT_x"),
    # input and output widths at an odd hidden width
    "s15a17_2x21": (15, 17, 2, 21, 16, 2, False, None, False, 0, 1, "dzT_x"),
    "s96a32_1x7_det": (96, 32, 1, 7, 16, 2, True, None, False, 0, 1, "dzT_x"),
    "s1a1_2x5": (1, 1, 2, 5, 16, 2, False, None, False, 0, 1, "dzT_x"),
    # dropout at an odd width
    "3x33_b17_dropout": (12, 5, 3, 33, 17, 2, False, 0.25, False, 1, 1, "dzT_x"),
}
GS_DAMAGE_CASES = ("3x17_b17", "2x768_offset")  # where the host test shows what the bounds reject


def _round_up(x, m):
    return (x + m - 1) // m * m


def gs_case(case):
    """The table row of a case id, from GS_CASES or TS_CASES (one layout up to the seed; the ids do not collide); a row
    that is in neither table is passed as the tuple itself."""
    if not isinstance(case, str):
        return case
    return GS_CASES[case] if case in GS_CASES else TS_CASES[case]


def gs_update_plan(S, A, NH, H, B, E):
    """(tq, orientation of the layers with H in-features, the count ``wide``) kd_update runs at, restated from deep_create
    (csrc/iql_deep.hip): 64 x 64 tiles (tq = 4) when (BP >= 1024 or Hp >= 768) and the 64 x 64 tiles of all
    trained tensors number >= 150, else 64 x 16 (tq = 1); a layer whose in-feature count is a multiple of 4
    is computed transposed (dW^T = X^T dZ, "xT_dz"), any other as dW = dZ^T X ("dzT_x")."""
    BP, Hp = _round_up(_round_up(B, 16), 32), _round_up(H, 32)
    wide = 0
    for n_in, n_out in [(S + A, 1)] * E + [(S, 1), (S, A)]:
        dims = [n_in] + [H] * NH + [n_out]
        wide += sum(-(-dims[l + 1] // 64) * -(-dims[l] // 64) for l in range(NH + 1))
    return (4 if (BP >= 1024 or Hp >= 768) and wide >= 150 else 1), ("xT_dz" if H % 4 == 0 else "dzT_x"), wide


def gs_inputs(case, seed=None):
    """(hyper, (qf, vf, actor), data, indices [GS_STEPS, B]) of a case: forward_nets' weights from the case's
    numpy seed, _shape_case's data on GS_ROWS rows.  Offset cases: hidden-layer biases + 3 (unit index % 4 != 3)
    or - 3: most of their units are on or off for the whole batch (3 to 15 % of V's see both signs at step 1), which
    keeps wide layers' thousands of pre-activations away from the kink -- they test tile geometry, the per-sample
    relu' masks are the small cases' part."""
    S, A, NH, H, B, E, det, drop, offset, case_seed = gs_case(case)[:10]
    rng = np.random.default_rng([case_seed if seed is None else seed, S, A, NH, H, B, E])
    nets = forward_nets(rng, S, A, H, NH, E, det, drop)
    if offset:
        shift = np.where(np.arange(H) % 4 != 3, 3.0, -3.0).astype(np.float32)
        for net, prefixes in zip(nets, ([f"q{e + 1}.net." for e in range(E)], ["v.net."], ["net.net."])):
            for prefix in prefixes:
                for _, bk in orc.linear_keys(net, prefix)[:-1]:
                    net[bk] = (net[bk] + shift).astype(np.float32)
    N = GS_ROWS
    data = {"observations": rng.standard_normal((N, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (N, A)).astype(np.float32),
            "rewards": rng.standard_normal(N).astype(np.float32),
            "next_observations": rng.standard_normal((N, S)).astype(np.float32),
            "terminals": (rng.uniform(size=N) < 0.05).astype(np.float32)}
    idx = rng.integers(0, N, (GS_STEPS, B)).astype(np.int64)
    hyper = dict(GS_HYPER, s_dim=S, a_dim=A, hidden=H, n_hidden=NH, n_critics=E, deterministic=det, dropout=drop,
                 n_rows=N, batch=B)
    return hyper, nets, data, idx


def gs_oracle_at(hyper, state, mode, total_it, acc=np.float32):
    """An IQLOracle holding ``state`` = (qf, vf, actor, q_target) after ``total_it`` steps."""
    qf, vf, actor, qt = state
    o = orc.IQLOracle(qf, vf, actor, iql_tau=hyper["iql_tau"], beta=hyper["beta"], max_steps=hyper["max_steps"],
                      discount=hyper["discount"], tau=hyper["tau"], lr=GS_LR, mode=mode, dropout=hyper["dropout"], acc=acc)
    o.q_target = {k: np.array(v, dtype=np.float32) for k, v in qt.items()}
    o.total_it = total_it
    return o


def gs_f64_step(hyper, state, batch, keeps=None):
    """float64 autograd of the three IQL losses (ref:581-637) at ``state``, on plain torch tensors:
    target_q = min_e q_target, detached; next_v detached; exp_adv detached and clamped at 100; the Gaussian
    term -Normal(mean, exp(clamp(log_std))).log_prob(a).sum(-1).  Two tensors are held as the fp32 numbers the
    step stores: the tanh output, which its backward reads (ATen's tanh_backward: g (1 - out^2)), and the detached
    weight exp_adv.  Where they saturate or underflow -- the wide offset cases at step 2: |pre-tanh| > 16,
    exp(beta adv) below 1e-45 -- the fp32 FORMAT decides that a gradient is exactly zero, not a summation order,
    and a reference that ignored it would call that zero wrong; anywhere else the rounding moves the result by
    1e-7 of itself.  Returns (losses, grads, margin) in the oracle's layout: margin[group] = the smallest hidden |pre-activation| of the group's trained forwards,
    for V also min |adv| (IQLOracle.last_margin)."""
    import torch
    t64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    as_f32 = lambda x: x.float().double()

    class TanhStoredF32(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = as_f32(torch.tanh(x))
            ctx.save_for_backward(out)
            return out

        @staticmethod
        def backward(ctx, g):
            out, = ctx.saved_tensors
            return g * (1.0 - out * out)

    qf, vf, actor, qt = ({k: t64(v) for k, v in d.items()} for d in state)
    for d in (qf, vf, actor):
        for v in d.values():
            v.requires_grad_(True)
    s, a, r, s2, d = [t64(x) for x in batch]
    r, d = r.reshape(-1), d.reshape(-1)
    scale = None if keeps is None else float(np.float32(1.0) / np.float32(1.0 - hyper["dropout"]))

    def mlp(x, p, prefix, keeps=None):
        keys, margin = orc.linear_keys(p, prefix), np.inf
        for l, (wk, bk) in enumerate(keys):
            x = x @ p[wk].T + p[bk]
            if l < len(keys) - 1:
                margin = min(margin, float(x.detach().abs().min()))
                x = torch.relu(x)
                if keeps is not None:
                    x = x * (t64(keeps[l]) * scale)
        return x, margin

    E = orc.n_critics(qf)
    with torch.no_grad():
        next_v = mlp(s2, vf, "v.net.")[0][:, 0]
        target_q = torch.stack([mlp(torch.cat([s, a], 1), qt, f"q{e + 1}.net.")[0][:, 0] for e in range(E)]).min(0).values
    v, m_v = mlp(s, vf, "v.net.")
    adv = target_q - v[:, 0]
    value_loss = ((hyper["iql_tau"] - (adv < 0).double()).abs() * adv ** 2).mean()
    targets = r + (1.0 - d) * hyper["discount"] * next_v
    qs = [mlp(torch.cat([s, a], 1), qf, f"q{e + 1}.net.") for e in range(E)]
    q_loss = sum(((q[:, 0] - targets) ** 2).mean() for q, _ in qs) / E
    exp_adv = as_f32(torch.exp(hyper["beta"] * adv.detach()).clamp(max=orc.EXP_ADV_MAX))
    out, m_a = mlp(s, actor, "net.net.", keeps)
    mean = TanhStoredF32.apply(out)
    if "log_std" in actor:
        std = torch.exp(actor["log_std"].clamp(orc.LOG_STD_MIN, orc.LOG_STD_MAX))
        bc = -torch.distributions.Normal(mean, std).log_prob(a).sum(-1)
    else:
        bc = ((mean - a) ** 2).sum(1)
    policy_loss = (exp_adv * bc).mean()
    (value_loss + q_loss + policy_loss).backward()  # (three disjoint parameter sets: one backward)
    grads = {g: {k: t.grad.numpy() for k, t in p.items()} for g, p in (("q", qf), ("v", vf), ("actor", actor))}
    margin = {"v": min(m_v, float(adv.detach().abs().min())), "q": min(m for _, m in qs), "actor": m_a}
    return {"value_loss": value_loss.item(), "q_loss": q_loss.item(), "actor_loss": policy_loss.item()}, grads, margin


def gs_reference_step(hyper, state, mode, batch, total_it, keeps=None):
    """The reference of ONE step at ``state``: {"losses": the oracle's in ``mode``, "grads": group -> name ->
    array, "gap": the same layout or None, "margin": group -> float}.
    fp32: gradients and margins from gs_f64_step.  bf16: the oracle in "bf16" mode; gap = what the same
    restatement with every sum in fp64 (acc=float64) differs by, elementwise."""
    o = gs_oracle_at(hyper, state, mode, total_it)
    losses = o.train(batch, keeps)
    if mode == "fp32":
        _, grads, margin = gs_f64_step(hyper, state, batch, keeps)
        return {"losses": losses, "grads": grads, "gap": None, "margin": margin, "oracle_grads": o.last_grads}
    o64 = gs_oracle_at(hyper, state, mode, total_it, acc=np.float64)
    o64.train(batch, keeps)
    gap = {g: {k: np.abs(o64.last_grads[g][k].astype(np.float64) - w) for k, w in d.items()} for g, d in o.last_grads.items()}
    return {"losses": losses, "grads": o.last_grads, "gap": gap, "margin": o.last_margin}


def gs_loose_bound(mode, B):
    """The project's bound for a net within GS_MARGIN of a kink (_shape_case): a few samples' share."""
    return max(4.0 / B, GS_BF16_FLOOR if mode == "bf16" else 0.0)


def gs_judge_grad(mode, got, want, gap=None, loose=None):
    """One gradient tensor against its reference: (ok, figures as text, max |err| / max |reference|, share of
    bit-identical entries).  A reference that is identically zero must be met exactly.  Errors are relative to
    the largest reference entry.
      fp32  max |err| <= GS_GRAD_TOL
      bf16  max |err| <= max(4 x max gap, GS_BF16_FLOOR), median |err| <= max(4 x median gap, a quarter bf16 ulp
            at the median |reference|)
      loose (a float: the net is within GS_MARGIN of a kink in this step) max |err| <= loose, nothing else."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, top = np.abs(got - want), float(np.abs(want).max())
    same = float(np.mean(err == 0))
    if top == 0.0:
        return bool(err.max() == 0.0), f"zero reference, max |got| {err.max():.3e}", float(err.max() != 0), same
    rel = float(err.max()) / top
    if loose is not None:
        return rel <= loose, f"max {rel:.3e} of the largest entry (LOOSE bound {loose:.2e})", rel, same
    if mode == "fp32":
        return rel <= GS_GRAD_TOL, f"max {rel:.3e} of the largest entry (bound {GS_GRAD_TOL:.0e})", rel, same
    max_b = max(4 * float(gap.max()), GS_BF16_FLOOR * top)
    med_b = max(4 * float(np.median(gap)), 0.25 * float(bf16_ulp(np.median(np.abs(want)))))
    ok = err.max() <= max_b and np.median(err) <= med_b
    return bool(ok), (f"max {rel:.3e} of the largest entry (bound {max_b / top:.3e}), median |err| {np.median(err):.3e} "
                      f"(bound {med_b:.3e}), bit-identical {same:.4f}; max gap {gap.max() / top:.3e}"), rel, same


def gs_judge_grads(mode, got, ref, B, groups=("q", "v", "actor")):
    """Every tensor of ``got`` (group -> name -> array) against ``ref`` (gs_reference_step): (failures as text,
    report lines, groups judged under the loose bound, largest relative error under the tight bounds, share of
    bit-identical entries over all tensors but the fp32 log_std)."""
    bad, lines, loose_groups, worst, n_same, n_all = [], [], [], 0.0, 0.0, 0
    for g in groups:
        loose = gs_loose_bound(mode, B) if ref["margin"][g] < GS_MARGIN else None
        if loose is not None:
            loose_groups.append(g)
        assert got[g].keys() == ref["grads"][g].keys()
        for k, want in ref["grads"][g].items():
            ok, text, rel, same = gs_judge_grad(mode, got[g][k], want, None if ref["gap"] is None else ref["gap"][g][k], loose)
            lines.append(f"grad {g}/{k} (margin {ref['margin'][g]:.1e}): {text}")
            if loose is None:
                worst = max(worst, rel)
            if k != "log_std":
                n_same, n_all = n_same + same * want.size, n_all + want.size
            if not ok:
                bad.append(lines[-1])
    return bad, lines, loose_groups, worst, n_same / n_all


def gs_adam_coef(step, lr, lr_actor_base, t_max):
    """make_adam_coef (csrc/step_math.h) for the step whose 1-based count is ``step``: the coefficients are
    formed in double and rounded to float; returned as the floats' values in float64.  neg_step: q, v, actor
    (the actor's lr on the cosine schedule after step - 1 scheduler steps)."""
    b1, b2, eps = GS_ADAM["beta1"], GS_ADAM["beta2"], GS_ADAM["eps"]
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    lr_a = lr_actor_base * (1.0 + np.cos(np.pi * (step - 1) / t_max)) * 0.5
    f = lambda x: float(np.float32(x))
    return dict(one_m_b1=f(1.0 - b1), b2=f(b2), one_m_b2=f(1.0 - b2), bc2_sqrt=f(np.sqrt(bc2)), eps=f(eps),
                neg_step={"q": f(-(lr / bc1)), "v": f(-(lr / bc1)), "actor": f(-(lr_a / bc1))})


def ulp32(x):
    """Spacing of float32 at |x| (normal numbers; the smallest normal's below)."""
    _, e = np.frexp(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126))
    return np.ldexp(1.0, e - 1 - 23)


def gs_judge_update(coef, group, p0, m0, v0, g, p1, m1, v1, lr, t0=None, t1=None, tau=None):
    """Adam and Polyak of one tensor from the GPU's own numbers, in float64 (adam_apply / polyak of
    csrc/step_math.h):  m = m0 + (g - m0)(1 - b1);  v = b2 v0 + (1 - b2) g g;  p = p0 - step m / (sqrt(v) /
    sqrt(bc2) + eps);  t = t0 + tau (p1 - t0) on the GPU's new p.  The two lerps are ATen's form, one fused
    multiply-add over the fp32-ROUNDED difference: the reference takes that difference as the fp32 number it is
    and does the rest in float64, so what is left to the kernel is the last rounding -- also where the two terms
    cancel (m0 = -g / 9, t0 = -tau p1: a few entries of a million), where half an ulp of the difference is many
    ulps of the result.  Bounds (derived, not fitted):
      moments    1e-6 relative, floor 1e-37 (g g underflows).
      parameter  1 ulp32(p) + 1e-5 lr: adam_apply is about six fp32 operations on float-rounded coefficients,
                 in bf16 mode with the hardware's 1-ulp sqrt / rcp (3e-7 of the step): ~1e-6 of an update <= lr.
      target     2 ulp32(t).
    Returns (failures, {"m": largest error / tolerance unit, ...}: moments in units of 1e-6 relative, the
    parameter's distance from p_ref in ulp32 and what of it exceeds one ulp32 in units of lr, the target in ulp32)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    p0, m0, v0, g, p1, m1, v1 = map(f, (p0, m0, v0, g, p1, m1, v1))
    f32_diff = lambda a, b: (a.astype(np.float32) - b.astype(np.float32)).astype(np.float64)  # (a, b hold fp32 values)
    m = m0 + f32_diff(g, m0) * coef["one_m_b1"]
    v = coef["b2"] * v0 + (coef["one_m_b2"] * g) * g
    p = p0 + coef["neg_step"][group] * (m / (np.sqrt(v) / coef["bc2_sqrt"] + coef["eps"]))
    bad, fig = [], {}
    fig["m"] = float((np.maximum(np.abs(m1 - m) - 1e-37, 0) / np.maximum(np.abs(m), 1e-300)).max() / 1e-6)
    fig["v"] = float((np.maximum(np.abs(v1 - v) - 1e-37, 0) / np.maximum(v, 1e-300)).max() / 1e-6)
    dp = np.abs(p1 - p)
    fig["p_ulp"], fig["p_lr"] = float((dp / ulp32(p)).max()), float(np.maximum(dp - ulp32(p), 0).max() / lr)
    if fig["m"] > 1.0:
        bad.append(f"exp_avg off by {fig['m']:.3g} x 1e-6")
    if fig["v"] > 1.0:
        bad.append(f"exp_avg_sq off by {fig['v']:.3g} x 1e-6")
    if np.any(dp > ulp32(p) + 1e-5 * lr):
        bad.append(f"parameter off by {fig['p_ulp']:.3g} ulp32 / {fig['p_lr']:.3g} lr at the worst entry")
    if t0 is not None:
        t = f(t0) + tau * f32_diff(p1, f(t0))
        fig["t_ulp"] = float((np.abs(f(t1) - t) / ulp32(t)).max())
        if fig["t_ulp"] > 2.0:
            bad.append(f"target off by {fig['t_ulp']:.3g} ulp32")
    return bad, fig


def gs_trajectory_margins(case, mode, seed=None):
    """The oracle's OWN two steps (lr = GS_LR) on a case: [{group: margin} per step]."""
    hyper, nets, data, idx = gs_inputs(case, seed)
    o = gs_oracle_at(hyper, nets + (nets[0],), mode, 0)
    out = []
    for t in range(GS_STEPS):
        o.train(orc.gather_batch(data, idx[t]), gs_keep_masks(hyper, t))
        out.append(dict(o.last_margin))
    return out


GS_SEED = 7  # the trainers' Philox key (dropout masks)


def gs_keep_masks(hyper, t):
    """The Philox keep masks of step t (0-based) as the device draws them, or None without dropout."""
    if not hyper["dropout"]:
        return None
    from oracle import philox
    B = hyper["batch"]  # (a Philox block covers 4 rows of one unit whatever the batch: whole blocks, then the real rows)
    return [philox.dropout_keep(GS_SEED, t, philox.dropout_stream(l), _round_up(B, 4), hyper["hidden"], hyper["dropout"])[:B]
            for l in range(hyper["n_hidden"])]


class gs_chunked_sums:
    """Inside the block the oracle forms every matrix product in fp32 over ``chunk`` terms at a time, the partial
    products added in order: the shape of an MFMA accumulation chain -- a third correct restatement of the step."""

    def __init__(self, chunk):
        self.chunk = chunk

    def _mm(self, a, b, acc):
        (M, K), N, c = a.shape, b.shape[1], self.chunk
        nk = -(-K // c)
        a3, b3 = np.zeros((M, nk * c), np.float32), np.zeros((nk * c, N), np.float32)  # (zero padding adds exact zeros)
        a3[:, :K], b3[:K] = a, b
        parts = a3.reshape(M, nk, c).transpose(1, 0, 2) @ b3.reshape(nk, c, N)  # [nk, M, N]: the chunks' products
        out = parts[0]
        for k in range(1, nk):
            out = out + parts[k]
        return out

    def __enter__(self):
        self.real, orc._mm = orc._mm, self._mm

    def __exit__(self, *exc):
        orc._mm = self.real


def gs_restatements_disagree(case, seed=None, chunks=(8, 32)):
    """In bf16 a rounding tie that falls the other way under another summation order moves a pre-activation by an
    ulp of ITS size, which in a deep, wide net flips relu' of units far further from zero than GS_MARGIN.  So the
    reference is asked to agree with itself first: along the oracle's own two steps, the oracle with chunked fp32
    sums (gs_chunked_sums; no GPU in it) is judged against the reference exactly as the GPU is.  Returns the
    tensors beyond the bounds -- a seed where correct restatements already differ by more cannot tell a wrong
    kernel from a right one."""
    hyper, nets, data, idx = gs_inputs(case, seed)
    o, bad = gs_oracle_at(hyper, nets + (nets[0],), "bf16", 0), []
    for t in range(GS_STEPS):
        state = tuple({k: v.copy() for k, v in d.items()} for d in (o.qf, o.vf, o.actor, o.q_target))
        batch, keeps = orc.gather_batch(data, idx[t]), gs_keep_masks(hyper, t)
        ref = gs_reference_step(hyper, state, "bf16", batch, t, keeps)
        for chunk in chunks:
            third = gs_oracle_at(hyper, state, "bf16", t)
            with gs_chunked_sums(chunk):
                third.train(batch, keeps)
            bad += [f"step {t + 1}, sums of {chunk}: {b}" for b in gs_judge_grads("bf16", third.last_grads, ref, hyper["batch"])[0]]
        o.train(batch, keeps)
    return bad


def gs_pick_seed(case, tries=64):
    """The first numpy seed at which the reference ALONE (a) keeps every net 2 x GS_MARGIN from a kink at both
    steps in both modes (twice the threshold: the GPU's parameters after step 1 differ from the oracle's by
    rounding) and (b) agrees with its own restatements in bf16 (gs_restatements_disagree).  GS_CASES records what
    this returns; cases at B >= 1024 cannot avoid a kink and keep seed 0 -- but for the offset cases of TS_CASES, whose
    biases keep most units on one side for the whole batch: those are searched like every other."""
    if gs_case(case)[4] >= 1024 and not (case in TS_CASES and TS_CASES[case][8]):
        return 0
    for seed in range(tries):
        if all(min(m.values()) >= 2 * GS_MARGIN for mode in ("fp32", "bf16") for m in gs_trajectory_margins(case, mode, seed)) \
                and not gs_restatements_disagree(case, seed):
            return seed
    raise AssertionError(f"{case}: no seed below {tries} keeps the reference away from the kinks")


# ---------------------------------------------------------------------------------------------
# Envelope tests of the tuned three-kernel step (csrc/iql_step.hip: n_hidden 2, hidden_dim 64 / 128 / 256;
# tests/test_gpu_tuned_step_envelope.py and, on the host, tests/test_tuned_step_envelope_host.py): the inputs,
# references and judges are the gs_* ones above, the cases and the launch plan are restated here.
# ---------------------------------------------------------------------------------------------
TS_CUS = 256            # compute units of an MI355X: what launch_update compares a lone seed's item table with
TS_UPDATE_LDS = 4608    # update_lds_floats(): 2 x max(64 x 36, 16 x 132) floats


def ts_update_slots(H, B, E, dropout):
    """Slots of a lone trainer's k_update item table, idle ones included (tuned_create, deal_items and flatten_table
    of csrc/api.hip restated).  A trained net has (H/64)(H/32) layer-2 tiles, H/16 layer-1 strips and
    ceil(out_pad/64)(H/32) layer-3 tiles; TwinQ puts net n on XCDs 2n and 2n + 1 (the lower half of every layer, by
    out-feature, on the first; layer-3 tiles alternate), more critics are dealt out in order, an eighth of all
    items per XCD.  The table is 8 x the longest column, grown by whole rows until it has an idle slot per 16 batch
    rows (32 slots for a trainer with dropout: they draw the next step's masks)."""
    rows16, NT = _round_up(B, 16) // 16, E + 2
    l2 = [o0 < H // 2 for o0 in range(0, H, 64) for _ in range(0, H, 32)]
    l1 = [o0 < H // 2 for o0 in range(0, H, 16)]
    l3 = [(i0 // 32) % 2 == 0 for _ in range(0, 16, 64) for i0 in range(0, H, 32)]  # (out_pad = 16 or 32: one row of tiles)
    per_net = len(l2) + len(l1) + len(l3)
    if NT == 4:
        low = sum(l2) + sum(l1) + sum(l3)
        cols = [low, per_net - low] * 4
    else:
        cols = [0] * 8
        for g in range(NT * per_net):
            cols[g * 8 // (NT * per_net)] += 1
    depth, n_real = max(cols), NT * per_net
    min_idle = 32 if dropout and rows16 < 32 else rows16
    while 8 * depth - n_real < min_idle:
        depth += 1
    return 8 * depth


def ts_tp_window(fwd_wgs, bwd_wgs):
    """(k_forward_tp, k_backward_tp) by use_tp's work-group counts alone: the throughput forward from 72 to 256
    work-groups, the throughput backward only beside it and from 144 to 256 of its own."""
    fwd_tp = 72 <= fwd_wgs <= 256
    return fwd_tp, fwd_tp and 144 <= bwd_wgs <= 256


def ts_plan(S, A, H, B, E, mode, dropout, n_seeds=1, cus=TS_CUS):
    """Which instantiation of each kernel a step takes, restated from the launchers of csrc/iql_step.hip
    (fwd_row_tiles, fwd_parts_per_wg, bwd_parts_per_wg, use_tp, launch_forward / _backward / _update) for a call
    without per-step valid-row counts, as one line of text:
      F<MT, PW, DROP> | Ftp<DROP>     k_forward: 16 x MT rows and PW layer-2 parts per work-group / k_forward_tp
      B<PRE, PW, NV> | Btp<nxn>       k_backward (NV: a padded batch) / k_backward_tp on nxn XCDs per trained net
      U<LAT, CNT>                     k_update: the 512-thread variant while a lone seed's table (ts_update_slots) has a
                                      CU per slot; CNT: bf16 on a padded batch
      k1 c/v                          layer-1 k-steps of the critics / of V and the actor (16 in-features in fp32, 32 in bf16)
      out n                           16-column output tiles of the actor
    B is the caller's batch size; the kernels work on B rounded up to 16 rows."""
    bf16, D_B = mode == "bf16", _round_up(B, 16)
    padded, rows = D_B != B, D_B * n_seeds
    parts = 4 if H >= 256 else H // 64
    fwd_wgs, bwd_wgs = (2 * E + 3) * (D_B // 64) * n_seeds, (E + 2) * (D_B // 32) * n_seeds
    fwd_tp, bwd_tp = ts_tp_window(fwd_wgs, bwd_wgs) if bf16 and H == 256 and D_B % 64 == 0 and not padded else (False, False)
    if fwd_tp:
        fwd = f"Ftp<{int(bool(dropout))}>"
    else:
        mt = 2 if rows >= 512 and D_B % 32 == 0 else 1
        pw = 2 if rows >= 1024 and parts % 2 == 0 else 1
        fwd = f"F<{mt},{pw},{int(bool(dropout))}>"
    if bwd_tp:
        bwd = f"Btp<{2 if E + 2 <= 4 and (D_B // 32) % 2 == 0 else 1}>"
    else:
        pw = 2 if rows >= 512 and parts % 2 == 0 else 1
        bwd = f"B<{int(pw == 1 and rows < 1024)},{pw},{int(padded)}>"
    lat = n_seeds == 1 and ts_update_slots(H, B, E, dropout) <= cus
    km = 32 if bf16 else 16
    return (f"{fwd} {bwd} U<{int(lat)},{int(bf16 and padded)}> k1 {_round_up(S + A, km) // km}/{_round_up(S, km) // km} "
            f"out {_round_up(A, 16) // 16}")


def ts_max_batch(A, E, deterministic):
    """The largest batch size check_cfg (csrc/api.hip) admits on the tuned step: the misc block of k_update sums the
    per-slab loss partials in its LDS, (round_up(B, 16) / 16) (E + 2 + (0 if deterministic else A)) + E + 2 floats
    of update_lds_floats()."""
    return (TS_UPDATE_LDS - (E + 2)) // (E + 2 + (0 if deterministic else A)) * 16


def _ts(fp32, bf16):
    return {"fp32": fp32, "bf16": bf16}


# id -> (S, A, 2, H, B, E, deterministic, dropout, offset biases, numpy seed, {mode: ts_plan's line}): GS_CASES'
# layout up to the seed (the first gs_pick_seed accepts; the offset cases at B >= 1024 are searched too), then what
# the case is meant to reach, checked against ts_plan before it is stepped.
TS_CASES = {
    # input and output widths at the edges of the header's envelope, one slab
    # one k-step that is almost all padding; a padded batch: NV, and CNT in bf16
    "s1a1_h64_b17": (1, 1, 2, 64, 17, 2, False, None, False, 1,
                     _ts("F<1,1,0> B<1,1,1> U<1,0> k1 1/1 out 1", "F<1,1,0> B<1,1,1> U<1,1> k1 1/1 out 1")),
    # exact tiles: no K padding for V / actor in fp32, one full output tile
    "s16a16_h64": (16, 16, 2, 64, 16, 2, False, None, False, 0,
                   _ts("F<1,1,0> B<1,1,0> U<1,0> k1 2/1 out 1", "F<1,1,0> B<1,1,0> U<1,0> k1 1/1 out 1")),
    # S + A = 128: every layer-1 k-step; odd S; one real column in the second output tile
    "s111a17_h64_e3": (111, 17, 2, 64, 16, 3, False, None, False, 5,
                       _ts("F<1,1,0> B<1,1,0> U<1,0> k1 8/7 out 2", "F<1,1,0> B<1,1,0> U<1,0> k1 4/4 out 2")),
    # S + A = 128 with A = 32, a full second output tile; two layer-2 parts
    "s96a32_h128_det": (96, 32, 2, 128, 16, 2, True, None, False, 6,
                        _ts("F<1,1,0> B<1,1,0> U<1,0> k1 8/6 out 2", "F<1,1,0> B<1,1,0> U<1,0> k1 4/3 out 2")),
    # OUTW = 2E + 2 + A = 50 output columns, ten trained nets
    "s20a32_h64_e8": (20, 32, 2, 64, 16, 8, False, None, False, 1,
                      _ts("F<1,1,0> B<1,1,0> U<1,0> k1 4/2 out 2", "F<1,1,0> B<1,1,0> U<1,0> k1 2/1 out 2")),
    # four layer-2 parts: one slab, and the bench shape's widths on two slabs
    "h256_b16": (17, 6, 2, 256, 16, 2, False, None, False, 1,
                 _ts("F<1,1,0> B<1,1,0> U<1,0> k1 2/2 out 1", "F<1,1,0> B<1,1,0> U<1,0> k1 1/1 out 1")),
    "h256_b32": (29, 8, 2, 256, 32, 2, False, None, False, 39,
                 _ts("F<1,1,0> B<1,1,0> U<1,0> k1 3/2 out 1", "F<1,1,0> B<1,1,0> U<1,0> k1 2/1 out 1")),
    # E = 8 at two parts (items dealt in order over the XCDs), and at four parts on a padded batch: 560 update items,
    # the 256-thread k_update for one seed, counted in bf16
    "h128_e8_det": (17, 6, 2, 128, 16, 8, True, None, False, 20,
                    _ts("F<1,1,0> B<1,1,0> U<1,0> k1 2/2 out 1", "F<1,1,0> B<1,1,0> U<1,0> k1 1/1 out 1")),
    "h256_e8_b40_off": (17, 6, 2, 256, 40, 8, False, None, True, 7,
                        _ts("F<1,1,0> B<1,1,1> U<0,0> k1 2/2 out 1", "F<1,1,0> B<1,1,1> U<0,1> k1 1/1 out 1")),
    # dropout: the masks plane on a padded batch, three bf16 k-steps; 32 idle slots that draw the next masks
    "h128_drop_b33": (45, 24, 2, 128, 33, 2, False, 0.25, False, 2,
                      _ts("F<1,1,1> B<1,1,1> U<1,0> k1 5/3 out 2", "F<1,1,1> B<1,1,1> U<1,1> k1 3/2 out 2")),
    "h256_drop_b16": (45, 24, 2, 256, 16, 2, False, 0.1, False, 16,
                      _ts("F<1,1,1> B<1,1,0> U<1,0> k1 5/3 out 2", "F<1,1,1> B<1,1,0> U<1,0> k1 3/2 out 2")),
    # 512 rows: 32-row forward work-groups; two parts per backward work-group from H = 128 on
    "h64_b512_off_det": (11, 3, 2, 64, 512, 2, True, None, True, 3,
                         _ts("F<2,1,0> B<1,1,0> U<1,0> k1 1/1 out 1", "F<2,1,0> B<1,1,0> U<1,0> k1 1/1 out 1")),
    "h128_b512_off": (17, 6, 2, 128, 512, 2, False, None, True, 0,
                      _ts("F<2,1,0> B<0,2,0> U<1,0> k1 2/2 out 1", "F<2,1,0> B<0,2,0> U<1,0> k1 1/1 out 1")),
    "h256_b512_off": (29, 8, 2, 256, 512, 2, False, None, True, 9,
                      _ts("F<2,1,0> B<0,2,0> U<1,0> k1 3/2 out 1", "F<2,1,0> B<0,2,0> U<1,0> k1 2/1 out 1")),
    # bf16: k_forward_tp (76 work-groups) beside k_backward, and (75) with dropout; both throughput kernels (152 / 160),
    # one XCD per net
    "h256_b256_e8_off": (17, 6, 2, 256, 256, 8, False, None, True, 2,
                         _ts("F<1,1,0> B<1,1,0> U<0,0> k1 2/2 out 1", "Ftp<0> B<1,1,0> U<0,0> k1 1/1 out 1")),
    "h256_b320_e6_off_drop": (17, 6, 2, 256, 320, 6, False, 0.1, True, 1,
                              _ts("F<1,1,1> B<1,1,0> U<0,0> k1 2/2 out 1", "Ftp<1> B<1,1,0> U<0,0> k1 1/1 out 1")),
    "h256_b512_e8_off": (17, 6, 2, 256, 512, 8, False, None, True, 35,
                         _ts("F<2,1,0> B<0,2,0> U<0,0> k1 2/2 out 1", "Ftp<0> Btp<1> U<0,0> k1 1/1 out 1")),
    # 1024 rows: two parts per forward work-group, the backward's operands behind its dZ2 phase; bf16: k_forward_tp
    # (112).  64 idle slots make the table 288 slots: the 256-thread k_update.  The same forward with dropout at H = 128
    "h256_b1024_off": (29, 8, 2, 256, 1024, 2, False, None, True, 6,
                       _ts("F<2,2,0> B<0,2,0> U<0,0> k1 3/2 out 1", "Ftp<0> B<0,2,0> U<0,0> k1 2/1 out 1")),
    "h128_b1024_off": (17, 6, 2, 128, 1024, 2, False, None, True, 1,
                       _ts("F<2,2,0> B<0,2,0> U<1,0> k1 2/2 out 1", "F<2,2,0> B<0,2,0> U<1,0> k1 1/1 out 1")),
    "h128_b1024_off_drop": (17, 6, 2, 128, 1024, 2, False, 0.1, True, 3,
                            _ts("F<2,2,1> B<0,2,0> U<1,0> k1 2/2 out 1", "F<2,2,1> B<0,2,0> U<1,0> k1 1/1 out 1")),
    # bf16: k_backward_tp on two XCDs per net (126 / 144 work-groups)
    "h256_b1152_off": (29, 8, 2, 256, 1152, 2, False, None, True, 3,
                       _ts("F<2,2,0> B<0,2,0> U<0,0> k1 3/2 out 1", "Ftp<0> Btp<2> U<0,0> k1 2/1 out 1")),
    # H = 64 never takes two parts: from 1024 rows on the backward's operands come behind the dZ2 phase (PRE false,
    # PW 1); the same on a padded batch with dropout
    "h64_b1024_off": (11, 3, 2, 64, 1024, 2, False, None, True, 0,
                      _ts("F<2,1,0> B<0,1,0> U<1,0> k1 1/1 out 1", "F<2,1,0> B<0,1,0> U<1,0> k1 1/1 out 1")),
    "h64_b1020_off_drop": (11, 3, 2, 64, 1020, 2, False, 0.1, True, 2,
                           _ts("F<2,1,1> B<0,1,1> U<1,0> k1 1/1 out 1", "F<2,1,1> B<0,1,1> U<1,1> k1 1/1 out 1")),
    # 1040 rows, no multiple of 32: 16-row forward work-groups with two parts; padded and with dropout
    "h128_b1040_off": (17, 6, 2, 128, 1040, 2, False, None, True, 1,
                       _ts("F<1,2,0> B<0,2,0> U<1,0> k1 2/2 out 1", "F<1,2,0> B<0,2,0> U<1,0> k1 1/1 out 1")),
    "h128_b1030_off_drop": (17, 6, 2, 128, 1030, 2, False, 0.1, True, 13,
                            _ts("F<1,2,1> B<0,2,1> U<1,0> k1 2/2 out 1", "F<1,2,1> B<0,2,1> U<1,1> k1 1/1 out 1")),
}
TS_DAMAGE_CASES = ("s111a17_h64_e3", "h256_b512_off")  # where the host test shows what the bounds reject


# ---- include/iqlhip.h as data: what tests/test_abi_host.py compares the ctypes binding with ----
class CType:
    """A C type as a declaration spells it, ``const`` dropped: ``base`` (a scalar, ``void``, ``char`` or a struct
    name), ``ptr`` levels of ``*`` and ``array``, the length of a ``[n]`` suffix or None."""

    def __init__(self, base, ptr=0, array=None):
        self.base, self.ptr, self.array = base, ptr, array

    def __repr__(self):
        return self.base + " " * bool(self.ptr) + "*" * self.ptr + (f"[{self.array}]" if self.array is not None else "")


def _c_int_expr(expr, macros):
    """An integer macro body: integers, earlier macros, + - * / and parentheses."""
    import re
    expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(macros[m.group(0)]), expr)
    assert re.fullmatch(r"[\d\s()+\-*/]+", expr), expr
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def _c_declarators(decl, macros):
    """A field or parameter declaration ``const float *a, *b[N]`` -> [("a", CType), ("b", CType)]; every
    declarator carries a name (the header names all its parameters)."""
    import re
    first, *more = [d.strip() for d in decl.split(",")]
    words = re.findall(r"[A-Za-z_]\w*", re.sub(r"\[.*?\]", "", first))
    words = [w for w in words if w != "const"]
    base, out = " ".join(words[:-1]), []
    for d in [first] + more:
        m = re.fullmatch(r"(.*?)([A-Za-z_]\w*)\s*(?:\[(.*?)\])?", d, re.S)
        assert m, d
        out.append((m.group(2), CType(base, m.group(1).count("*"),
                                      _c_int_expr(m.group(3), macros) if m.group(3) is not None else None)))
    return out


def parse_c_header(text):
    """The declarations of a C header in the plain style of include/iqlhip.h (no function pointers, no nested
    structs, no bit fields): {"macros": {name: int}, "enums": {name: int}, "structs": {name: [(field, CType)]},
    "opaque": {names of ``typedef struct x x;``}, "functions": {name: (CType, [(param, CType)])}}."""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    macros = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M):
        macros[name] = _c_int_expr(body, macros)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    enums = {}
    for body in re.findall(r"typedef\s+enum\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.S):
        for name, value in re.findall(r"(\w+)\s*=\s*([^,}]+)", body):
            enums[name] = _c_int_expr(value, macros)
    text = re.sub(r"typedef\s+enum\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        assert "{" not in body, name
        structs[name] = [f for decl in body.split(";") if decl.strip() for f in _c_declarators(decl.strip(), macros)]
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    opaque = set()
    for tag, name in re.findall(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", text):
        assert tag == name, (tag, name)
        opaque.add(name)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)
    functions = {}
    for stmt in text.split(";"):
        stmt = stmt.strip().lstrip("}").strip()  # (the brace that closes extern "C")
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, re.S)
        assert m and "(" not in m.group(3), "not a prototype: " + stmt
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        words = [w for w in re.findall(r"[A-Za-z_]\w*", ret) if w != "const"]
        assert name not in functions, name
        functions[name] = (CType(" ".join(words), ret.count("*")),
                           [] if params == "void" else [_c_declarators(p, macros)[0] for p in params.split(",")])
    return {"macros": macros, "enums": enums, "structs": structs, "opaque": opaque, "functions": functions}
