"""oracle/relabel_oracle.py pinned against tests/golden/dataset_ops.npz (captured
from the reference's own functions).  CPU only."""
import numpy as np
import pytest

from oracle import relabel_oracle as ro
from tests import helpers


@pytest.fixture(scope="module")
def g():
    return np.load(helpers.GOLDEN + "/dataset_ops.npz")


def g5_dataset(g, use_timeouts=True):
    ds = {k.split("/")[-1]: g[k] for k in g.files if k.startswith("g5/ds/")}
    ds["terminals"] = ds["terminals"].astype(bool)
    ds["timeouts"] = ds["timeouts"].astype(bool)
    if not use_timeouts:
        ds.pop("timeouts")
    return ds


def mlp_weights(g, prefix):
    """[W0,b0,W1,b1,...,Wout,bout] from the stand-in state-dict names."""
    keys = [k[len(prefix):] for k in g.files if k.startswith(prefix)]
    hidden = sorted({k.split(".")[1] for k in keys if k.startswith("layers.")},
                    key=lambda s: 0 if s == "0" else int(s.split("_")[1]))
    out = []
    for h in hidden:
        out += [g[f"{prefix}layers.{h}.W"], g[f"{prefix}layers.{h}.b"]]
    out += [g[prefix + "out.W"], g[prefix + "out.b"]]
    return out


def test_reward_range_and_modify_reward(g):
    rew, term = g["g4/rewards"], g["g4/terminals"]
    mn, mx, tl = ro.return_reward_range(rew, term, 12)
    np.testing.assert_allclose([mn, mx], g["g4/range"], rtol=1e-12)
    np.testing.assert_array_equal(tl, g["g4/trj_lens"])
    for nr in range(1, 9):
        np.testing.assert_allclose(ro.modify_reward(rew, term, "antmaze-medium-diverse-v2", nr, 12),
                                   g[f"g4/antmaze_nr{nr}"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ro.modify_reward(rew, term, "halfcheetah-medium-v2", 1, 12),
                               g["g4/halfcheetah"], rtol=1e-6)
    np.testing.assert_array_equal(ro.modify_reward(rew, term, "pen-human-v1", 1, 12), g["g4/pen_untouched"])


def test_cvar(g):
    preds = g["cvar/preds"]
    for alpha in (0.0, 0.5, 0.9, 0.95):
        np.testing.assert_allclose(ro.cvar_tail_mean(preds, alpha), g[f"cvar/vec_alpha{alpha}"], rtol=1e-6)
        emp = [ro.empirical_cvar(preds[:, i], alpha) for i in range(preds.shape[1])]
        np.testing.assert_allclose(emp, g[f"cvar/emp_alpha{alpha}"], rtol=1e-6)
        np.testing.assert_allclose(ro.cvar_stability_check(preds, alpha, 20), g[f"cvar/stab_alpha{alpha}"],
                                   rtol=1e-6)
    assert ro.empirical_cvar(preds[:1, 0], 0.9) == pytest.approx(float(g["cvar/single"]))
    with pytest.raises(ValueError):
        ro.empirical_cvar(preds[:, 0], 1.0)


@pytest.mark.parametrize("use_to", [True, False])
@pytest.mark.parametrize("toe", [False, True])
def test_mr_relabel(g, use_to, toe):
    ds = g5_dataset(g, use_to)
    out = ro.qlearning_dataset_mr(ds, mlp_weights(g, "g5/rm/"), 15, terminate_on_end=toe)
    tag = f"g5/mr/timeouts{int(use_to)}_toe{int(toe)}"
    for k, v in out.items():
        want = g[f"{tag}/{k}"]
        assert v.shape == want.shape, k
        np.testing.assert_allclose(np.asarray(v, dtype=np.float32), want, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("ql", [5, 20])
def test_pt_windows_bug_compatible(g, ql):
    ds = g5_dataset(g)
    keep, ep_steps = ro.keep_mask_and_steps(ds["terminals"], ds["timeouts"], 15)
    sts, acts, ts, am = ro.pt_windows(ds["observations"], ds["actions"], ep_steps, ql)
    tag = f"g5/pt/ql{ql}"
    np.testing.assert_array_equal(sts, g[f"{tag}/win_states"])
    np.testing.assert_array_equal(acts, g[f"{tag}/win_actions"])
    np.testing.assert_array_equal(ts, g[f"{tag}/win_timesteps"])
    np.testing.assert_array_equal(am, g[f"{tag}/win_mask"])
    # the kept rows of the relabelled dataset
    np.testing.assert_array_equal(ds["observations"][:-1][keep], g[f"{tag}/observations"])
    np.testing.assert_array_equal(ds["terminals"][:-1][keep].astype(np.float32), g[f"{tag}/terminals"])
    # rewards of the recording fake model (see tests/golden/make_fixtures.py Recorder)
    w = np.arange(1, ql + 1, dtype=np.float32)
    val = ((sts.sum(-1) + 2.0 * acts.sum(-1) + 0.01 * ts.astype(np.float32)) * am * w).cumsum(1)[:, -1]
    np.testing.assert_allclose(val[keep], g[f"{tag}/rewards"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("alpha,burn", [(0.0, 0), (0.5, 1), (0.9, 2)])
def test_mr_ensemble(g, alpha, burn):
    ds = g5_dataset(g)
    sets = [mlp_weights(g, f"g5/ens/snap{i}/") for i in range(burn, 6)]
    out, _ = ro.qlearning_dataset_ensemble(ds, sets, alpha, 15)
    tag = f"g5/ens/alpha{alpha}_burn{burn}"
    for k, v in out.items():
        np.testing.assert_allclose(np.asarray(v, dtype=np.float32), g[f"{tag}/{k}"], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("alpha,ns", [(0.5, 500), (0.75, 5), (0.0, 0)])
def test_bnn(g, alpha, ns):
    ds = g5_dataset(g)
    all_w = [[g[f"g5/bnn/w{i}/{j}"] for j in range(6)] for i in range(8)]
    if 0 < ns < len(all_w):  # ref:929-932 subsample with default_rng(0)
        idx = np.random.default_rng(seed=0).choice(len(all_w), size=ns, replace=False)
        all_w = [all_w[i] for i in sorted(idx)]
    out, _ = ro.qlearning_dataset_ensemble(ds, all_w, alpha, 15)
    tag = f"g5/bnn/alpha{alpha}_n{ns}"
    for k, v in out.items():
        np.testing.assert_allclose(np.asarray(v, dtype=np.float32), g[f"{tag}/{k}"], rtol=2e-6, atol=2e-6)


def test_pt_forward_self_consistency():
    """Parity unpinned (no runnable reference): structural checks of the restatement."""
    rng = np.random.default_rng(0)
    S, A, QL = 5, 3, 6
    p = ro.make_pt_params(rng, S, A, 20, embd=16, pref=8, inter=32, layers=2)
    st = rng.standard_normal((4, QL, S)).astype(np.float32)
    ac = rng.standard_normal((4, QL, A)).astype(np.float32)
    ts = np.tile(np.arange(QL), (4, 1))
    am = np.ones((4, QL), np.float32)
    v = ro.pt_value_last(p, st, ac, ts, am, num_heads=4)
    assert v.shape == (4,) and np.isfinite(v).all()
    # left padding with mask 0 == the shorter unpadded window with the same timesteps
    st2 = np.zeros((4, QL + 3, S), np.float32); st2[:, 3:] = st
    ac2 = np.zeros((4, QL + 3, A), np.float32); ac2[:, 3:] = ac
    ts2 = np.zeros((4, QL + 3), np.int64); ts2[:, 3:] = ts
    am2 = np.zeros((4, QL + 3), np.float32); am2[:, 3:] = 1
    v2 = ro.pt_value_last(p, st2, ac2, ts2, am2, num_heads=4)
    np.testing.assert_allclose(v2, v, rtol=1e-5, atol=1e-5)


# ---- the generators and references of the GPU envelope tests (tests/helpers.py): what those tests
# ---- rely on is checked here, on the host
CVAR_S = (2, 3, 32, 33, 64, 65, 67, 128, 129, 131, 256, 257, 1248, 1249, 1251, 2399, 2400)


def test_cvar_launch_configurations_and_tail_sizes():
    cfg = {S: helpers.cvar_launch_config(S) for S in CVAR_S}
    assert [cfg[S] for S in (32, 33, 64, 65, 128, 129, 256, 257, 1248, 1249, 2400)] == \
        [(128, 2), (64, 4), (64, 4), (32, 8), (32, 8), (32, 16), (32, 16), (32, 32), (32, 32), (16, 32), (16, 32)]
    for S in CVAR_S:
        tails = helpers.cvar_n_tails(S)
        assert tails[0] == 1 and tails[-1] == S and all(1 <= t <= S for t in tails) and len(set(tails)) == len(tails)
        assert all(ro.n_tail_of(a, S) in tails for a in (0.5, 0.9, 0.95))
        if S >= 32:
            assert {8, 9, S // 2, S - 1} <= set(tails)


@pytest.mark.parametrize("S", CVAR_S)
def test_cvar_column_families_have_their_stated_properties(S):
    rng = np.random.default_rng(S)
    for n_tail in helpers.cvar_n_tails(S):
        N = 2 * len(helpers.CVAR_FAMILIES) + 1
        preds, names = helpers.cvar_matrix(rng, S, N, n_tail, first=n_tail)
        assert preds.dtype == np.float32 and preds.shape == (S, N) and np.isfinite(preds).all()
        assert set(names) == set(helpers.CVAR_FAMILIES)  # round-robin: every family in every matrix
        want, tol = helpers.cvar_ref(preds, n_tail)
        assert np.isfinite(want).all() and np.isfinite(tol).all() and np.abs(want).max() * n_tail < 3e38
        kth = min(n_tail, S - 1)  # the reference's own route (ref:1009-1011), in fp64
        np.testing.assert_allclose(want, np.partition(preds.astype(np.float64), kth, axis=0)[:n_tail].mean(axis=0),
                                   rtol=1e-12, atol=0)
        for c, name in enumerate(names):
            col = preds[:, c]
            srt = np.sort(col)
            if name == "constant":
                assert np.unique(col).size == 1
            elif name in ("two_half", "two_tail"):
                k = S // 2 if name == "two_half" else n_tail
                assert (col == col.min()).sum() == (k if 0 < k < S else S) and np.unique(col).size == (2 if 0 < k < S else 1)
                if 0 < k < S:
                    assert srt[k - 1] < srt[k]  # the split sits at rank k exactly
            elif name == "ulps":
                if S >= 32:  # (fewer rows cannot hold one value nine times)
                    assert (col == srt[n_tail - 1]).sum() > 8
                assert np.unique(col).size <= 16 and col.min() >= 1 and col.max() <= 1 + 15 * 2.0 ** -23
            elif name in ("wide", "negative") and S >= 32:
                mag = np.abs(col[col != 0].astype(np.float64))
                assert np.log10(mag.max() / mag.min()) > 20
                assert (col < 0).all() if name == "negative" else ((col < 0).any() and (col > 0).any())
            elif name == "zeros_denormals" and S < 32:
                assert col.min() <= -1e-30
            elif name == "zeros_denormals":
                assert col.min() <= -1e-30 and np.abs(col).max() < 1e-28
                tiny = np.finfo(np.float32).tiny
                assert ((col == 0) & ~np.signbit(col)).any() and ((col == 0) & np.signbit(col)).any()
                assert ((col != 0) & (np.abs(col) < tiny)).any()
            elif name == "ties":
                assert S < 32 or np.unique(col).size < S
            elif name == "ascending":
                assert np.array_equal(col, srt)
            elif name == "descending":
                assert np.array_equal(col[::-1], srt)


def test_cvar_integer_matrix_sums_exactly():
    m = helpers.cvar_int_matrix(np.random.default_rng(0), 2400, 35)
    assert np.array_equal(m, np.round(m)) and np.abs(m).max() <= 1000 and np.abs(m).sum(axis=0).max() < 1 << 24


def test_mlp_reference_reproduces_the_relabel_oracle():
    rng = np.random.default_rng(3)
    for dims, act, code in (([37, 256, 256, 1], "relu", 0), ([13, 100, 7], "relu", 0), ([6, 8, 8, 3], "tanh", 1)):
        ws, bs = helpers.mlp_weights_for(rng, dims)
        x = rng.standard_normal((50, dims[0])).astype(np.float32)
        want = ro.reward_mlp_forward([a for pair in zip(ws, bs) for a in pair], x, act)
        np.testing.assert_allclose(helpers.mlp_forward_ref(ws, bs, x, code, 0), want, rtol=0, atol=1e-6)
        np.testing.assert_allclose(helpers.mlp_forward_ref(ws, bs, x, code, 0, dtype=np.float32), want, rtol=0, atol=1e-6)
    # the table codes: the functions test_qmlp_activations_match_numpy names, in table order
    v = np.linspace(-3, 3, 13)
    for i, name in enumerate(helpers.FLAX_ACTIVATIONS):
        for hidden in (True, False):
            assert np.array_equal(helpers.mlp_act(8 + i, hidden)(v), helpers.FLAX_ACTIVATIONS[name](v))
    assert list(helpers.FLAX_ACTIVATIONS) == ["cos", "tanh", "relu", "softplus", "sin", "leaky_relu", "swish", "none"]
    assert np.array_equal(helpers.mlp_act(0, True)(v), np.maximum(v, 0)) and np.array_equal(helpers.mlp_act(0, False)(v), v)
    assert np.array_equal(helpers.mlp_act(1, True)(v), np.tanh(v)) and np.array_equal(helpers.mlp_act(1, False)(v), np.tanh(v))
    # dropout masks enter as given
    keep = [rng.uniform(size=(50, 8)) < 0.5] * 2
    ws, bs = helpers.mlp_weights_for(rng, [6, 8, 8, 3])
    x = rng.standard_normal((50, 6)).astype(np.float32)
    h = np.maximum(x.astype(np.float64) @ ws[0] + bs[0], 0) * keep[0] * 2.0
    h = np.maximum(h @ ws[1] + bs[1], 0) * keep[1] * 2.0
    np.testing.assert_allclose(helpers.mlp_forward_ref(ws, bs, x, 0, 0, keeps=keep, scale=2.0), h @ ws[2] + bs[2], atol=1e-12)


# ---- the preference-transformer envelope cases (tests/helpers.py, tests/test_gpu_pt_envelope.py): the
# ---- float64 mode of pt_value_last is the yardstick there.  Here: the float32 restatement and the
# ---- float64 one agree inside the bounds those tests apply, so a kernel that misses them is wrong
def test_pt_float64_mode_keeps_the_bf16_rounding_points():
    rng = np.random.default_rng(2)
    S, A, QL = 5, 3, 6
    p = ro.make_pt_params(rng, S, A, 20, embd=16, pref=8, inter=32, layers=2)
    st = rng.standard_normal((4, QL, S)).astype(np.float32)
    ac = rng.standard_normal((4, QL, A)).astype(np.float32)
    ts, am = np.tile(np.arange(QL), (4, 1)), np.ones((4, QL), np.float32)
    v32 = ro.pt_value_last(p, st, ac, ts, am, num_heads=4)
    assert v32.dtype == np.float32
    np.testing.assert_array_equal(v32, ro.pt_value_last(p, st, ac, ts, am, num_heads=4, dtype=np.float32))
    v64 = ro.pt_value_last(p, st, ac, ts, am, num_heads=4, dtype=np.float64)
    assert v64.dtype == np.float64 and not np.array_equal(v64, v32.astype(np.float64))
    np.testing.assert_allclose(v32, v64, rtol=0, atol=1e-5)
    # one rounding from float64, ties to even, 8 significant bits
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.14159, 0.0, 1e-3])
    r = ro._bf16_as(x, np.float64)
    np.testing.assert_array_equal(r[:3], [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7])
    np.testing.assert_array_equal(r, ro._bf16_as(r, np.float64))
    np.testing.assert_array_equal(r.astype(np.float32), ro.bf16(r.astype(np.float32)))
    assert np.all(np.abs(r - x) <= helpers.bf16_ulp(x) / 2)


def test_pt_oracle_windows_trimmed_to_their_batch():
    """The long cases pad a batch to its longest window, not to query_length: the same value."""
    case = (2, 64, 4, 64, 5, 3, 17)
    p, obs, act, lens, starts, t0, _ = helpers.pt_case_inputs(case)
    full = helpers.oracle_windows(p, obs, act, starts, lens, t0, 17, 4, dtype=np.float64)
    np.testing.assert_allclose(helpers.oracle_windows(p, obs, act, starts, lens, t0, 17, 4, dtype=np.float64, trim=True),
                               full, rtol=0, atol=1e-12)
    np.testing.assert_allclose(helpers.oracle_windows(p, obs, act, starts, lens, t0, 40, 4, dtype=np.float64),
                               full, rtol=0, atol=1e-12)
    # and a prefix of one longer forward is the window of that length
    pre = helpers.oracle_prefixes(p, obs, act, 7, 17, 3, 4, dtype=np.float64)
    ln = np.arange(1, 18, dtype=np.int32)
    np.testing.assert_allclose(pre, helpers.oracle_windows(p, obs, act, np.full(17, 7), ln, np.full(17, 3), 17, 4,
                                                           dtype=np.float64), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", helpers.PT_TUNED_CASES + helpers.PT_GENERAL_CASES, ids=helpers.pt_case_id)
def test_pt_envelope_case_float32_vs_float64(case):
    """Worst over the cases and both timestep modes: max |d| 6.7e-4 (the widest tuned shape, win_t0 None),
    median <= 5.6e-7.  Every case passes with its own shape as the seed (helpers.PT_CASE_SEEDS is empty)."""
    L, E, heads, I, S, A, QL = case
    p, obs, act, lens, starts, t0, _ = helpers.pt_case_inputs(case)
    assert lens.min() == 1 and lens.max() == QL and len(lens) <= 161
    assert (starts >= 0).all() and (starts + lens <= len(obs)).all() and (t0 + lens <= len(p["timestep_embed.weight"])).all()
    trim = QL > 64
    for tt in (t0,) if trim else (t0, None):  # (the long cases once: their forwards take seconds)
        f32 = helpers.oracle_windows(p, obs, act, starts, lens, tt, QL, heads, trim=trim)
        f64 = helpers.oracle_windows(p, obs, act, starts, lens, tt, QL, heads, dtype=np.float64, trim=trim)
        mx, med = helpers.check_close(f32, f64, short=lens <= 8)
        print(f"{helpers.pt_case_id(case)}: float32 vs float64 max |d| {mx:.3g}, median {med:.3g}")


@pytest.mark.parametrize("case,n", [(helpers.PT_GENERAL_LONG, 1024), (helpers.PT_GENERAL_TOP, 4096)],
                         ids=["long", "top"])
def test_pt_envelope_long_case_float32_vs_float64(case, n):
    """Every prefix of the one forward.  QL 1024: max |d| 2.1e-4, median 8.6e-7; QL 4096: 1.1e-3 /
    7.9e-7 (the float64 forward over 4096 transitions: 9.5 s on one core of the development host)."""
    heads = case[2]
    p, obs, act, start, t0, lens, _ = helpers.pt_prefix_inputs(case, n, [1, 2, n // 2, n - 1, n], 0)
    f32 = helpers.oracle_prefixes(p, obs, act, start, n, t0, heads)
    f64 = helpers.oracle_prefixes(p, obs, act, start, n, t0, heads, dtype=np.float64)
    mx, med = helpers.check_close(f32, f64, short=np.arange(1, n + 1) <= 8)
    print(f"{helpers.pt_case_id(case)} ({n}): float32 vs float64 max |d| {mx:.3g}, median {med:.3g}")


def test_pt_clamp_rule_passes_valid_windows_through():
    rng = np.random.default_rng(0)
    lens, starts, t0 = helpers.random_windows(rng, 60, 40, 8, 16)
    s2, l2, t2 = helpers.pt_clamp_windows(starts, lens, t0, 60, 41, 8)
    assert np.array_equal(s2, starts) and np.array_equal(l2, lens) and np.array_equal(t2, t0)
    s2, l2, t2 = helpers.pt_clamp_windows([-4, 58, 160, 5, 5, 5, 5, 5], [5, 5, 3, 0, -3, 13, 4, 3],
                                          [0, 0, 0, 0, 0, 0, -1, 40], 60, 41, 8)
    assert s2.tolist() == [0, 55, 57, 5, 5, 5, 5, 5] and l2.tolist() == [5, 5, 3, 1, 1, 8, 4, 3]
    assert t2.tolist() == [0, 0, 0, 0, 0, 0, 0, 38]
    assert [a.tolist() for a in helpers.pt_clamp_windows([0], [8], [2], 3, 41, 8)] == [[0], [3], [2]]
