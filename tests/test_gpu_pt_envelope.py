"""GPU: both preference-transformer relabel paths -- the tuned one-block kernel k_pt_relabel
(csrc/pt.hip) and the layer-wise general path (csrc/pt_general.hip) -- over the whole envelope that
include/iqlhip.h states for them.  -m gpu.

PT numerics are PARITY UNPINNED (no runnable reference: JAX is absent).  The yardstick here is the
float64 mode of the numpy restatement (oracle/relabel_oracle.py:pt_value_last, dtype=np.float64:
every sum in float64, the three bf16 rounding points of ops.py:74-79 where they are);
tests/test_relabel_oracle.py shows on the host that the float32 restatement of every case below
stays inside the same two bounds, so a kernel that misses them is wrong.  The bounds are those of
test_gpu_pt_general.py: 5e-3 everywhere (a bf16 flip of a q.k logit), a median of 1e-5 on the
windows of length <= 8 (a wrong tile, chunk or head split errs by the size of the values).

Every case reads obs / act as the interior rows of larger device tensors whose other rows are NaN:
a read one row outside the arrays shows up as NaN instead of as a plausible number."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import helpers
from tests.helpers import check_close, oracle_prefixes, oracle_windows, pt_case_id
from tests.test_gpu_pt_general import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3  # NaN rows on either side of the dataset rows


def dv(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def guarded(x):
    """x on the device as rows GUARD .. GUARD + n of a tensor whose other rows are NaN.  A row slice
    of a contiguous tensor is contiguous: window_values takes it as it is, without a copy."""
    big = np.full((x.shape[0] + 2 * GUARD,) + x.shape[1:], np.nan, np.float32)
    big[GUARD:GUARD + x.shape[0]] = x
    whole = dv(big)
    view = whole[GUARD:GUARD + x.shape[0]]
    assert view.is_contiguous() and view.data_ptr() == whole.data_ptr() + GUARD * x.shape[1] * 4
    assert view.contiguous().data_ptr() == view.data_ptr() and bool(torch.isnan(whole[GUARD - 1]).all())
    return view


def run_case(case, kernel):
    """The windows of helpers.pt_case_inputs with win_t0 given and with None, against the float64
    oracle."""
    L, E, heads, I, S, A, QL = case
    p, obs, act, lens, starts, t0, max_ep = helpers.pt_case_inputs(case)
    m = make_model(p, S, A, max_ep, heads, max_pos=max(64, 2 * QL))
    assert m.tuned_shape() == (kernel == "tuned")
    o, a = guarded(obs), guarded(act)
    for tt in (t0, None):
        got = m.window_values(o, a, dv(starts), dv(lens), QL, win_t0=None if tt is None else dv(tt),
                              kernel=kernel).cpu().numpy()
        want = oracle_windows(p, obs, act, starts, lens, tt, QL, heads, dtype=np.float64, trim=QL > 64)
        d = np.abs(got - want)
        print(f"{kernel} {pt_case_id(case)} win_t0 {'given' if tt is not None else 'None'}: {len(lens)} windows, "
              f"max |d| {d.max():.3g}, median {np.median(d):.3g}, median of len <= 8 {np.median(d[lens <= 8]):.3g}")
        check_close(got, want, short=lens <= 8)


@pytest.mark.parametrize("case", helpers.PT_TUNED_CASES, ids=pt_case_id)
def test_tuned_kernel_over_its_envelope(case):
    """k_pt_relabel at the corners of its envelope (helpers.PT_TUNED_CASES says what each reaches): the
    second and later KCH chunks of embed_ln, whole and partial; inter_dim 768 and 1024; the launch with
    one work-group per CU (LDS > 80 KiB); three and more job rounds per window.
    Observed on an MI355X, max / median |d| vs the float64 oracle, win_t0 given | None:
    S1 A1 QL1 8.1e-07 / 1.6e-07 | 3.9e-07 / 1.4e-07
    S49 A3 3.7e-07 / 1.0e-07 | 5.2e-07 / 1.1e-07
    S3 A49 3.8e-04 / 1.7e-07 | 7.3e-07 / 2.2e-07
    S96 A96 I1024 1.1e-04 / 1.8e-07 | 1.9e-03 / 2.2e-07
    S191 A1 I768 5.0e-07 / 1.2e-07 | 6.3e-07 / 1.3e-07
    h16 I1024 7.2e-07 / 1.6e-07 | 5.0e-07 / 1.6e-07
    QL129 5.6e-05 / 1.4e-07 | 1.1e-04 / 1.5e-07
    QL300 4.3e-05 / 1.5e-07 | 4.4e-05 / 1.2e-07"""
    run_case(case, "tuned")


@pytest.mark.parametrize("case", helpers.PT_GENERAL_CASES, ids=pt_case_id)
def test_general_path_over_its_envelope(case):
    """k_attn at every (HDL, DPL, G) family the envelope allows -- head_dim 256, 128, 192, 96, 48, 12,
    6, 8 and 4, up to 64 heads --, S + A = 256 with the split at either end and in the middle, and the
    edges of the 32-row token tile (query_length 1, 16, 17).
    Observed on an MI355X, max / median |d| vs the float64 oracle, win_t0 given | None, in the order of
    helpers.PT_GENERAL_CASES:
    E256 h1 I64 S5 A3 QL9: 3.6e-05 / 3.0e-07 | 6.3e-04 / 2.1e-07
    E128 h1 I128 S5 A3 QL9: 7.2e-05 / 2.0e-07 | 6.3e-06 / 1.9e-07
    E256 h2 I256 S5 A3 QL9: 1.7e-04 / 3.3e-07 | 9.0e-05 / 3.4e-07
    E192 h1 I192 S5 A3 QL9: 1.3e-04 / 2.4e-07 | 2.8e-04 / 3.0e-07
    E192 h2 I192 S5 A3 QL9: 1.8e-04 / 3.0e-07 | 9.5e-05 / 2.3e-07
    E192 h4 I192 S5 A3 QL9: 1.3e-04 / 3.3e-07 | 1.0e-04 / 2.3e-07
    E192 h16 I192 S5 A3 QL9: 4.4e-05 / 3.7e-07 | 2.3e-05 / 1.6e-07
    E192 h32 I192 S5 A3 QL9: 5.0e-05 / 2.4e-07 | 4.5e-05 / 2.5e-07
    E64 h8 I64 S5 A3 QL9: 3.4e-04 / 1.7e-07 | 4.1e-07 / 1.4e-07
    E128 h32 I128 S5 A3 QL9: 6.4e-05 / 2.4e-07 | 2.9e-05 / 3.3e-07
    E256 h64 I1024 S5 A3 QL9: 9.9e-05 / 3.7e-07 | 2.8e-04 / 6.6e-07
    E64 h4 I64 S255 A1 QL6: 7.0e-07 / 1.6e-07 | 2.1e-05 / 2.2e-07
    E64 h4 I64 S1 A255 QL6: 1.5e-06 / 2.3e-07 | 2.9e-04 / 1.6e-07
    E128 h4 I256 S128 A128 QL6: 5.4e-06 / 1.7e-07 | 6.8e-07 / 1.7e-07
    E64 h4 I64 S5 A3 QL1: 2.8e-05 / 1.5e-07 | 5.1e-07 / 1.7e-07
    E64 h4 I64 S5 A3 QL16: 1.4e-04 / 1.2e-07 | 3.6e-05 / 1.4e-07
    E64 h4 I64 S5 A3 QL17: 1.8e-05 / 1.8e-07 | 1.2e-04 / 1.8e-07"""
    run_case(case, "general")


def test_tuned_widest_shape_many_windows_per_workgroup():
    """S + A = 192 with inter_dim 1024 takes more than 80 KiB of LDS: one work-group per CU, so the
    grid and the queue stride are the CU count.  Nine or ten windows per work-group (a full batch of 8
    parked tails and a partial one): every value equals, bit for bit, what the window gets in calls of
    at most 64 windows (one per work-group), and 24 of them the float64 oracle."""
    case = helpers.PT_TUNED_WIDEST
    L, E, heads, I, S, A, QL = case
    rng = np.random.default_rng(list(case) + [1])  # (the case's own seed made its weights and rows)
    p, obs, act, _, _, _, max_ep = helpers.pt_case_inputs(case)
    m = make_model(p, S, A, max_ep, heads)
    n_rows = obs.shape[0]
    n_win = torch.cuda.get_device_properties(0).multi_processor_count * 9 + 5
    lens = rng.integers(1, QL + 1, n_win).astype(np.int32)
    starts = rng.integers(0, n_rows - QL, n_win).astype(np.int64)
    t0 = rng.integers(0, max_ep - QL, n_win).astype(np.int32)
    o, a, st, ln, tt = guarded(obs), guarded(act), dv(starts), dv(lens), dv(t0)
    got = m.window_values(o, a, st, ln, QL, win_t0=tt, kernel="tuned").cpu().numpy()
    assert np.isfinite(got).all()
    alone = np.concatenate([m.window_values(o, a, st[i:i + 64], ln[i:i + 64], QL, win_t0=tt[i:i + 64],
                                            kernel="tuned").cpu().numpy() for i in range(0, n_win, 64)])
    np.testing.assert_array_equal(got, alone)
    pick = rng.choice(n_win, 24, replace=False)
    want = oracle_windows(p, obs, act, starts[pick], lens[pick], t0[pick], QL, heads, dtype=np.float64)
    np.testing.assert_allclose(got[pick], want, rtol=helpers.PT_TOL, atol=helpers.PT_TOL)


def run_prefixes(case, n, lengths, n_random, t0_zero=False):
    """The general path on prefixes of ONE stretch of n transitions against one float64 forward over
    it (oracle_prefixes), win_t0 given and None."""
    L, E, heads, I, S, A, QL = case
    p, obs, act, start, t0, lens, max_ep = helpers.pt_prefix_inputs(case, n, lengths, n_random)
    m = make_model(p, S, A, max_ep, heads, max_pos=2 * QL)
    o, a = guarded(obs), guarded(act)
    st, ln = dv(np.full(len(lens), start, np.int64)), dv(lens)
    first = None
    for tt in (0 if t0_zero else t0, None):
        got = m.window_values(o, a, st, ln, QL, win_t0=None if tt is None else dv(np.full(len(lens), tt, np.int32)),
                              kernel="general").cpu().numpy()
        if t0_zero and first is not None:  # timesteps 0.. either way: one forward serves both runs
            np.testing.assert_array_equal(got, first)
            continue
        first = got
        t = time.perf_counter()
        want = oracle_prefixes(p, obs, act, start, n, tt or 0, heads, dtype=np.float64)[lens - 1]
        seconds = time.perf_counter() - t
        d = np.abs(got - want)
        print(f"general {pt_case_id(case)} prefixes of {n}, win_t0 {'given' if tt is not None else 'None'}: lens "
              f"{lens.tolist()}, max |d| {d.max():.3g}, median {np.median(d):.3g}; oracle forward {seconds:.1f} s")
        check_close(got, want, short=lens <= 8)


def test_general_path_long_windows():
    """query_length 1024 (tp = 2048: 64 token tiles a window): the prefixes of lengths 1, 2, 511, 512,
    513, 1023, 1024 and 8 random ones of one stretch of rows.
    Observed on an MI355X: max / median |d| 2.2e-04 / 1.2e-06 with win_t0 given, 1.4e-04 / 1.2e-06 with None."""
    run_prefixes(helpers.PT_GENERAL_LONG, 1024, [1, 2, 511, 512, 513, 1023, 1024], 8)


def test_general_path_top_of_the_envelope():
    """query_length 4096, the stated top (tp = 8192): windows of lengths 1, 2, 2047, 2048, 4095 and 4096
    against ONE float64 forward over the 4096 transitions (9.5 s on one core of the development host,
    under the 30 s at which 2048 would have taken its place).  The timesteps start at 0, so that this
    one forward is the reference of the run with win_t0 given and of the run with None; the two runs
    are bit-identical.  Observed on an MI355X: max / median |d| 4.4e-06 / 4.3e-07."""
    n = helpers.PT_GENERAL_TOP[6]
    run_prefixes(helpers.PT_GENERAL_TOP, n, [1, 2, n // 2 - 1, n // 2, n - 1, n], 0, t0_zero=True)


def short_windows(rng, n_rows, max_ep):
    lens = np.concatenate([np.arange(1, 21), rng.integers(1, 21, 20)]).astype(np.int32)
    starts = np.array([rng.integers(0, n_rows - l + 1) for l in lens], np.int64)
    t0 = np.array([rng.integers(0, max_ep + 2 - l) for l in lens], np.int32)
    return lens, starts, t0


@pytest.mark.parametrize("kernel,big", [("tuned", 300), ("general", 4096)])
def test_value_does_not_depend_on_query_length(kernel, big):
    """query_length enters both paths only through the clamp and, on the general path, the row pitch tp
    of a window: the same 40 windows of length <= 20 under query_length 20 and under 300 (tuned) or 4096
    (general, two blocks: tp = 8192) are bit-identical, with win_t0 given and None."""
    S, A, heads, max_ep, n_rows = 5, 3, 4, big + 20, 300  # (win_t0 None: the timestep table holds query_length)
    rng = np.random.default_rng(big)
    from oracle import relabel_oracle as ro
    p = ro.make_pt_params(rng, S, A, max_ep, embd=64, pref=8, inter=256 if kernel == "tuned" else 64,
                          layers=1 if kernel == "tuned" else 2)
    m = make_model(p, S, A, max_ep, heads, max_pos=2 * big)
    obs = rng.standard_normal((n_rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    lens, starts, t0 = short_windows(rng, n_rows, max_ep)
    o, a, st, ln = guarded(obs), guarded(act), dv(starts), dv(lens)
    for tt in (dv(t0), None):
        small = m.window_values(o, a, st, ln, 20, win_t0=tt, kernel=kernel).cpu().numpy()
        large = m.window_values(o, a, st, ln, big, win_t0=tt, kernel=kernel).cpu().numpy()
        assert np.isfinite(small).all()
        np.testing.assert_array_equal(large, small)
    want = oracle_windows(p, obs, act, starts, lens, None, 20, heads, dtype=np.float64)
    check_close(small, want, short=lens <= 8)


def entry_values(m, kernel, obs, act, starts, lens, t0, QL):
    """The C entry point itself (RewardPT.window_values raises on t0 + len > n_temb before it calls)."""
    from iqlpref_amd import _lib
    lib = _lib.load()
    st, ln, tt = dv(np.asarray(starts, np.int64)), dv(np.asarray(lens, np.int32)), dv(np.asarray(t0, np.int32))
    out = torch.full((len(lens),), float("nan"), dtype=torch.float32, device=DEV)
    if kernel == "general":
        w, keep = m._general_model()
        nbytes = C.c_size_t()
        _lib.check(lib.iqlhip_pt_general_workspace_bytes(C.byref(w), QL, len(lens), C.byref(nbytes)))
        ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=DEV)
        _lib.check(lib.iqlhip_pt_relabel_general(C.byref(w), _lib.ptr(obs), _lib.ptr(act), obs.shape[0], _lib.ptr(st),
                                                 _lib.ptr(ln), _lib.ptr(tt), len(lens), QL, _lib.ptr(ws), nbytes.value,
                                                 _lib.ptr(out), _lib.stream_ptr()))
    else:
        w, keep, _ = m._weights()
        _lib.check(lib.iqlhip_pt_relabel(C.byref(w), _lib.ptr(obs), _lib.ptr(act), obs.shape[0], _lib.ptr(st),
                                         _lib.ptr(ln), _lib.ptr(tt), len(lens), QL, _lib.ptr(out), _lib.stream_ptr()))
    res = out.cpu().numpy()
    del keep
    return res


@pytest.mark.parametrize("kernel", ["tuned", "general"])
def test_windows_outside_their_preconditions_are_clamped(kernel):
    """include/iqlhip.h: a window that violates its preconditions "yields a value for the clamped window,
    never an out-of-bounds read".  Each precondition broken on its own -- len 0, -3, query_length + 5;
    start -4, n_rows - 2 with len 5, n_rows + 100; t0 -1, n_temb - 1 with len 3 -- among valid windows,
    and a dataset of 3 rows under query_length 8: bit-identical to the same call with the windows
    clamped on the host (helpers.pt_clamp_windows), and finite with the NaN rows around obs / act."""
    S, A, heads, max_ep, QL = 5, 3, 4, 40, 8
    rng = np.random.default_rng(7)
    from oracle import relabel_oracle as ro
    p = ro.make_pt_params(rng, S, A, max_ep, embd=64, pref=8, inter=256 if kernel == "tuned" else 64,
                          layers=1 if kernel == "tuned" else 2)
    m = make_model(p, S, A, max_ep, heads)
    n_temb = max_ep + 1
    for n_rows in (60, 3):
        obs = rng.standard_normal((n_rows, S)).astype(np.float32)
        act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
        o, a = guarded(obs), guarded(act)
        if n_rows == 60:
            #          len: 0, -3, QL + 5 | start: -4, n_rows - 2, n_rows + 100 | t0: -1, n_temb - 1 | valid
            lens = [0, -3, QL + 5, 5, 5, 3, 4, 3, 1, 8, 5]
            starts = [10, 11, 12, -4, n_rows - 2, n_rows + 100, 20, 21, 0, n_rows - 8, 30]
            t0 = [3, 4, 5, 6, 7, 8, -1, n_temb - 1, 0, n_temb - 8, 9]
        else:
            lens, starts, t0 = [8, 8, 2], [0, 1, 1], [0, 5, 7]
        cs, cl, ct = helpers.pt_clamp_windows(starts, lens, t0, n_rows, n_temb, QL)
        assert (cs >= 0).all() and (cs + cl <= n_rows).all() and (ct >= 0).all() and (ct + cl <= n_temb).all()
        got = entry_values(m, kernel, o, a, starts, lens, t0, QL)
        want = entry_values(m, kernel, o, a, cs, cl, ct, QL)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, want)
        # the clamped windows are valid ones: RewardPT.window_values takes them, and the oracle agrees
        via = m.window_values(o, a, dv(cs), dv(cl), QL, win_t0=dv(ct), kernel=kernel).cpu().numpy()
        np.testing.assert_array_equal(via, want)
        check_close(want, oracle_windows(p, obs, act, cs, cl, ct, QL, heads, dtype=np.float64))
        # without win_t0 (timesteps 0..): the len and start violations through window_values itself
        keep = np.array(t0) == ct
        got0 = m.window_values(o, a, dv(np.asarray(starts, np.int64)[keep]), dv(np.asarray(lens, np.int32)[keep]), QL,
                               kernel=kernel).cpu().numpy()
        want0 = m.window_values(o, a, dv(cs[keep]), dv(cl[keep]), QL, kernel=kernel).cpu().numpy()
        assert np.isfinite(got0).all()
        np.testing.assert_array_equal(got0, want0)
