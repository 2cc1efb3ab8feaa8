"""iqlhip_cvar_tail_mean over its stated envelope (1 <= n_tail <= S <= 2400, any N) against the fp64
np.sort(col)[:n_tail].mean() per column.  -m gpu.

The launcher (csrc/cvar.hip) picks k_cvar<COLS, L> from S: <128,2> up to 32 rows, <64,4> to 64,
<32,8> to 128, <32,16> to 256, <32,32> to 1248 and <16,32> beyond.  S below has both sides of every
such boundary, N both sides of every COLS, n_tail both sides of the short-tail path (8 | 9).  The
selection is exact by construction, so only the fp32 summation order separates the kernel from the
reference: the bound is that of helpers.cvar_ref, per column -- far below what one wrongly chosen
element would cost."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_ALL = (2, 3, 32, 33, 64, 65, 67, 128, 129, 131, 256, 257, 1248, 1249, 1251, 2399, 2400)
SENTINEL = -12345.0


def _n_list(S):
    cols, _ = helpers.cvar_launch_config(S)
    return ((1,) if S in (2, 2400) else ()) + (cols - 1, cols + 1, 2 * cols + 3)


def _run(preds, n_tail):
    from iqlpref_amd.relabel import cvar_tail_mean_device
    return cvar_tail_mean_device(preds, n_tail).cpu().numpy()


def test_the_s_list_meets_every_launch_configuration():
    assert {helpers.cvar_launch_config(S) for S in S_ALL} == {(128, 2), (64, 4), (32, 8), (32, 16), (32, 32), (16, 32)}
    assert all(max(_n_list(S)) <= 260 for S in S_ALL)


@pytest.mark.parametrize("S", S_ALL)
def test_tail_mean_of_every_column_family(S):
    rng = np.random.default_rng(S)
    worst = 0.0
    for N in _n_list(S):
        for n_tail in helpers.cvar_n_tails(S):
            preds, names = helpers.cvar_matrix(rng, S, N, n_tail, first=S + n_tail)
            got = _run(torch.from_numpy(preds).to(DEV), n_tail)
            want, tol = helpers.cvar_ref(preds, n_tail)
            err = np.abs(got.astype(np.float64) - want)
            bad = np.flatnonzero(~(err <= tol))
            worst = max(worst, float(np.max(err / np.maximum(tol, 1e-300))))
            assert bad.size == 0, (f"S={S} N={N} n_tail={n_tail}: columns {bad[:8]} ({[names[c] for c in bad[:8]]}) "
                                   f"got {got[bad[:8]]} want {want[bad[:8]]} bound {tol[bad[:8]]}")
            if n_tail == 1:  # the column minimum itself (IEEE leaves the sign of a zero minimum open)
                mn = preds.min(axis=0)
                nz = mn != 0
                np.testing.assert_array_equal(got[nz].view(np.uint32), mn[nz].view(np.uint32))
                assert np.all(got[~nz] == 0)
    print(f"S={S}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("S", S_ALL)
def test_integer_columns_are_summed_exactly(S):
    """Integer entries in [-1000, 1000]: every fp32 partial sum is exact in any order, only the final
    division rounds -- and the build divides with correct rounding (no fast-math flag; hipcc's default
    fp32 division is IEEE), so the result is THE float of int_sum / n_tail, bit for bit."""
    rng = np.random.default_rng(1000 + S)
    cols, _ = helpers.cvar_launch_config(S)
    preds = helpers.cvar_int_matrix(rng, S, 2 * cols + 3)
    dev = torch.from_numpy(preds).to(DEV)
    for n_tail in helpers.cvar_n_tails(S):
        int_sum = np.sort(preds.astype(np.int64), axis=0)[:n_tail].sum(axis=0)
        assert np.abs(int_sum).max() < 1 << 24
        want = int_sum.astype(np.float32) / np.float32(n_tail)
        np.testing.assert_array_equal(_run(dev, n_tail), want, err_msg=f"S={S} n_tail={n_tail}")


def test_refusals_leave_the_output_alone():
    from iqlpref_amd import _lib
    lib = _lib.load()
    preds = torch.zeros(2401, 8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    call = lambda S, n_tail: _lib.check(lib.iqlhip_cvar_tail_mean(_lib.ptr(preds), S, 8, n_tail, _lib.ptr(out),
                                                                  _lib.stream_ptr()))
    with pytest.raises(NotImplementedError):  # IQLHIP_ERR_UNSUPPORTED
        call(2401, 100)
    for S, n_tail in ((20, 0), (20, 21), (2400, 2401), (0, 1)):
        with pytest.raises(ValueError):       # IQLHIP_ERR_INVALID
            call(S, n_tail)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == np.float32(SENTINEL))
    call(2400, 2400)  # the envelope's end itself is served
    assert np.all(out.cpu().numpy() == 0)
