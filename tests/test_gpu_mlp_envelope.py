"""iqlhip_mlp_forward over the envelope include/iqlhip.h states (1..8 layers, widths 1..1024, both
weight layouts, every activation code, row strides, dropout) against a plain fp64 numpy forward
(tests/helpers.py:mlp_forward_ref).  -m gpu.

Which kernel a case enters (csrc/mlp_f32.hip): a net with a width above 256 runs k_mlp_wide; any
other runs k_mlp_f32<0> (relu hidden layers), <1> (tanh) or <2> (a table activation, hidden or
final).  Its last layer takes the k-split narrow path up to 48 outputs and the main path from 49."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import philox
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = helpers.ACT_FLAX_BASE  # code T + i: entry i of the table (cos, tanh, relu, softplus, sin, leaky_relu, swish, none)
ROWS = (1, 17, 64, 65, 130)  # k_mlp_f32, 64-row tiles: one row, a partial tile, a full one, one more row, three tiles
ROWS_WIDE = (1, 16, 17, 40)  # k_mlp_wide, 16-row groups
TOL = 2e-5                   # the project's rtol = atol for fp32 forwards of up to four layers


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _is_wide(dims):
    return max(dims) > 256


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, list) else str(v)


def _seed(dims):
    return sum((i + 1) * d for i, d in enumerate(dims))


def _inputs(dims, rng=None):
    rng = rng or np.random.default_rng(_seed(dims))
    ws, bs = helpers.mlp_weights_for(rng, dims)
    n = max(ROWS_WIDE if _is_wide(dims) else ROWS)
    return ws, bs, rng.standard_normal((n, dims[0])).astype(np.float32)


def _check(dims, hidden, out, ws, bs, x, atol=TOL, rtol=TOL, dropout=None):
    """Every row count and both layouts against the fp64 forward; the layouts bit-equal to each other."""
    import iqlpref_amd as ia
    assert [w.shape[0] for w in ws] + [ws[-1].shape[1]] == list(dims)
    keeps = scale = None
    if dropout is not None:
        p, seed, call = dropout
        scale = np.float32(1) / np.float32(1 - p)
        # (the descriptor holds p as a float: the threshold is that of the rounded value)
        keeps = [philox.mlp_dropout_keep(seed, call, l, x.shape[0], dims[l + 1], float(np.float32(p)))
                 for l in range(len(ws) - 1)]
    want = helpers.mlp_forward_ref(ws, bs, x, hidden, out, keeps=keeps, scale=scale)
    tb, tx = [_up(b) for b in bs], _up(x)
    t_io, t_oi = [_up(w) for w in ws], [_up(w.T) for w in ws]
    last = None
    for n in (ROWS_WIDE if _is_wide(dims) else ROWS):
        got = [ia.mlp_forward_f32(tw, tb, tx[:n], w_in_out=io, hidden_act=hidden, out_act=out,
                                  dropout=dropout).cpu().numpy() for io, tw in ((True, t_io), (False, t_oi))]
        assert got[0].shape == (n, dims[-1])
        err = np.abs(got[0] - want[:n])
        print(f"dims={dims} act=({hidden},{out}) n={n}: max |err| = {err.max():.3e}")
        np.testing.assert_allclose(got[0], want[:n], rtol=rtol, atol=atol, err_msg=f"dims={dims} n={n}")
        # the repack writes one fragment image from either layout
        np.testing.assert_array_equal(got[0].view(np.uint32), got[1].view(np.uint32), err_msg=f"layouts, n={n}")
        last = got[0]
    return last


# ---- the last layer's path boundary (narrow up to 48 outputs, main from 49) in every instantiation
def _boundary_cases():
    out = []
    for stem in ([8, 16], [20, 64, 32]):
        for n_out in (1, 16, 17, 33, 48, 49, 64, 200, 256):
            for hidden in (0, 1, T + 6):      # relu -> k_mlp_f32<0>, tanh -> <1>, swish -> <2>
                for fin in (0, 1, T + 0):     # none, tanh, cos (cos puts <0> and <1> nets into <2> as well)
                    out.append((stem + [n_out], hidden, fin))
    return out


# [8, 16, 64] and [8, 16, 256] with a table activation: k_mlp_f32<2>, no width above 256, a main-path
# last layer.  Its raw sums pass through the LDS buffer, whose row stride was sized from dims[:-1]
# alone (round_up(16, 16) + 4 = 20 < 64): rows aliased each other and the highest store left the
# allocation.  Both shapes are in _boundary_cases() with swish and with cos; named here so that they
# stay in the table whatever happens to the lists above.
STRIDE_DEFECT_SHAPES = ([8, 16, 64], [8, 16, 256])


def test_the_stride_defect_shapes_are_in_the_table():
    cases = _boundary_cases()
    for dims in STRIDE_DEFECT_SHAPES:
        assert (dims, T + 6, 0) in cases and (dims, 0, T + 0) in cases and (dims, T + 6, T + 0) in cases
        assert max(dims) <= 256 and -(-dims[-1] // 16) * 16 >= 64 and -(-dims[-1] // 16) * 16 > -(-max(dims[:-1]) // 16) * 16 + 4


@pytest.mark.parametrize("dims,hidden,fin", _boundary_cases(), ids=_id)
def test_last_layer_path_boundary(dims, hidden, fin):
    _check(dims, hidden, fin, *_inputs(dims))


# ---- every table entry, hidden and final, on the main path of k_mlp_f32<2> and in k_mlp_wide
@pytest.mark.parametrize("dims", ([10, 32, 48, 80], [10, 272, 40, 5]), ids=("main", "wide"))
@pytest.mark.parametrize("i", range(8))
def test_every_table_activation(dims, i):
    _check(dims, T + i, T + (i + 3) % 8, *_inputs(dims))


# ---- depth, and 1024 (the envelope's end) as input, hidden and output width.  For the eight-layer and
# the 1024-wide nets the bound is derived, not guessed: 4x what a plain fp32 numpy forward of the same
# net is away from the fp64 one over the case's rows (another, equally valid fp32 summation order),
# with the project's 2e-5 as the floor, absolute.  The fp32-vs-fp64 figures beside the cases are the
# largest absolute differences this file's inputs give for hidden relu / tanh / swish: 4x each lies
# below the floor, which is therefore the bound in force.
DEEP = [
    ([5, 1], False),                                    # one layer: the narrow path alone
    ([37, 64], False),                                  # one layer on the main path
    ([300, 7], False),                                  # one layer, wide through its input
    ([6, 24, 24, 24, 24, 24, 24, 24, 3], True),         # 8.5e-8 / 2.3e-7 / 2.2e-8
    ([6, 24, 24, 24, 300, 24, 24, 24, 3], True),        # 1.1e-7 / 3.2e-7 / 3.5e-8  (k_mlp_wide: one layer > 256)
    ([1024, 16, 2], True),                              # 1.1e-6 / 7.3e-7 / 1.1e-6
    ([7, 1024, 2], True),                               # 2.5e-7 / 2.6e-7 / 3.9e-7
    ([7, 16, 1024], True),                              # 8.4e-7 / 4.6e-7 / 7.9e-7
]


def _fp32_gap(dims, hidden, fin, ws, bs, x):
    return float(np.abs(helpers.mlp_forward_ref(ws, bs, x, hidden, fin, dtype=np.float32).astype(np.float64)
                        - helpers.mlp_forward_ref(ws, bs, x, hidden, fin)).max())


@pytest.mark.parametrize("hidden", (0, 1, T + 6), ids=("relu", "tanh", "swish"))
@pytest.mark.parametrize("dims,derived", DEEP, ids=_id)
def test_depth_and_the_widest_layers(dims, derived, hidden):
    ws, bs, x = _inputs(dims)
    if not derived:  # up to four layers and 256 wide: the project's tolerance
        _check(dims, hidden, 0, ws, bs, x)
        return
    gap = _fp32_gap(dims, hidden, 0, ws, bs, x)
    print(f"dims={dims} hidden={hidden}: fp32 numpy vs fp64 = {gap:.3e}")
    _check(dims, hidden, 0, ws, bs, x, atol=max(4 * gap, TOL), rtol=0)


# ---- widths of 1 and widths off the 16-column tile
@pytest.mark.parametrize("hidden,fin", ((0, 0), (1, 1), (T + 0, T + 3)), ids=("relu", "tanh", "cos-softplus"))
@pytest.mark.parametrize("dims", ([1, 1, 1], [1, 15, 1], [17, 1, 17], [31, 33, 15, 2]), ids=_id)
def test_widths_of_one_and_off_tile(dims, hidden, fin):
    _check(dims, hidden, fin, *_inputs(dims))


# ---- the boundary between the two kernels, 256 | 257, as hidden, input and output width: the smaller
# net is the larger one's weights cut down, so the two sides differ in that one width only
@pytest.mark.parametrize("hidden", (0, 1, T + 4), ids=("relu", "tanh", "sin"))
@pytest.mark.parametrize("pos,big", ((1, [12, 257, 9]), (0, [257, 40, 3]), (2, [12, 40, 257])), ids=("hidden", "in", "out"))
def test_kernel_boundary_256_257(pos, big, hidden):
    rng = np.random.default_rng(257 + pos)
    ws, bs = helpers.mlp_weights_for(rng, big)
    x = rng.standard_normal((max(ROWS), big[0])).astype(np.float32)
    for width in (256, 257):
        dims = list(big)
        dims[pos] = width
        w2 = [w[:dims[l], :dims[l + 1]] for l, w in enumerate(ws)]
        b2 = [b[:dims[l + 1]] for l, b in enumerate(bs)]
        assert _is_wide(dims) == (width == 257)
        n = max(ROWS_WIDE if width == 257 else ROWS)
        _check(dims, hidden, 0, w2, b2, np.ascontiguousarray(x[:n, :dims[0]]))


# ---- dropout away from the actor's shape
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("hidden", (1, T + 3), ids=("tanh", "softplus"))
@pytest.mark.parametrize("dims", ([9, 40, 24, 3], [9, 300, 24, 3]), ids=("w40", "wide"))
def test_dropout_masks_follow_the_philox_oracle(dims, hidden, p):
    """Width 40 is padded to 48 columns: the dropout pass runs over the padding too.  softplus(0) != 0:
    a padding column that took the activation would show in the next layer."""
    ws, bs, x = _inputs(dims)
    a = _check(dims, hidden, 0, ws, bs, x, dropout=(p, 1234567890123, 7))
    b = _check(dims, hidden, 0, ws, bs, x, dropout=(p, 1234567890123, 8))
    assert not np.array_equal(a, b)  # a fresh mask per dropout_call
    assert not np.array_equal(a, _check(dims, hidden, 0, ws, bs, x))


# ---- row strides: only a C caller can pass them
def _call(ws, bs, hidden, fin, x_ptr, n, x_stride, out_ptr, out_stride):
    from iqlpref_amd import _lib
    d = _lib.MlpDesc()
    d.n_layers = len(ws)
    for i, (w, b) in enumerate(zip(ws, bs)):
        d.dims[i], d.dims[i + 1] = w.shape
        d.weights[i], d.biases[i] = w.data_ptr(), b.data_ptr()
    d.w_in_out, d.hidden_act, d.out_act = 1, hidden, fin
    _lib.check(_lib.load().iqlhip_mlp_forward(C.byref(d), C.c_void_p(x_ptr), n, x_stride, C.c_void_p(out_ptr),
                                              out_stride, _lib.stream_ptr()))
    torch.cuda.synchronize()


SENTINEL = -12345.0


@pytest.mark.parametrize("dims", ([11, 20, 1], [11, 20, 24], [11, 20, 80], [11, 260, 24]), ids=_id)
def test_row_strides_through_the_c_entry_point(dims):
    import iqlpref_amd as ia
    rng = np.random.default_rng(_seed(dims))
    ws, bs = helpers.mlp_weights_for(rng, dims)
    tw, tb = [_up(w) for w in ws], [_up(b) for b in bs]
    n, k_in, n_out = 70, dims[0], dims[-1]
    hidden, fin = T + 6, 1
    wide_x = _up(rng.standard_normal((n, k_in + 5)).astype(np.float32))
    x = wide_x[:, 3:3 + k_in].contiguous()
    dense = ia.mlp_forward_f32(tw, tb, x, w_in_out=True, hidden_act=hidden, out_act=fin).cpu().numpy()
    np.testing.assert_allclose(dense, helpers.mlp_forward_ref(ws, bs, x.cpu().numpy(), hidden, fin), rtol=TOL, atol=TOL)
    # x: a column window of a wider matrix; out: a column window of a wider, sentinel-filled matrix
    wide_out = torch.full((n, n_out + 3), SENTINEL, dtype=torch.float32, device=DEV)
    _call(tw, tb, hidden, fin, wide_x.data_ptr() + 3 * 4, n, k_in + 5, wide_out.data_ptr() + 2 * 4, n_out + 3)
    got = wide_out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 2:2 + n_out].view(np.uint32), dense.view(np.uint32))
    outside = np.delete(got, np.s_[2:2 + n_out], axis=1)
    assert outside.shape == (n, 3) and np.all(outside == np.float32(SENTINEL))
    # strides below the row width are refused
    for xs, os_ in ((k_in - 1, n_out + 3), (k_in + 5, n_out - 1)):
        with pytest.raises(ValueError):
            _call(tw, tb, hidden, fin, wide_x.data_ptr(), n, xs, wide_out.data_ptr(), os_)
    assert np.array_equal(wide_out.cpu().numpy(), got)
    if n_out == 1:
        # what the header documents: out_stride = 1 writes the n predictions into row k of an [S][N] matrix
        S, k = 4, 2
        preds = torch.full((S, n), SENTINEL, dtype=torch.float32, device=DEV)
        _call(tw, tb, hidden, fin, wide_x.data_ptr() + 3 * 4, n, k_in + 5, preds.data_ptr() + k * n * 4, 1)
        got = preds.cpu().numpy()
        np.testing.assert_array_equal(got[k].view(np.uint32), dense[:, 0].view(np.uint32))
        assert np.all(np.delete(got, k, axis=0) == np.float32(SENTINEL))


def test_what_the_entry_point_refuses():
    """Nothing of the stated envelope is skipped above; what lies outside it is refused, not run."""
    import iqlpref_amd as ia
    x = torch.zeros(4, 3, device=DEV)
    mk = lambda dims: ([torch.zeros(dims[i], dims[i + 1], device=DEV) for i in range(len(dims) - 1)],
                       [torch.zeros(dims[i + 1], device=DEV) for i in range(len(dims) - 1)])
    with pytest.raises(NotImplementedError):
        ia.mlp_forward_f32(*mk([3, 1025, 2]), x, w_in_out=True)
    from iqlpref_amd import _lib
    ws, bs = mk([3, 4, 2])
    for n_layers in (0, 9):  # (the Python wrapper cannot describe these)
        d = _lib.MlpDesc()
        d.n_layers = n_layers
        for i in range(9):
            d.dims[i] = 4
        for i in range(8):
            d.weights[i], d.biases[i] = ws[0].data_ptr(), bs[0].data_ptr()
        out = torch.zeros(4, 4, device=DEV)
        with pytest.raises(ValueError):
            _lib.check(_lib.load().iqlhip_mlp_forward(C.byref(d), _lib.ptr(x), 4, 4, _lib.ptr(out), 4, _lib.stream_ptr()))
    for code in (2, 7, 16, -1):
        with pytest.raises(ValueError):
            ia.mlp_forward_f32(*mk([3, 4, 2]), x, w_in_out=True, hidden_act=code)
        with pytest.raises(ValueError):
            ia.mlp_forward_f32(*mk([3, 4, 2]), x, w_in_out=True, out_act=code)
    with pytest.raises(ValueError):
        ia.mlp_forward_f32(*mk([3, 4, 2]), x, w_in_out=True, dropout=(1.0, 0, 0))
