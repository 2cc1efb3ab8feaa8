"""Host side of the general preference-transformer path (iqlhip_pt_relabel_general): exports,
the shape envelope, the workspace query and the Python routing.  No device is touched: every
check here runs before any HIP call."""
import ctypes as C

import pytest
import torch

FAKE = 0x1000  # a non-null "device" pointer; the calls below refuse before they could use one


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    return _lib, _lib.load()


def _model(L=2, E=128, heads=4, I=512, S=29, A=8):
    _l, _ = _lib()
    blocks = (_l.PtBlock * L)()
    for b in blocks:
        for name, _t in _l.PtBlock._fields_:
            setattr(b, name, FAKE)
    m = _l.PtModel()
    m.state_dim, m.action_dim, m.embd_dim, m.num_heads = S, A, E, heads
    m.inter_dim, m.num_layers, m.n_temb, m.eps = I, L, 1001, 1e-5
    for name in ("state_wT", "state_b", "action_wT", "action_b", "temb", "sln_w", "sln_b",
                 "lnf_w", "lnf_b", "pref_w_last"):
        setattr(m, name, FAKE)
    m.blocks = C.cast(blocks, C.POINTER(_l.PtBlock))
    return m, blocks


def test_general_symbols_exported():
    _l, lib = _lib()
    for name in ("iqlhip_pt_relabel_general", "iqlhip_pt_general_workspace_bytes"):
        assert hasattr(lib, name) and name in _l.SYMBOLS


@pytest.mark.parametrize("field,value,needle", [
    ("num_layers", 9, "num_layers"), ("embd_dim", 96, "embd_dim"), ("embd_dim", 320, "embd_dim"),
    ("num_heads", 3, "num_heads"), ("num_heads", 64, "num_heads"),  # 64 heads of 128: head_dim 2
    ("inter_dim", 1088, "inter_dim"), ("state_dim", 250, "state_dim"),
])
def test_general_refuses_shapes_outside_envelope(field, value, needle):
    _l, lib = _lib()
    m, keep = _model()
    setattr(m, field, value)
    p = C.c_void_p(FAKE)
    rc = lib.iqlhip_pt_relabel_general(C.byref(m), p, p, 100, p, p, None, 10, 20, p, 1 << 20, p, None)
    assert rc == _l.ERR_UNSUPPORTED
    assert needle in lib.iqlhip_last_error().decode()
    nbytes = C.c_size_t()
    assert lib.iqlhip_pt_general_workspace_bytes(C.byref(m), 20, 10, C.byref(nbytes)) == _l.ERR_UNSUPPORTED


def test_general_accepts_envelope_corners():
    _l, lib = _lib()
    nbytes = C.c_size_t()
    for kw in (dict(L=1, E=64, heads=16, I=64, S=1, A=1), dict(L=8, E=256, heads=64, I=1024, S=200, A=56),
               dict(L=3, E=192, heads=1, I=320, S=45, A=24)):
        m, keep = _model(**kw)
        assert lib.iqlhip_pt_general_workspace_bytes(C.byref(m), 100, 1, C.byref(nbytes)) == 0, \
            lib.iqlhip_last_error().decode()


def test_general_workspace_grows_up_to_the_chunk_cap():
    _l, lib = _lib()
    m, keep = _model(L=2, E=256, heads=4, I=1024)
    size = lambda n: (lib.iqlhip_pt_general_workspace_bytes(C.byref(m), 100, n, C.byref(nbytes)), nbytes.value)[1]
    nbytes = C.c_size_t()
    sizes = [size(n) for n in (1, 2, 10, 100)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3]
    capped = size(10 ** 9)
    assert sizes[3] < capped == size(2 * 10 ** 9) <= 1 << 30
    # a workspace smaller than one window is refused before any launch
    p = C.c_void_p(FAKE)
    rc = lib.iqlhip_pt_relabel_general(C.byref(m), p, p, 1000, p, p, None, 10, 100, p, sizes[0] - 4, p, None)
    assert rc == _l.ERR_INVALID


def test_routing_and_max_pos_check():
    import iqlpref_amd as ia
    assert ia.RewardPT(29, 8, 100).tuned_shape()
    assert ia.RewardPT(29, 8, 100, num_heads=16, intermediate_dim=1024).tuned_shape()
    assert not ia.RewardPT(29, 8, 100, num_layers=2).tuned_shape()
    assert not ia.RewardPT(29, 8, 100, embd_dim=128).tuned_shape()
    assert not ia.RewardPT(29, 8, 100, intermediate_dim=320).tuned_shape()
    assert not ia.RewardPT(150, 100, 100).tuned_shape()
    # the general path checks 2 * query_length <= max_pos on the host, before any device work
    m = ia.RewardPT(5, 3, 50, num_layers=2, max_pos=16)
    obs, act = torch.zeros(20, 5), torch.zeros(20, 3)
    st, ln = torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="max_pos"):
        m.window_values(obs, act, st, ln, 9)
    with pytest.raises(ValueError, match="max_pos"):
        ia.RewardPT(5, 3, 50, max_pos=16).window_values(obs, act, st, ln, 9, kernel="general")
    with pytest.raises(ValueError, match="kernel"):
        m.window_values(obs, act, st, ln, 4, kernel="fast")


# ---- every edge of both stated envelopes (include/iqlhip.h): refused one step outside, accepted one
# ---- step inside.  The checks run ahead of any HIP call, so the fake pointers are never used.
def _tuned(S=29, A=8, E=64, heads=4, I=256, L=1):
    _l, _ = _lib()
    w = _l.PtWeights()
    w.state_dim, w.action_dim, w.embd_dim, w.num_heads = S, A, E, heads
    w.inter_dim, w.num_layers, w.n_temb, w.eps = I, L, 1001, 1e-5
    for name, t in _l.PtWeights._fields_:
        if t is C.c_void_p:
            setattr(w, name, FAKE)
    return w


@pytest.mark.parametrize("kw,needle", [
    (dict(S=185, A=8), "state/action"), (dict(S=1, A=192), "state/action"),  # S + A = 193
    (dict(I=320), "inter_dim"), (dict(I=1280), "inter_dim"), (dict(I=64), "inter_dim"),
    (dict(heads=3), "num_heads"), (dict(heads=32), "num_heads"),
    (dict(E=128), "embd_dim"), (dict(L=2), "num_layers"),
])
def test_tuned_refuses_shapes_outside_envelope(kw, needle):
    _l, lib = _lib()
    w = _tuned(**kw)
    p = C.c_void_p(FAKE)
    rc = lib.iqlhip_pt_relabel(C.byref(w), p, p, 100, p, p, None, 10, 20, p, None)
    assert rc == _l.ERR_UNSUPPORTED
    assert needle in lib.iqlhip_last_error().decode()


@pytest.mark.parametrize("kw,ql,needle", [
    (dict(E=96), 20, "embd_dim"), (dict(E=320), 20, "embd_dim"), (dict(E=0), 20, "embd_dim"),
    (dict(E=64, heads=32), 20, "num_heads"),  # head_dim 2
    (dict(heads=3), 20, "num_heads"), (dict(heads=0), 20, "num_heads"),
    (dict(I=96), 20, "inter_dim"), (dict(I=1088), 20, "inter_dim"), (dict(I=0), 20, "inter_dim"),
    (dict(S=249, A=8), 20, "state_dim"), (dict(S=1, A=256), 20, "state_dim"),  # S + A = 257
    (dict(), 4097, "query_length"),
    (dict(L=0), 20, "num_layers"), (dict(L=9), 20, "num_layers"),
])
def test_general_refuses_one_step_outside_every_edge(kw, ql, needle):
    _l, lib = _lib()
    L = kw.pop("L", 2)
    m, keep = _model(L=max(L, 1), **kw)
    m.num_layers = L
    p = C.c_void_p(FAKE)
    rc = lib.iqlhip_pt_relabel_general(C.byref(m), p, p, 100, p, p, None, 10, ql, p, 1 << 20, p, None)
    assert rc == _l.ERR_UNSUPPORTED
    assert needle in lib.iqlhip_last_error().decode()
    nbytes = C.c_size_t()
    assert lib.iqlhip_pt_general_workspace_bytes(C.byref(m), ql, 10, C.byref(nbytes)) == _l.ERR_UNSUPPORTED


@pytest.mark.parametrize("kw,ql", [
    (dict(L=8, E=256, heads=64, I=1024, S=128, A=128), 4096),  # every top at once
    (dict(L=8, E=256, heads=64, I=1024, S=255, A=1), 4096), (dict(L=8, E=256, heads=64, I=1024, S=1, A=255), 4096),
    (dict(L=1, E=192, heads=32, I=192), 20),   # head_dim 6
    (dict(L=1, E=64, heads=16, I=64, S=1, A=1), 1),  # every bottom at once; head_dim 4
    (dict(L=2, E=256, heads=1, I=1024), 4096),  # head_dim 256
])
def test_general_accepts_one_step_inside_every_edge(kw, ql):
    _l, lib = _lib()
    m, keep = _model(**kw)
    nbytes = C.c_size_t()
    assert lib.iqlhip_pt_general_workspace_bytes(C.byref(m), ql, 1, C.byref(nbytes)) == 0, \
        lib.iqlhip_last_error().decode()
    tp = -(-2 * ql // 32) * 32  # a window's token rows: X [tp][E], QKV [tp][3E], O / H [tp][max(E, I)], + its tail row
    mx = max(m.embd_dim, m.inter_dim)
    assert nbytes.value == 4 * (tp * (4 * m.embd_dim + mx) + 32 * (2 * m.embd_dim + mx))
