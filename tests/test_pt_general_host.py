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
