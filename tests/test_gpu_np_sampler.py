"""numpy's legacy RandomState.randint on the device (csrc/np_sampler.hip, iqlhip_np_randint), bit for bit
against numpy itself: the indices, and the whole state afterwards.  -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib
from iqlpref_amd import custom_offline as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIS = [1, 2, 3, 1000, 2 ** 19 + 1, 496113, 2 ** 20, 2 ** 31 + 1, 2 ** 32]


def _start(seed, how):
    """A RandomState at a chosen pos: 624 (fresh seed), 0, 1, 623, or after random(3) (pos 6)."""
    rs = np.random.RandomState(seed)
    if how == "p0":  # pos 0: the key is used as it stands, no twist first
        st = rs.get_state()
        rs.set_state((st[0], st[1], 0, 0, 0.0))
    elif how == "p1":
        rs.randint(0, 2 ** 32, size=1)
    elif how == "p623":
        rs.randint(0, 2 ** 32, size=623)
    elif how == "random3":
        rs.random_sample(3)
    return rs


def _device_draw(rss, his, n, B, state=None):
    """One iqlhip_np_randint launch over the states of ``rss`` (or the given device state)."""
    lib = _lib.load()
    K = len(his)
    if state is None:
        state = torch.from_numpy(np.stack([co.pack_np_state(r.get_state()) for r in rss]).view(np.int32)).to(DEV)
    outs = [torch.full((n, B), -7, dtype=torch.int64, device=DEV) for _ in range(K)]
    with torch.cuda.device(DEV):
        _lib.check(lib.iqlhip_np_randint(_lib.ptr(state), (C.c_int64 * K)(*his), K, B, n,
                                         (C.c_void_p * K)(*[o.data_ptr() for o in outs]), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], state


def _host_draw(rs, hi, n, B):
    return np.stack([rs.randint(0, hi, size=B) for _ in range(n)])


def _check(rs_dev_state, rs_host, k=0):
    got = rs_dev_state.cpu().numpy().view(np.uint32)[k]
    want = co.pack_np_state(rs_host.get_state())
    assert int(got[624]) == int(want[624]), f"pos {got[624]} != {want[624]}"
    np.testing.assert_array_equal(got[:624], want[:624])


@pytest.mark.parametrize("hi", HIS)
@pytest.mark.parametrize("how", ["fresh", "p0", "p1", "p623", "random3"])
def test_randint_matches_numpy(hi, how):
    seed = 17 + HIS.index(hi)
    B, n = 256, 7
    (got,), state = _device_draw([_start(seed, how)], [hi], n, B)
    host = _start(seed, how)
    want = _host_draw(host, hi, n, B)
    np.testing.assert_array_equal(got, want)
    _check(state, host)


@pytest.mark.parametrize("B", [1, 16, 256, 1000])
@pytest.mark.parametrize("n", [1, 7, 2000])
def test_batch_shapes(B, n):
    for hi in (496113, 2 ** 19 + 1):
        (got,), state = _device_draw([_start(B + n, "random3")], [hi], n, B)
        host = _start(B + n, "random3")
        np.testing.assert_array_equal(got, _host_draw(host, hi, n, B))
        _check(state, host)


def test_two_calls_are_one_stream():
    """5 + 7 batches in two calls on the same device state = 12 batches in one call = numpy."""
    hi, B = 2 ** 19 + 1, 100
    (a,), state = _device_draw([_start(3, "fresh")], [hi], 5, B)
    (b,), state = _device_draw(None, [hi], 7, B, state=state)
    (c,), state12 = _device_draw([_start(3, "fresh")], [hi], 12, B)
    np.testing.assert_array_equal(np.concatenate([a, b]), c)
    host = _start(3, "fresh")
    np.testing.assert_array_equal(c, _host_draw(host, hi, 12, B))
    np.testing.assert_array_equal(state.cpu().numpy(), state12.cpu().numpy())
    _check(state, host)


def test_eight_streams_in_one_launch():
    his = [1000, 2 ** 19 + 1, 496113, 2 ** 32, 1, 3, 2 ** 31 + 1, 2 ** 20]
    hows = ["fresh", "p0", "p1", "p623", "random3", "fresh", "random3", "p1"]
    rss = [_start(100 + k, h) for k, h in enumerate(hows)]
    got, state = _device_draw(rss, his, 33, 64)
    for k, (hi, how) in enumerate(zip(his, hows)):
        host = _start(100 + k, how)
        np.testing.assert_array_equal(got[k], _host_draw(host, hi, 33, 64), err_msg=f"stream {k}")
        _check(state, host, k)


def test_index_stream_global_generator_and_gauss_fields():
    """NumpyIndexStream on numpy's global generator: after the call get_state() is exactly what the
    host draws leave, has_gauss / cached_gaussian included; consecutive calls alternate index areas."""
    stream = co.NumpyIndexStream(DEV)
    np.random.seed(5)
    np.random.standard_normal()  # has_gauss = 1
    before = np.random.get_state()
    got = [stream.draw(496113, 9, 32)[0].cpu().numpy() for _ in range(3)]
    after = np.random.get_state()
    np.random.set_state(before)
    want = [_host_draw(np.random, 496113, 9, 32) for _ in range(3)]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    ref = np.random.get_state()
    assert after[0] == ref[0] and after[2] == ref[2] and after[3] == ref[3] == 1 and after[4] == ref[4]
    np.testing.assert_array_equal(after[1], ref[1])


def test_index_stream_several_generators():
    stream = co.NumpyIndexStream(DEV)
    gens = [np.random.RandomState(s) for s in (1, 2, 3)]
    out = stream.draw([10, 2 ** 32, 77777], 20, 50, gens)
    for k, (s, hi) in enumerate(zip((1, 2, 3), (10, 2 ** 32, 77777))):
        host = np.random.RandomState(s)
        np.testing.assert_array_equal(out[k].cpu().numpy(), _host_draw(host, hi, 20, 50))
        np.testing.assert_array_equal(gens[k].get_state()[1], host.get_state()[1])
        assert gens[k].get_state()[2] == host.get_state()[2]


def test_invalid_arguments():
    lib = _lib.load()
    state = torch.from_numpy(co.pack_np_state(np.random.RandomState(0).get_state()).view(np.int32)[None]).to(DEV)
    out = torch.empty((2, 4), dtype=torch.int64, device=DEV)

    def call(his, K=1, B=4, n=2, st=state):
        with torch.cuda.device(DEV):
            _lib.check(lib.iqlhip_np_randint(_lib.ptr(st), (C.c_int64 * max(len(his), 1))(*his), K, B, n,
                                             (C.c_void_p * 17)(*([out.data_ptr()] * 17)), _lib.stream_ptr()))

    for his in ([0], [-5], [2 ** 32 + 1]):
        with pytest.raises(ValueError):
            call(his)
    with pytest.raises(ValueError):
        call([10] * 17, K=17)
    with pytest.raises(ValueError):
        call([10], K=0)
    with pytest.raises(ValueError):
        call([10], B=0)
    bad = state.clone()
    bad[0, 624] = 625
    with pytest.raises(ValueError):
        call([10], st=bad)
    before = state.clone()
    call([10])  # the valid call still works after the refusals
    torch.cuda.synchronize()
    assert not torch.equal(before, state)
    with pytest.raises(ValueError):
        co.NumpyIndexStream(DEV).draw(0, 2, 4)
