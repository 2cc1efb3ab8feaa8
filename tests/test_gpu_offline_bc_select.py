"""The any-percent selection on the device (csrc/prep.hip: iqlhip_prep_trajectory_returns,
iqlhip_prep_gather_trajectories; offline_bc.select_best_trajectories).  -m gpu.

Against tests/golden/offline_bc_select.npz -- the reference's own keep_best_trajectories -- and against the host
restatement run in this process, bit for bit: first rows, lengths, the returns as raw bits, the kept trajectory
numbers and the five gathered arrays.  ORDER is compared with the golden arrays on the cases whose returns are
pairwise distinct; the all-zero case is compared with the host path of this process only (the order among equal
returns is the sorting host's).  The cases (tests/offline_bc_env.py) are the smallest at which the kernels take
another path: one row, one trajectory, every row a trajectory, cuts and terminals that coincide and alternate, a
terminal on a cut, a dropped trailing run, 3001 rows across the scan's 1024-row chunks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import minari_cases as mc, offline_bc_env as obe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
WIDTHS = (1, 3, 17, 45, 128)  # odd, a multiple of 4 only at 128 (the step's widest state), rows off 16-byte boundaries


@pytest.fixture(scope="module")
def select(golden_dir):
    return mc.load(golden_dir, "offline_bc_select.npz")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _raw_returns(rew, done, max_len, discount=0.99, n=None, scale_rows=None):
    """The entry point itself on sentinel-filled outputs: (rc, starts, lengths, returns, count)."""
    from iqlpref_amd import _lib, offline_bc
    lib = _lib.load()
    n = rew.shape[0] if n is None else n
    scale = _dev(offline_bc.return_scale_table(discount, max(1, min(max_len, 4096) if scale_rows is None else scale_rows)))
    starts = torch.full((rew.shape[0] + 1,), -7, dtype=torch.int64, device=DEV)
    lengths = torch.full((rew.shape[0] + 1,), -7, dtype=torch.int64, device=DEV)
    returns = torch.full((rew.shape[0] + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    count = C.c_int64(-7)
    with torch.cuda.device(DEV):
        rc = lib.iqlhip_prep_trajectory_returns(_lib.ptr(rew), _lib.ptr(done), n, max_len, _lib.ptr(scale), _lib.ptr(starts),
                                                _lib.ptr(lengths), _lib.ptr(returns), C.byref(count), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, starts.cpu().numpy(), lengths.cpu().numpy(), returns.cpu().numpy(), count.value


@pytest.mark.parametrize("name", [n for n in sorted(obe.CASES) if n != "n1_open"])
def test_trajectories_and_returns_are_the_references(select, name):
    """Starts, lengths and the bits of the returns: golden = host restatement = device; nothing is written behind
    the last trajectory."""
    from iqlpref_amd import offline_bc
    n, max_len, term_rows, fracs, ordered = obe.CASES[name]
    g = mc.run_of(select, f"{name}/float32")
    data = obe.selection_case(name)
    h_starts, h_lengths = offline_bc.trajectory_bounds(data["terminals"], max_len)
    h_returns = offline_bc.trajectory_returns(data["rewards"], h_starts, h_lengths, 0.99)
    rc, starts, lengths, returns, count = _raw_returns(_dev(data["rewards"]), _dev(data["terminals"], torch.uint8), max_len,
                                                       scale_rows=min(max_len, n))
    assert rc == 0 and count == len(g["starts"]) == len(h_starts)
    for got, host, gold in ((starts, h_starts, g["starts"]), (lengths, h_lengths, g["lengths"])):
        np.testing.assert_array_equal(got[:count], gold)
        np.testing.assert_array_equal(host, gold)
        assert (got[count:] == -7).all()
    np.testing.assert_array_equal(bits(returns[:count]), bits(g["returns"]))
    np.testing.assert_array_equal(bits(h_returns), bits(g["returns"]))
    assert (returns[count:] == SENTINEL).all()
    s, l, r = offline_bc.device_trajectory_returns(_dev(data["rewards"]), _dev(data["terminals"], torch.uint8), 0.99, max_len)
    assert s.shape == l.shape == r.shape == (count,)
    np.testing.assert_array_equal(bits(r.cpu().numpy()), bits(g["returns"]))


def test_no_complete_trajectory_is_an_error_and_writes_nothing(select):
    """n = 1 without a terminal: IQLHIP_ERR_INVALID / ValueError, every output as it was."""
    from iqlpref_amd import _lib, offline_bc
    assert str(select["n1_open/float32/raises"]) == "IndexError"  # (the reference fails here too, on its empty order)
    data = obe.selection_case("n1_open")
    rc, starts, lengths, returns, count = _raw_returns(_dev(data["rewards"]), _dev(data["terminals"], torch.uint8), 1000,
                                                       scale_rows=1000)
    assert rc == _lib.ERR_INVALID and count == -7
    assert (starts == -7).all() and (lengths == -7).all() and (returns == SENTINEL).all()
    with pytest.raises(ValueError, match="no complete trajectory"):
        offline_bc.select_best_trajectories(*[data[k] for k in offline_bc.ARRAYS], 1.0, 0.99, device=DEV)
    # a longer open run: the same
    rc, starts, _, returns, count = _raw_returns(torch.ones(2000, device=DEV), torch.zeros(2000, dtype=torch.uint8, device=DEV),
                                                 4096)
    assert rc == _lib.ERR_INVALID and count == -7 and (starts == -7).all() and (returns == SENTINEL).all()


def test_refusals_come_before_any_launch():
    from iqlpref_amd import _lib, offline_bc
    lib = _lib.load()
    rew, done = torch.ones(8, device=DEV), torch.ones(8, dtype=torch.uint8, device=DEV)
    assert _raw_returns(rew, done, 0)[0] == _lib.ERR_INVALID
    assert _raw_returns(rew, done, 4, n=0)[0] == _lib.ERR_INVALID
    rc, starts, _, _, count = _raw_returns(rew, done, (1 << 20) + 1, scale_rows=8)
    assert rc == _lib.ERR_UNSUPPORTED and count == -7 and (starts == -7).all()
    assert _raw_returns(rew, done, 1 << 20, scale_rows=8)[0] == 0  # (the edge itself: rows never reach the table's end)
    p, null = _lib.ptr, C.c_void_p(0)
    count = C.c_int64(0)
    i64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert lib.iqlhip_prep_trajectory_returns(null, p(done), 8, 4, p(rew), p(i64), p(i64), p(rew), C.byref(count),
                                              _lib.stream_ptr()) == _lib.ERR_INVALID
    dst = torch.full((9,), SENTINEL, device=DEV)
    args = lambda **kw: [kw.get("src", p(rew)), kw.get("n", 8), kw.get("width", 1), p(i64), p(i64), kw.get("n_traj", 8), p(i64),
                         p(i64), kw.get("m", 8), kw.get("total", 8), kw.get("dst", p(dst)), _lib.stream_ptr()]
    for bad in (dict(src=null), dict(dst=null), dict(n=0), dict(width=0), dict(n_traj=0), dict(n_traj=9), dict(m=0), dict(m=9),
                dict(total=7), dict(total=9)):
        assert lib.iqlhip_prep_gather_trajectories(*args(**bad)) == _lib.ERR_INVALID, bad
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()
    with pytest.raises(NotImplementedError):
        offline_bc.device_trajectory_returns(rew, done, 0.99, (1 << 20) + 1)
    # entries of `chosen` that name no trajectory, or rows that do not fit, are skipped on the device
    starts, lengths = _dev(np.asarray([0, 4], np.int64)), _dev(np.asarray([4, 4], np.int64))
    out = offline_bc.gather_trajectories(torch.arange(8, dtype=torch.float32, device=DEV), starts, lengths,
                                         _dev(np.asarray([1, 5], np.int64)), _dev(np.asarray([0, 4], np.int64)), 8,
                                         out=torch.full((8,), SENTINEL, device=DEV))
    np.testing.assert_array_equal(out.cpu().numpy(), [4, 5, 6, 7] + [SENTINEL] * 4)


@pytest.mark.parametrize("name", [n for n in sorted(obe.CASES) if n != "n1_open"])
def test_selection_is_the_references_and_the_hosts(select, name):
    """select_best_trajectories at every fraction of the case (max(1, ...) and 1.0 among them): the kept trajectory
    numbers and the five arrays equal the host restatement of this process; on the cases with distinct returns
    they equal the reference's arrays."""
    from iqlpref_amd import offline_bc
    n, max_len, term_rows, fracs, ordered = obe.CASES[name]
    g = mc.run_of(select, f"{name}/float32")
    data = obe.selection_case(name)
    for frac in fracs:
        sel, chosen = offline_bc.select_best_trajectories(*[data[k] for k in offline_bc.ARRAYS], frac, 0.99, max_len,
                                                          device=DEV)
        host = {k: v.copy() for k, v in data.items()}
        offline_bc.keep_best_trajectories(host, frac, 0.99, max_len)
        assert len(chosen) == max(1, int(frac * len(g["starts"])))
        total = int(g["lengths"][chosen].sum())
        for k in offline_bc.ARRAYS:
            got = sel[k].cpu().numpy()
            assert got.dtype == np.float32 and got.shape == host[k].shape and got.shape[0] == total, (k, got.shape)
            np.testing.assert_array_equal(bits(got), bits(host[k].astype(np.float32)), err_msg=f"{frac}/{k} (host)")
            if ordered:
                np.testing.assert_array_equal(bits(got), bits(g[f"{frac}/{k}"].astype(np.float32)), err_msg=f"{frac}/{k}")
        if ordered:
            np.testing.assert_array_equal(chosen, g[f"{frac}/top"])
        # dst is whole trajectories, one behind the other, in the order of `chosen`
        rows = sel["observations"].cpu().numpy()[:, 0].astype(np.int64)
        want = np.concatenate([np.arange(s, s + l) for s, l in zip(g["starts"][chosen], g["lengths"][chosen])])
        np.testing.assert_array_equal(rows, want)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", ["m7_n50", "chunks"])
def test_gather_at_every_width(select, name, width):
    """One array [n, width] gathered in the reference's order (its selected observations are the row numbers), into
    a sentinel-filled dst one row longer than needed: the rows are src[order], the extra row is untouched.  The
    source is also offset by one float so that no row lies on a 16-byte boundary."""
    from iqlpref_amd import offline_bc
    n, max_len, term_rows, fracs, ordered = obe.CASES[name]
    g = mc.run_of(select, f"{name}/float32")
    rng = np.random.default_rng(width)
    src = rng.standard_normal((n, width)).astype(np.float32)
    starts, lengths = _dev(g["starts"]), _dev(g["lengths"])
    for frac in fracs:
        order = g[f"{frac}/observations"][:, 0].astype(np.int64)
        top = g[f"{frac}/top"]
        L = g["lengths"][top]
        offsets = _dev(np.cumsum(L) - L)
        for shift in (0, 1):
            flat = torch.full((n * width + 4,), SENTINEL, device=DEV)
            flat[shift:shift + n * width] = _dev(src).reshape(-1)
            src_d = flat[shift:shift + n * width].view(n, width)
            dst = torch.full((len(order) + 1, width), SENTINEL, device=DEV)
            out = offline_bc.gather_trajectories(src_d, starts, lengths, _dev(top), offsets, len(order), out=dst)
            got = out.cpu().numpy()
            np.testing.assert_array_equal(bits(got[:-1]), bits(src[order]), err_msg=f"frac {frac} shift {shift}")
            assert (got[-1] == SENTINEL).all()
