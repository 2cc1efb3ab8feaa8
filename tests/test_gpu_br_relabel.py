"""iqlhip_posterior_choice and custom_offline_br.qlearning_dataset on the GPU.  -m gpu.

1. against tests/golden/br_relabel.npz (the reference's own posterior_sampler / qlearning_dataset on the
   CPU, make_br_fixture.py), predictions uploaded from the fixture: indices, final generator state, the
   single draw and the median bit for bit; the mean within (n - 1) 2^-23 max|preds[:, c]| per row (two
   fp32 summations of n terms in any order differ by no more);
2. against numpy itself (one randint(0, S, size=(N, n)) + take_along_axis) from start positions 0, 623,
   624 and mid-key, over many twists and chunk boundaries, at S = 2400 and at every samples-per-lane
   instantiation of the reduce kernel; same bounds;
3. qlearning_dataset end to end with the predictions made on the device: 2e-5 absolute (the bound
   tests/test_gpu_relabel.py holds the reward MLP to; first sample, mean and median are 1-Lipschitz in the
   sup norm of the predictions), generator state bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import br_env
from tests import custom_train_env as cte

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "br_relabel.npz")))


@pytest.fixture(scope="module")
def br():
    from iqlpref_amd import custom_offline_br
    return custom_offline_br


def _cases(golden, prefix):
    return sorted({k.split("/")[1] for k in golden if k.startswith(prefix + "/")})


def _start(seed, how):
    """A RandomState at a chosen pos: 624 (fresh seed), 0, 623, or mid-key."""
    rs = np.random.RandomState(seed)
    if how == "p0":
        st = rs.get_state()
        rs.set_state((st[0], st[1], 0, 0, 0.0))
    elif how == "p623":
        rs.randint(0, 2 ** 32, size=623)
    elif how == "mid":
        rs.randint(0, 2 ** 32, size=301)
    return rs


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    assert sa[2] == sb[2], f"pos {sa[2]} != {sb[2]}"
    np.testing.assert_array_equal(sa[1], sb[1])
    assert sa[3:] == sb[3:]


def _mean_bound(preds, n):
    return (n - 1) * 2.0 ** -23 * np.abs(preds).max(axis=0)


def _check_against(br, preds, n, host_rs, dev_rs, with_idx):
    """Both modes from generators in the same state; the host side is numpy's randint."""
    S, N = preds.shape
    dp = torch.from_numpy(preds).to(DEV)
    for mode in (br.MEAN, br.MEDIAN):
        h, d = np.random.RandomState(), np.random.RandomState()
        h.set_state(host_rs.get_state()), d.set_state(dev_rs.get_state())
        idx = h.randint(0, S, size=(N, n))
        samples = np.ascontiguousarray(np.take_along_axis(preds.T, idx, axis=1))
        got = br.posterior_choice(dp, n, mode, d, return_indices=with_idx)
        if with_idx:
            got, gidx = got
            np.testing.assert_array_equal(gidx.cpu().numpy().view(np.uint16), idx.astype(np.uint16))
        got = got.cpu().numpy()
        _same_state(d, h)
        if mode == br.MEDIAN:
            want = np.median(samples, axis=1)
            print(f"S={S} N={N} n={n} median: {np.count_nonzero(got != want)} rows differ")
            assert got.tobytes() == want.tobytes()
        elif n == 1:
            assert got.tobytes() == samples[:, 0].tobytes()
        else:
            err = np.abs(got.astype(np.float64) - samples.mean(1).astype(np.float64))
            bound = _mean_bound(preds, n)
            print(f"S={S} N={N} n={n} mean: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all()
    host_rs.set_state(h.get_state()), dev_rs.set_state(d.get_state())


# --------------------------------------------------------------------------- #
# 1. the reference's recorded output
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_idx", [True, False])
def test_kernel_reproduces_reference_sampler(golden, br, with_idx):
    for case in _cases(golden, "sampler"):
        S, n = (int(x[1:]) for x in case.split("_"))
        g = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"sampler/{case}/")}
        preds = golden[f"preds/{S}"]
        samples = g["samples"].reshape(preds.shape[1], n)
        dp = torch.from_numpy(preds).to(DEV)
        for mode in (br.MEAN, br.MEDIAN):
            np.random.seed(int(g["seed"]))
            got = br.posterior_choice(dp, n, mode, return_indices=with_idx)
            if with_idx:
                got, idx = got
                np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint16), g["idx"], err_msg=case)
            got = got.cpu().numpy()
            st = np.random.get_state()
            np.testing.assert_array_equal(st[1], g["np_key"], err_msg=case)
            assert st[2] == g["np_pos"], case
            if mode == br.MEDIAN:
                assert got.tobytes() == np.median(samples, axis=1).tobytes(), case
            elif n == 1:
                assert got.tobytes() == samples[:, 0].tobytes(), case
            else:
                err = np.abs(got.astype(np.float64) - samples.mean(1).astype(np.float64))
                assert (err <= _mean_bound(preds, n)).all(), case


def test_posterior_sampler_mirror(golden, br):
    """The materialising mirror of bref:179-186 on the global generator, has_gauss kept."""
    for case in ("S65_n7", "S129_n1"):
        S, n = (int(x[1:]) for x in case.split("_"))
        g = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"sampler/{case}/")}
        np.random.seed(int(g["seed"]))
        got = br.posterior_sampler(torch.from_numpy(golden[f"preds/{S}"]).to(DEV), n).cpu().numpy()
        assert got.shape == (golden[f"preds/{S}"].shape[1], n)
        assert got.tobytes() == g["samples"].reshape(got.shape).tobytes()
        assert np.random.get_state()[2] == g["np_pos"]
    rs = np.random.RandomState(5)
    rs.standard_normal()
    before = rs.get_state()
    br.posterior_sampler(torch.from_numpy(golden["preds/65"]).to(DEV), 3, rs)
    assert rs.get_state()[3] == 1 and rs.get_state()[4] == before[4]


# --------------------------------------------------------------------------- #
# 2. numpy itself
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("how", ["fresh", "p0", "p623", "mid"])
@pytest.mark.parametrize("with_idx", [True, False])
def test_start_positions(br, how, with_idx):
    rng = np.random.default_rng(3)
    for S, N, n in ((65, 1000, 1), (500, 777, 10), (129, 333, 7)):
        preds = rng.standard_normal((S, N)).astype(np.float32)
        _check_against(br, preds, n, _start(31, how), _start(31, how), with_idx)


def test_two_calls_are_one_stream(br):
    """Consecutive calls continue the stream: the generators stay in step over three rounds."""
    preds = np.random.default_rng(4).standard_normal((300, 4001)).astype(np.float32)
    h, d = _start(8, "mid"), _start(8, "mid")
    for n in (3, 1, 20):
        _check_against(br, preds, n, h, d, False)


@pytest.mark.parametrize("n", [64, 65, 128, 200, 500, 1023, 1024])
def test_every_lane_width(br, n):
    preds = np.random.default_rng(n).standard_normal((500, 1501)).astype(np.float32)
    _check_against(br, preds, n, _start(n, "fresh"), _start(n, "fresh"), n in (65, 1024))


def test_ties_and_small_posteriors(br):
    """Quantised predictions (many equal values in a row) and S = 2, 3."""
    rng = np.random.default_rng(9)
    for S, n in ((2, 9), (3, 10), (40, 100)):
        preds = (np.round(rng.standard_normal((S, 999)) * 2) / 2 + 0.0).astype(np.float32)  # (+ 0.0: no -0.0)
        _check_against(br, preds, n, _start(S, "fresh"), _start(S, "fresh"), True)


def test_many_twists_and_chunks(br):
    """N n >= 2^24 at S = 500: ~27k twists, 17 chunks through the 4-slot ring; N is odd."""
    S, N, n = 500, 167_773, 100
    assert N * n >= 2 ** 24
    preds = np.random.default_rng(1).standard_normal((S, N), dtype=np.float32)
    _check_against(br, preds, n, _start(77, "mid"), _start(77, "mid"), False)


def test_first_draw_across_chunks(br):
    """n_samps = 1 over more than one chunk (the direct gather kernel), with the indices."""
    S, N = 65, (1 << 21) + 12_345
    preds = np.random.default_rng(2).standard_normal((S, N), dtype=np.float32)
    _check_against(br, preds, 1, _start(78, "fresh"), _start(78, "fresh"), True)


@pytest.mark.parametrize("n", [37, 64])
def test_widest_posterior(br, n):
    """S = 2400, the cap: the tile narrows to 8 transitions."""
    S, N = 2400, 20_011
    preds = np.random.default_rng(n).standard_normal((S, N), dtype=np.float32)
    _check_against(br, preds, n, _start(79, "p623"), _start(79, "p623"), n == 37)


def test_small_workspace_gives_the_same(br):
    """A workspace below the query is used in smaller chunks; one that holds no 32-row chunk is refused."""
    from iqlpref_amd import _lib
    lib = _lib.load()
    S, N, n = 129, 5000, 10
    preds = np.random.default_rng(6).standard_normal((S, N)).astype(np.float32)
    dp = torch.from_numpy(preds).to(DEV)
    want_rs = _start(12, "fresh")
    want = br.posterior_choice(dp, n, br.MEDIAN, want_rs).cpu().numpy()
    state = torch.from_numpy(br.pack_np_state(_start(12, "fresh").get_state()).view(np.int32)).to(DEV)
    out = torch.empty(N, dtype=torch.float32, device=DEV)
    small = 4 * 64 * n * 2  # four slots of 64 rows
    ws = torch.empty(small, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.iqlhip_posterior_choice(_lib.ptr(state), _lib.ptr(dp), S, N, n, br.MEDIAN, _lib.ptr(out), None,
                                               _lib.ptr(ws), small, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()
        np.testing.assert_array_equal(state.cpu().numpy().view(np.uint32), br.pack_np_state(want_rs.get_state()))
        before = state.clone()
        with pytest.raises(ValueError):
            _lib.check(lib.iqlhip_posterior_choice(_lib.ptr(state), _lib.ptr(dp), S, N, n, br.MEDIAN, _lib.ptr(out),
                                                   None, _lib.ptr(ws), 4 * 31 * n * 2, _lib.stream_ptr()))
        bad = state.clone()
        bad[624] = 625
        with pytest.raises(ValueError):
            _lib.check(lib.iqlhip_posterior_choice(_lib.ptr(bad), _lib.ptr(dp), S, N, n, br.MEDIAN, _lib.ptr(out),
                                                   None, _lib.ptr(ws), small, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(before, state)


# --------------------------------------------------------------------------- #
# 3. qlearning_dataset end to end
# --------------------------------------------------------------------------- #
def test_qlearning_dataset_against_reference(golden, br):
    dataset = cte.MinariDataset(int(golden["data_seed"]), tuple(golden["lengths"]))
    env = dataset.recover_environment()
    sets = br_env.posterior_layers(int(golden["post_seed"]), 65, env.S, env.A, int(golden["hidden"]))
    map_set = br_env.posterior_layers(int(golden["map_seed"]), 1, env.S, env.A, int(golden["hidden"]))[0]
    model = br.PosteriorRewardNet(sets, map_set, "relu", DEV)
    preds = model.predictions(br_env.obs_act_of(dataset)).cpu().numpy()
    print("device predictions vs the stand-in's: max abs", np.abs(preds - golden["preds/65"]).max())
    np.testing.assert_allclose(preds, golden["preds/65"], rtol=0, atol=2e-5)
    for case in _cases(golden, "dataset"):
        rtype, n = case.split("_")
        rtype, n = int(rtype[4:]), (None if n == "nNone" else int(n[1:]))
        g = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"dataset/{case}/")}
        np.random.seed(int(g["seed"]))
        before = np.random.get_state()
        d = br.qlearning_dataset(dataset, model, rtype, n)
        assert set(d) == {"observations", "actions", "next_observations", "rewards", "terminals"}
        assert d["rewards"].dtype == np.float32 and d["rewards"].shape == g["rewards"].shape
        print(f"{case}: max abs reward error {np.abs(d['rewards'] - g['rewards']).max():.3g}")
        np.testing.assert_allclose(d["rewards"], g["rewards"], rtol=0, atol=2e-5, err_msg=case)
        for k in ("observations", "actions", "next_observations", "terminals"):
            assert tuple(g[f"{k}/shape"]) == d[k].shape
            np.testing.assert_allclose(np.asarray(d[k], np.float64).sum(), g[f"{k}/sum"], rtol=1e-6)
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], g["np_key"], err_msg=case)
        assert st[2] == g["np_pos"], case
        if rtype == 3:
            assert st[2] == before[2] and np.array_equal(st[1], before[1])
        # the same call on the reference's own predictions: types 0, 2, 3 and 7 to the bit
        np.random.seed(int(g["seed"]))
        rec = br_env.RecordedPosterior(golden["preds/65"], golden["map_preds"], DEV)
        r = br.qlearning_dataset(dataset, rec, rtype, n)["rewards"]
        if rtype == 1:
            np.testing.assert_allclose(r, g["rewards"], rtol=0, atol=float(_mean_bound(golden["preds/65"], n).max()))
        else:
            assert r.tobytes() == g["rewards"].tobytes(), case


def test_rng_argument_leaves_the_global_generator_alone(golden, br):
    dataset = cte.MinariDataset(int(golden["data_seed"]), tuple(golden["lengths"]))
    rec = br_env.RecordedPosterior(golden["preds/65"], None, DEV)
    np.random.seed(1)
    before = np.random.get_state()
    rs = np.random.RandomState(int(golden["dataset/type2_n7/seed"]))
    r = br.qlearning_dataset(dataset, rec, 2, 7, rng=rs)["rewards"]
    assert r.tobytes() == golden["dataset/type2_n7/rewards"].tobytes()
    assert rs.get_state()[2] == golden["dataset/type2_n7/np_pos"]
    after = np.random.get_state()
    assert after[2] == before[2] and np.array_equal(after[1], before[1])
    with pytest.raises(NotImplementedError):
        br.qlearning_dataset(dataset, br.PosteriorRewardNet(br_env.posterior_layers(1, 2, 45, 24), device=DEV), 3)
