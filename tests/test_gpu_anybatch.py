"""Any batch size >= 1 on the HIP path: a trainer created with batch_size = B runs on B rounded up to whole 16-row
slabs and counts only rows [0, B).  -m gpu.

Against the reference's own trajectories at B = 7, 17, 100, 250, 1000 (tuned step) and 50 (general step), against
the counted path that existed before (batch 112 with n_valid = 100), against the oracle where no reference exists,
seed groups against their members alone, the index streams, and the bounds of the caller's arrays."""
import numpy as np
import pytest
import torch

from oracle import philox
from tests import helpers
from tests import test_gpu_step as step
from tests.test_anybatch_host import TRAJ_ANYBATCH, as_its_kind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _state(tr):
    """Everything a step writes: parameters (with log_std), Adam moments, target."""
    torch.cuda.synchronize()
    return tr._params.clone(), tr._exp_avg.clone(), tr._exp_avg_sq.clone(), tr._target.clone()


def _same_state(a, b):
    for what, x, y in zip(("params", "exp_avg", "exp_avg_sq", "target"), _state(a), _state(b)):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name,kind", TRAJ_ANYBATCH)
def test_trajectory_parity_any_batch(gh, monkeypatch, name, kind, mode):
    """tests/test_gpu_step.py::test_trajectory_parity itself -- its checks, TOL, BF16_DELTA_*, MOMENT_TOL*, the
    kink-margin rule and the step_kind assertion -- on the reference's trajectories at batch sizes that are no
    multiple of 16, with the reference's indices [K, B] and (traj_b17_pen_drop) masks [K, 2, B, H]."""
    as_its_kind(monkeypatch, name, kind)
    assert helpers.load_traj(name, mode)[1]["batch"] % 16 != 0
    step.test_trajectory_parity(gh, name, mode)


def test_padded_batch_equals_the_counted_path(gh):
    """Tuned fp32: batch 100 = batch 112 stepped with n_valid = 100 on the same first 100 indices per step, bit for
    bit (what the 12 other rows gather differs: they contribute exactly nothing)."""
    d, hyper, data, nets = helpers.load_traj("traj_b100_antmaze", "fp32")
    K, B = hyper["k_steps"], hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    idx = torch.from_numpy(d["indices"]).to(gh.DEV)
    a = gh.make_trainer(hyper, nets, "fp32")
    la = a.train_steps(buf, K, B, indices=idx, graph_unroll=0)
    b = gh.make_trainer(hyper, nets, "fp32")
    idx112 = torch.cat([idx, idx.flip(1)[:, :12]], dim=1).contiguous()
    nv = torch.full((K,), B, dtype=torch.int32, device=gh.DEV)
    lb = b.train_steps(buf, K, 112, indices=idx112, n_valid=nv, graph_unroll=0)
    assert a.step_kind(B) == b.step_kind(112) == "tuned"
    assert torch.equal(la, lb)
    _same_state(a, b)
    # a caller's own count composes with the padding: clamp(n_valid, 1, B)
    c, e = gh.make_trainer(hyper, nets, "fp32"), gh.make_trainer(hyper, nets, "fp32")
    nv2 = torch.tensor([B, 37, 1, 500, 0, 99, 100, 64], dtype=torch.int32, device=gh.DEV)[:K]
    lc = c.train_steps(buf, K, B, indices=idx, n_valid=nv2, graph_unroll=0)
    le = e.train_steps(buf, K, 112, indices=idx112, n_valid=nv2.clamp(1, B), graph_unroll=0)
    assert torch.equal(lc, le)
    _same_state(c, e)


@pytest.mark.parametrize("S,A,H,B,det,E,mode", [
    (11, 3, 64, 1, False, 2, "fp32"), (11, 3, 64, 1, False, 2, "bf16"),          # one real row
    (17, 6, 128, 100, False, 4, "fp32"), (17, 6, 128, 100, False, 4, "bf16"),    # E = 4 critics
    (29, 8, 256, 1000, False, 4, "bf16")])  # the launch shape that picks the throughput kernels at batch 1024
def test_shapes_without_a_reference_vs_oracle(gh, S, A, H, B, det, E, mode):
    """tests/test_gpu_step.py's oracle check (losses and the gradient of every step, final parameters) with the
    on-device Philox indices: those of rows < B equal oracle/philox.py::sample_indices(seed, step, B, n_rows)."""
    step._shape_case(gh, S, A, H, 2, B, det, None, E, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graph_replay_equals_plain_launches(gh, mode):
    d, hyper, data, nets = helpers.load_traj("traj_b100_antmaze", mode)
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    idx = torch.from_numpy(d["indices"]).to(gh.DEV)
    runs = []
    for unroll in (0, 4):
        tr = gh.make_trainer(hyper, nets, mode, seed=5)
        losses = [tr.train_steps(buf, hyper["k_steps"], B, indices=idx, graph_unroll=unroll),  # injected indices
                  tr.train_steps(buf, 11, B, graph_unroll=unroll)]                                # Philox indices
        runs.append((torch.cat(losses), tr))
        assert (tr.launch_counts()[1] > 0) == (unroll > 0)
    assert torch.equal(runs[0][0], runs[1][0])
    _same_state(runs[0][1], runs[1][1])


@pytest.mark.parametrize("group_mode", ["group", "split", "streams", "general"])
def test_seed_group_members_equal_themselves_alone(gh, group_mode):
    """K = 3 trainers at batch 100 (tuned step; batch 50 at three hidden layers of 96 units for the general
    step's group launches): every member bit-identical to itself stepped alone."""
    import iqlpref_amd as ia
    name = "traj_b50_deep3_w96" if group_mode == "general" else "traj_b100_antmaze"
    d, hyper, data, nets = helpers.load_traj(name, "bf16")
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    seeds = (3, 4, 5)
    rng = np.random.default_rng(0)
    idx = [torch.from_numpy(rng.integers(0, hyper["n_rows"], (6, B))).to(gh.DEV) for _ in seeds]
    alone = [gh.make_trainer(hyper, nets, "bf16", seed=s) for s in seeds]
    want = [torch.cat([t.train_steps(buf, 13, B, graph_unroll=4), t.train_steps(buf, 6, B, indices=i, graph_unroll=0)])
            for t, i in zip(alone, idx)]
    group = ia.SeedGroup([gh.make_trainer(hyper, nets, "bf16", seed=s) for s in seeds], chunk=5, mode=group_mode)
    assert group.mode == group_mode
    got = group.train_steps(buf, 13, B, return_losses=True, graph_unroll=4)
    got2 = group.train_steps(buf, 6, B, return_losses=True, indices=idx, graph_unroll=0)
    group.synchronize()
    for w, g, g2, ta, tg in zip(want, got, got2, alone, group.trainers):
        assert torch.equal(w, torch.cat([g, g2]))
        _same_state(ta, tg)
    assert not torch.equal(want[0], want[1])
    group.close()


def test_index_streams_at_batch_100(gh):
    """ReplayBuffer.sample(100) gathers the rows of sample_indices(seed, call, 100, n); NumpyIndexStream at B = 100
    leaves numpy's generator where n host randint(0, hi, 100) calls leave it."""
    from iqlpref_amd import custom_offline as co
    d, hyper, data, nets = helpers.load_traj("traj_b100_antmaze", "fp32")
    buf = gh.make_buffer(hyper, data)
    torch.manual_seed(99)
    for call in range(2):
        b = buf.sample(100)
        ix = philox.sample_indices(99, call, 100, hyper["n_rows"])
        assert b[0].shape == (100, hyper["s_dim"])
        np.testing.assert_array_equal(b[0].cpu().numpy(), data["observations"][ix])
        np.testing.assert_array_equal(b[2].cpu().numpy()[:, 0], data["rewards"][ix])
    stream = co.NumpyIndexStream(gh.DEV)
    np.random.seed(5)
    before = np.random.get_state()
    got = stream.draw(4097, 9, 100)[0].cpu().numpy()
    after = np.random.get_state()
    np.random.set_state(before)
    want = np.stack([np.random.randint(0, 4097, size=100) for _ in range(9)])
    np.testing.assert_array_equal(got, want)
    ref = np.random.get_state()
    np.testing.assert_array_equal(after[1], ref[1])
    assert after[2:] == ref[2:]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_nothing_is_read_beyond_the_callers_arrays(gh, mode):
    """indices [K, 17] and dropout_keep [K, 2, 17, H] are the last bytes of their allocations' used part, each
    followed by a sentinel: the run is the same whatever the sentinels hold (indices there would point at other rows,
    mask bytes there would drop other units), and the sentinels are untouched."""
    d, hyper, data, nets = helpers.load_traj("traj_b17_pen_drop", mode)
    K, B, H = hyper["k_steps"], hyper["batch"], hyper["hidden"]
    buf = gh.make_buffer(hyper, data)
    keep = np.unpackbits(d["dropout_keep"], axis=-1)[..., :H]
    n_idx, n_keep, tail = K * B, keep.size, 4096
    runs = []
    for fill_idx, fill_keep in ((3, 0), (hyper["n_rows"] - 1, 1)):
        area_i = torch.full((n_idx + tail,), fill_idx, dtype=torch.int64, device=gh.DEV)
        area_k = torch.full((n_keep + tail,), fill_keep, dtype=torch.uint8, device=gh.DEV)
        area_i[:n_idx] = torch.from_numpy(d["indices"]).reshape(-1).to(gh.DEV)
        area_k[:n_keep] = torch.from_numpy(np.ascontiguousarray(keep)).reshape(-1).to(gh.DEV)
        tr = gh.make_trainer(hyper, nets, mode)
        losses = tr.train_steps(buf, K, B, indices=area_i[:n_idx].view(K, B),
                                dropout_keep=area_k[:n_keep].view(K, 2, B, H), graph_unroll=0)
        runs.append((losses, tr))
        torch.cuda.synchronize()
        assert (area_i[n_idx:] == fill_idx).all() and (area_k[n_keep:] == fill_keep).all()
    assert torch.equal(runs[0][0], runs[1][0])
    _same_state(runs[0][1], runs[1][1])
