"""Any batch size >= 1, the parts that need no GPU: the oracle against the reference's trajectories at batch
sizes that are no multiple of 16 (tests/golden/make_anybatch_fixture.py), the configuration check of the C-ABI, the
byte model, and the host logic of the sweep expansion and the block-epoch sampler at such sizes."""
import ctypes

import numpy as np
import pytest

from tests import helpers
from tests.test_oracle_golden import test_trajectory_matches_reference as _oracle_vs_reference

# (name, the step that runs it)
TRAJ_ANYBATCH = [("traj_b7_cheetah_det", "tuned"), ("traj_b17_pen_drop", "tuned"), ("traj_b100_antmaze", "tuned"),
                 ("traj_b250_h256", "tuned"), ("traj_b1000_h256", "tuned"), ("traj_b50_deep3_w96", "general")]


def as_its_kind(monkeypatch, name, kind):
    """The checks this file borrows tell the general step's trajectories by helpers.TRAJ_SHAPES."""
    if kind == "general":
        monkeypatch.setattr(helpers, "TRAJ_SHAPES", helpers.TRAJ_SHAPES + [name])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name,kind", TRAJ_ANYBATCH)
def test_oracle_matches_reference_at_any_batch(monkeypatch, name, kind, mode):
    """The comparison and the bounds of tests/test_oracle_golden.py, on the new trajectories: the reference and
    the oracle alone stay inside every cap the GPU test reuses."""
    as_its_kind(monkeypatch, name, kind)
    d, hyper, _, _ = helpers.load_traj(name, mode)
    assert hyper["batch"] % 16 != 0 and d["indices"].shape == (hyper["k_steps"], hyper["batch"])
    if hyper["dropout"] is not None:  # the reference's masks, batch % 4 != 0
        assert d["dropout_keep"].shape[:3] == (hyper["k_steps"], hyper["n_hidden"], hyper["batch"])
    _oracle_vs_reference(name, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name,kind", TRAJ_ANYBATCH)
def test_oracle_alone_stays_inside_the_gpu_caps(name, kind, mode):
    """The "all but x % of entries" caps that tests/test_gpu_step.py::test_trajectory_parity puts on the HIP step
    against the oracle, put on the oracle against the reference's own arrays: the Adam moments (all but 0.5 % of a
    tensor within MOMENT_TOL*) and the fp32 parameters (all but 1 % within TOL's bound; 0.1 % on the general
    step).  A fixture at which the oracle itself leaves the reference by more cannot referee a third
    implementation: its seed is changed (tests/golden/make_anybatch_fixture.py), never the cap."""
    from oracle import iql_oracle as orc
    from tests import test_gpu_step as step
    d, hyper, data, nets = helpers.load_traj(name, mode)
    o = helpers.make_oracle(hyper, nets, mode)
    for t in range(hyper["k_steps"]):
        o.train(orc.gather_batch(data, d["indices"][t]), helpers.keep_masks(d, hyper, t))
    t1, t2 = step.MOMENT_TOL_DEEP if (mode == "bf16" and kind == "general") else step.MOMENT_TOL[mode]
    for which, net in (("q", "q_adam"), ("v", "v_adam"), ("actor", "actor_adam")):
        for k in o.m[which]:
            for arr, key, tol in ((o.m[which][k], "exp_avg", t1), (o.v2[which][k], "exp_avg_sq", t2)):
                want, got = helpers.golden_param(d, f"final/{net}/{k}/{key}", arr)
                if want is None:
                    continue
                err = np.abs(got - want.reshape(got.shape)) / (np.abs(want).max() + 1e-30)
                assert (err > tol).mean() <= 5e-3, (which, k, key, float((err > tol).mean()), float(err.max()))
    if mode == "fp32":
        cap = 1e-3 if kind == "general" else 1e-2
        for net, pd in (("qf", o.qf), ("vf", o.vf), ("actor", o.actor), ("q_target", o.q_target)):
            for k, v in pd.items():
                want, got = helpers.golden_param(d, f"final/{net}/{k}", v)
                diff = np.abs(got - want.reshape(got.shape))
                assert (diff > step.TOL["fp32"]["pg"]).mean() < cap, (net, k, float(diff.max()))


def _cfg(batch, hidden=256, n_hidden=0):
    from iqlpref_amd import _lib
    c = _lib.TrainerConfig()
    c.state_dim, c.action_dim, c.hidden_dim, c.batch_size, c.n_hidden = 29, 8, hidden, batch, n_hidden
    c.precision, c.cosine_t_max, c.dropout_p = 1, 10, -1.0
    return c


def test_arena_layout_takes_any_positive_batch():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    lib = _lib.load()
    offs = (ctypes.c_int64 * _lib.N_TENSORS)()
    n_p, n_t = ctypes.c_int64(), ctypes.c_int64()
    want = None
    for batch in (256, 100, 7, 1):
        c = _cfg(batch)
        assert lib.iqlhip_arena_layout(ctypes.byref(c), ctypes.byref(offs), ctypes.byref(n_p), ctypes.byref(n_t)) == 0, \
            (batch, lib.iqlhip_last_error())
        got = (list(offs), n_p.value, n_t.value)  # the arenas do not depend on the batch
        want = want or got
        assert got == want
    for batch in (100, 7, 1):  # the general step's shapes too
        c = _cfg(batch, hidden=96, n_hidden=3)
        assert lib.iqlhip_arena_layout(ctypes.byref(c), None, None, None) == 0, (batch, lib.iqlhip_last_error())
    for batch in (0, -16):
        c = _cfg(batch)
        assert lib.iqlhip_arena_layout(ctypes.byref(c), None, None, None) != 0
        assert b"batch_size" in lib.iqlhip_last_error()


def test_step_cost_counts_the_real_rows():
    from iqlpref_amd import _lib
    lib = _lib.load()
    S, A, H = 29, 8, 256
    sizes = []
    for in_dim, out in ((S + A, 1), (S + A, 1), (S, 1), (S, A)):
        sizes += [H * in_dim, H, H * H, H, out * H, out]
    sizes.append(A)
    b = ctypes.c_double()
    c = _cfg(100)
    assert lib.iqlhip_step_cost(ctypes.byref(c), ctypes.byref(b), None) == 0
    assert b.value == 4 * 100 * (2 * S + A + 2) + 32 * sum(sizes) + 8 * sum(sizes[:12])


def test_sweep_batch_axis_makes_one_launch_batch_per_size():
    import iqlpref_amd.sweep as sw
    cfgs = sw.expand_sweep({"method": "grid", "parameters": {"batch_size": {"values": [100, 256]},
                                                             "seed": {"values": [0, 1]}}})
    assert sorted(c.batch_size for c in cfgs) == [100, 100, 256, 256]
    dims = (17, 6)
    keys = {sw.shape_key(c, dims) for c in cfgs}
    assert len(keys) == 2  # members of a launch share the batch size


def test_block_epoch_sampler_with_a_batch_that_divides_nothing():
    import torch
    from iqlpref_amd.custom_offline_bb import BlockEpochSampler
    N, B = 250, 100
    s = BlockEpochSampler(N, B, generator=torch.Generator().manual_seed(3))
    assert len(s) == 3 and s.n_blocks == 2 and s.tail == 50
    idx, valid = s.host_indices(0, 6)  # two epochs
    assert idx.shape == (6, B) and list(valid) == [B, B, 50] * 2
    for ep in range(2):
        rows = np.concatenate([idx[3 * ep + t, :valid[3 * ep + t]] for t in range(3)])
        assert sorted(rows.tolist()) == list(range(N))  # every row once an epoch
        np.testing.assert_array_equal(idx[3 * ep + 2, :50], np.arange(200, 250))  # the rows left over, in order
    assert idx.min() >= 0 and idx.max() < N  # the slots beyond the count too
