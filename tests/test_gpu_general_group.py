"""Seed groups and hipGraph replay of the general layer-wise step (csrc/iql_deep.hip; ``SeedGroup(mode=
"general")``, ``train_steps(graph_unroll=U)`` on a general-step trainer).  The yardstick everywhere: the
same seeds stepped alone with plain launches (``graph_unroll=0``), which tests/test_gpu_step.py and
tests/test_gpu_reference_runs.py pin to the oracle and to reference runs.  Everything is compared bit for
bit: the losses of every step, parameters, target, Adam moments, total_it.  -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
STATE = ("_params", "_target", "_exp_avg", "_exp_avg_sq")


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def same_state(a, b, where=""):
    assert a.total_it == b.total_it, where
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{where}{name}"


def fresh(gh, *, S=29, A=8, H=96, NH=3, E=2, mode="bf16", seed=0, w_seed=0, det=False, dropout=None,
          max_steps=1000, beta=3.0, iql_tau=0.7, actor_lr=3e-4):
    """A trainer on networks drawn from torch.manual_seed(w_seed) (equal w_seed: equal initial weights)."""
    import iqlpref_amd as ia
    torch.manual_seed(w_seed)
    q = ia.TwinQ(S, A, hidden_dim=H, n_hidden=NH) if E == 2 else \
        ia.EnsembleQ(S, A, hidden_dim=H, n_hidden=NH, n_critics=E)
    v = ia.ValueFunction(S, hidden_dim=H, n_hidden=NH)
    cls = ia.DeterministicPolicy if det else ia.GaussianPolicy
    actor = cls(S, A, 1.0, hidden_dim=H, n_hidden=NH, dropout=dropout)
    q, v, actor = q.to(gh.DEV), v.to(gh.DEV), actor.to(gh.DEV)
    return ia.ImplicitQLearning(
        max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=actor_lr),
        q_network=q, q_optimizer=torch.optim.Adam(q.parameters(), lr=3e-4), v_network=v,
        v_optimizer=torch.optim.Adam(v.parameters(), lr=3e-4), iql_tau=iql_tau, beta=beta, max_steps=max_steps,
        device=gh.DEV, precision=mode, seed=seed)


def random_buffer(gh, n, S, A, seed=0):
    import iqlpref_amd as ia
    rng = np.random.default_rng(seed)
    buf = ia.ReplayBuffer(S, A, n + 7, gh.DEV)
    buf.load_d4rl_dataset(helpers.synth_dataset(rng, n, S, A))
    return buf


# ---- 1. group = solo on the reference-pinned shapes ---------------------------------------------------------- #
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", helpers.TRAJ_SHAPES)
def test_general_group_matches_solo_plain_launches(gh, name, mode):
    import iqlpref_amd as ia
    d, hyper, data, nets = helpers.load_traj(name, mode)
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    seeds = (3, 4, 5)
    alone = [gh.make_trainer(hyper, nets, mode, seed=s) for s in seeds]
    assert alone[0].step_kind(B) == "general"
    want = [t.train_steps(buf, 37, B, graph_unroll=0).cpu().numpy() for t in alone]
    group = ia.SeedGroup([gh.make_trainer(hyper, nets, mode, seed=s) for s in seeds], mode="general")
    assert group.mode == "general"
    got = group.train_steps(buf, 30, B, return_losses=True, graph_unroll=4)
    got2 = group.train_steps(buf, 7, B, return_losses=True, graph_unroll=0)
    group.synchronize()
    assert group.launch_counts() == (2 + 7, 7)  # 30 = 7 replays of 4 steps + 2 plain steps; then 7 plain
    for w, g, g2, ta, tg in zip(want, got, got2, alone, group.trainers):
        np.testing.assert_array_equal(w, torch.cat([g, g2]).cpu().numpy())
        same_state(ta, tg, f"{name}/{mode}: ")
        assert tg.launch_counts() == (0, 0)  # the members issued nothing themselves
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    group.close()


# ---- 2. a member alone between group calls and after close() --------------------------------------------------- #
def test_member_stepped_alone_between_group_calls_continues_the_run(gh):
    import iqlpref_amd as ia
    d, hyper, data, nets = helpers.load_traj("traj_deep3_w96", "bf16")
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    seeds = (7, 8, 9)
    alone = [gh.make_trainer(hyper, nets, "bf16", seed=s) for s in seeds]
    want = [t.train_steps(buf, 10 + 6 + 9 + 5, B, graph_unroll=0).cpu().numpy() if k == 1 else
            t.train_steps(buf, 10 + 9, B, graph_unroll=0).cpu().numpy() for k, t in enumerate(alone)]
    members = [gh.make_trainer(hyper, nets, "bf16", seed=s) for s in seeds]
    group = ia.SeedGroup(members, mode="general")
    a = group.train_steps(buf, 10, B, return_losses=True, graph_unroll=4)
    mid = members[1].train_steps(buf, 6, B, graph_unroll=3)  # alone, while a member (and with a graph of its own)
    # members 0 and 2 are at step 10, member 1 at 16: one group call steps them from where each stands
    b = group.train_steps(buf, 9, B, return_losses=True, graph_unroll=4)
    group.synchronize()
    group.close()
    tail = members[1].train_steps(buf, 5, B, graph_unroll=0)
    np.testing.assert_array_equal(want[1], torch.cat([a[1], mid, b[1], tail]).cpu().numpy())
    for k in (0, 2):
        np.testing.assert_array_equal(want[k], torch.cat([a[k], b[k]]).cpu().numpy())
    for ta, tg in zip(alone, members):
        same_state(ta, tg)
    assert members[1].total_it == 30 and members[0].total_it == 19


# ---- 3. injected indices / masks, own buffers ------------------------------------------------------------------ #
def test_general_group_injected_indices_masks_and_own_buffers(gh):
    import iqlpref_amd as ia
    d, hyper, data, nets = helpers.load_traj("traj_shallow1_w40_drop", "fp32")
    B, H, NH, n = hyper["batch"], hyper["hidden"], hyper["n_hidden"], 11
    assert hyper["dropout"] is not None
    rng = np.random.default_rng(5)
    idx = [torch.from_numpy(rng.integers(0, hyper["n_rows"], (n, B))).to(gh.DEV) for _ in range(3)]
    keep = [torch.from_numpy((rng.uniform(size=(n, NH, B, H)) >= hyper["dropout"]).astype(np.uint8)).to(gh.DEV)
            for _ in range(3)]
    bufs = [gh.make_buffer(hyper, data) for _ in range(3)]
    alone = [gh.make_trainer(hyper, nets, "fp32", seed=s) for s in (1, 2, 3)]
    want = [t.train_steps(bufs[k], n, B, indices=idx[k], dropout_keep=keep[k] if k != 1 else None,
                          graph_unroll=0).cpu().numpy() for k, t in enumerate(alone)]
    members = [gh.make_trainer(hyper, nets, "fp32", seed=s) for s in (1, 2, 3)]
    group = ia.SeedGroup(members, mode="general")
    got = group.train_steps(bufs, n, B, indices=idx, dropout_keep=[keep[0], None, keep[2]], return_losses=True,
                            graph_unroll=4)
    group.synchronize()
    for k in range(3):
        np.testing.assert_array_equal(want[k], got[k].cpu().numpy())
        same_state(alone[k], members[k])
    assert not np.array_equal(want[0], want[2])
    # a mask built for another depth / width / step count is refused before it reaches the device
    for bad in (keep[0][:, :, :, : H - 1], keep[0][: n - 1], torch.cat([keep[0], keep[0]], dim=1)):
        with pytest.raises(ValueError, match="dropout_keep"):
            group.train_steps(bufs, n, B, dropout_keep=[bad, None, None])
        with pytest.raises(ValueError, match="dropout_keep"):
            alone[0].train_steps(bufs[0], n, B, dropout_keep=bad)
    assert members[0].total_it == n
    group.close()


# ---- 4. solo graph replay -------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_solo_graph_replay_matches_plain_launches(gh, mode):
    d, hyper, data, nets = helpers.load_traj("traj_deep3_w96", mode)
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    plain, graph = gh.make_trainer(hyper, nets, mode, seed=11), gh.make_trainer(hyper, nets, mode, seed=11)
    assert graph.launch_counts() == (0, 0)
    want = plain.train_steps(buf, 23 + 14, B, graph_unroll=0).cpu().numpy()
    assert plain.launch_counts() == (37, 0)
    got = graph.train_steps(buf, 23, B, graph_unroll=5)
    assert graph.launch_counts() == (3, 4)
    got2 = graph.train_steps(buf, 14, B, graph_unroll=3)  # another unroll: captured again
    assert graph.launch_counts() == (3 + 2, 4 + 4)
    np.testing.assert_array_equal(want, torch.cat([got, got2]).cpu().numpy())
    same_state(plain, graph)


# ---- 5. launch geometries that differ between a group and a solo launch ------------------------------------------ #
GEOMETRIES = {
    # 16 slabs x 7 evaluations = 112 work-groups alone (512 threads), 224 / 128 for two: forward stays, ...
    "w512_d3_k4": dict(K=4, H=512, NH=3, B=256),        # ... four members: 448 / 256 -> forward 256 threads
    "e4_b1024_k2": dict(K=2, H=256, NH=3, B=1024, E=4),  # wide update tiles (tq = 4)
    "w1000_d2_k2": dict(K=2, H=1000, NH=2, B=256),       # not a multiple of 64, the default depth
    "w40_d1_k16": dict(K=16, H=40, NH=1, B=256),         # the largest group
    "d6_k2": dict(K=2, H=128, NH=6, B=256),              # the deepest network
    "w512_d3_k2": dict(K=2, H=512, NH=3, B=256),
    # the thread count a group picks against the one a member runs alone, in both precisions and at the most
    # likely real shape: 3 x 256 alone 112 / 64 work-groups (512 threads), five members 560 / 320 (256 threads)
    "w512_d3_k4_fp32": dict(K=4, H=512, NH=3, B=256, mode="fp32"),
    "w256_d3_k5": dict(K=5, H=256, NH=3, B=256),
    "w256_d3_k5_fp32": dict(K=5, H=256, NH=3, B=256, mode="fp32"),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_group_launch_geometry_does_not_change_a_members_bits(gh, name):
    import iqlpref_amd as ia
    g = GEOMETRIES[name]
    K, B, S, A = g["K"], g["B"], 29, 8
    kw = dict(S=S, A=A, H=g["H"], NH=g["NH"], E=g.get("E", 2), mode=g.get("mode", "bf16"))
    buf = random_buffer(gh, 5000, S, A, seed=3)
    alone = [fresh(gh, seed=20 + k, w_seed=k, **kw) for k in range(K)]
    assert alone[0].step_kind(B) == "general"
    want = [t.train_steps(buf, 12, B, graph_unroll=0).cpu().numpy() for t in alone]
    members = [fresh(gh, seed=20 + k, w_seed=k, **kw) for k in range(K)]
    group = ia.SeedGroup(members, mode="general")
    got = group.train_steps(buf, 12, B, return_losses=True, graph_unroll=5)
    group.synchronize()
    assert group.launch_counts() == (2, 2)
    for k in range(K):
        assert np.isfinite(want[k]).all()
        np.testing.assert_array_equal(want[k], got[k].cpu().numpy())
        same_state(alone[k], members[k], f"{name}[{k}]: ")
    assert not np.array_equal(want[0], want[1])
    group.close()


# ---- 6. members of different configs ------------------------------------------------------------------------------ #
def test_members_of_different_configs_in_one_general_group(gh):
    import iqlpref_amd as ia
    S, A, B = 45, 24, 64
    cfgs = [dict(beta=3.0, iql_tau=0.7, actor_lr=3e-4, dropout=0.1), dict(beta=10.0, iql_tau=0.9, actor_lr=1e-3, dropout=0.2),
            dict(beta=3.0, iql_tau=0.9, actor_lr=1e-3, dropout=0.1), dict(beta=10.0, iql_tau=0.7, actor_lr=3e-4, dropout=0.2)]
    buf = random_buffer(gh, 3000, S, A, seed=4)
    mk = lambda k, c: fresh(gh, S=S, A=A, H=72, NH=4, seed=30 + k, w_seed=9, max_steps=50, **c)
    alone = [mk(k, c) for k, c in enumerate(cfgs)]
    want = [t.train_steps(buf, 21, B, graph_unroll=0).cpu().numpy() for t in alone]
    members = [mk(k, c) for k, c in enumerate(cfgs)]
    group = ia.SeedGroup(members, mode="general")
    got = group.train_steps(buf, 21, B, return_losses=True, graph_unroll=6)
    group.synchronize()
    for k in range(4):
        np.testing.assert_array_equal(want[k], got[k].cpu().numpy())
        same_state(alone[k], members[k])
    assert not np.array_equal(want[0], want[1])
    group.close()


def test_sweep_grid_on_the_general_step_equals_runs_trained_one_by_one(gh, tmp_path):
    import iqlpref_amd as ia
    from iqlpref_amd import sweep as sw
    from tests import fake_envs
    from tests.test_gpu_sweep import same, synth
    env_name = "antmaze-medium-diverse-v2"
    env = fake_envs.FakeGymEnv(env_name)
    S, A = fake_envs.DIMS[env_name]
    data = synth(3000, S, A)
    spec = {"method": "grid", "parameters": {
        "env": {"value": env_name}, "hidden_dim": {"value": 96}, "n_hidden": {"value": 3}, "batch_size": {"value": 64},
        "max_timesteps": {"value": 40}, "log_freq": {"value": 10}, "eval_freq": {"value": 20},
        "buffer_size": {"value": 10_000_000}, "device": {"value": gh.DEV},
        "beta": {"values": [3.0, 10.0]}, "iql_tau": {"values": [0.7, 0.9]}}}

    def run(sub, **kw):
        cfgs = sw.expand_sweep(spec, checkpoints_path=str(tmp_path / sub))
        assert len(cfgs) == 4 and sw.plan_batches(cfgs, [(S, A)] * 4, 8) == [[0, 1, 2, 3]]
        logs = []
        evaluate = lambda actor, t: (np.array([float(actor.net.linears()[3].weight.detach().double().sum()), 1.0]), [t])
        trs = ia.train_runs(cfgs, env, {k: np.array(v) for k, v in data.items()},
                            logger=lambda d, step: logs.append((step, dict(d))), evaluate=evaluate, **kw)
        return cfgs, trs, logs

    cfg_g, tr_g, log_g = run("general", group_mode="general")
    cfg_s, tr_s, log_s = run("one_by_one", runs_per_gpu=1)
    assert all(t.step_kind(64) == "general" for t in tr_g)
    by_run = lambda logs, i: [(st, d) for st, d in logs if d["run"] == i]
    for i in range(4):
        assert by_run(log_g, i) == by_run(log_s, i) and len(by_run(log_g, i)) == 4 + 2
        same_state(tr_g[i], tr_s[i])
        for f in ("checkpoint_19.pt", "checkpoint_39.pt"):
            same(torch.load(os.path.join(cfg_g[i].checkpoints_path, f), weights_only=True),
                 torch.load(os.path.join(cfg_s[i].checkpoints_path, f), weights_only=True), f)
    assert not torch.equal(tr_g[0]._params, tr_g[1]._params)


# ---- 7. refusals --------------------------------------------------------------------------------------------------- #
def test_general_groups_refuse_what_they_cannot_run(gh):
    import iqlpref_amd as ia
    B = 64
    buf = random_buffer(gh, 1000, 29, 8)
    tuned = [fresh(gh, H=64, NH=2, seed=k) for k in range(2)]
    gen3 = [fresh(gh, H=96, NH=3, seed=k) for k in range(2)]
    gen4 = fresh(gh, H=96, NH=4)
    forced = bool(os.environ.get("IQLHIP_FORCE_GENERAL"))
    if not forced:
        with pytest.raises(ValueError, match="tuned step"):  # decided by step_kind() once the handles exist
            ia.SeedGroup(tuned, mode="general").train_steps(buf, 2, B)
    with pytest.raises(ValueError):
        ia.SeedGroup([gen3[0], gen4], mode="general")
    with pytest.raises(ValueError, match="tuned step"):
        ia.SeedGroup(gen3, mode="group")
    with pytest.raises(ValueError):
        ia.SeedGroup([fresh(gh, H=96, NH=3, seed=k) for k in range(17)], mode="general")
    assert ia.SeedGroup(gen3).mode == "streams"  # the default has not moved
    # the library itself: tuned + general members, and members of different depth
    if not forced:
        lib, C = ia._lib.load(), __import__("ctypes")
        hs = []
        for t in (tuned[0], gen3[0], gen4):
            t._ensure_handle(B)
            hs.append(t._handle.value)
        for pair in ((hs[0], hs[1]), (hs[1], hs[2])):
            g = C.c_void_p()
            assert lib.iqlhip_group_create(C.byref(g), (C.c_void_p * 2)(*pair), 2) == ia._lib.ERR_INVALID


# ---- 8. the cosine schedule across graph boundaries, remainders and calls ------------------------------------------- #
def test_cosine_schedule_across_graphs_remainders_and_calls(gh):
    import iqlpref_amd as ia
    B, S, A = 64, 29, 8
    buf = random_buffer(gh, 2000, S, A, seed=6)
    mk = lambda k: fresh(gh, S=S, A=A, H=96, NH=3, seed=40 + k, w_seed=k, max_steps=60)
    alone, members = [mk(k) for k in range(2)], [mk(k) for k in range(2)]
    want = [t.train_steps(buf, 60, B, graph_unroll=0).cpu().numpy() for t in alone]
    group = ia.SeedGroup(members, mode="general")
    a = group.train_steps(buf, 40, B, return_losses=True, graph_unroll=8)
    b = group.train_steps(buf, 20, B, return_losses=True, graph_unroll=8)
    group.synchronize()
    assert group.launch_counts() == (4, 5 + 2)
    for k in range(2):
        np.testing.assert_array_equal(want[k], torch.cat([a[k], b[k]]).cpu().numpy())
        same_state(alone[k], members[k])
        assert members[k].actor_optimizer.param_groups[0]["lr"] == alone[k].actor_optimizer.param_groups[0]["lr"]
    group.close()
