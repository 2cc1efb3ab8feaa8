"""Host logic of iqlpref_amd.finetune against tests/golden/finetune_run.npz (two runs of the reference's
algorithms/finetune/iql.py:train on the CPU, make_finetune_fixture.py).  No GPU."""
import dataclasses
import math
import os

import numpy as np
import pytest

from iqlpref_amd import finetune as ft

RUNS = ("gauss", "det")

# |CosineAnnealingLR's recursion - closed form| in float64 over the fixture's 90 steps at T_max = 30, base 3e-4,
# measured on the CPU with torch's own scheduler (test_cosine_bound_is_what_the_schedulers_differ_by measures it
# again): 6.02e-18.  Four times that, because the recursion's rounding depends on the path taken.
COSINE_MEASURED = 6.02e-18
COSINE_BOUND = 4 * COSINE_MEASURED


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "finetune_run.npz")))


def _run(golden, name):
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}


def test_config_defaults_match_the_reference(golden):
    d = ft.TrainConfig()
    keys = [f.name for f in dataclasses.fields(ft.TrainConfig) if f.name not in ("name", "checkpoints_path")]
    assert sorted(keys) == golden["defaults/keys"].tolist()
    for k, want in zip(golden["defaults/keys"].tolist(), golden["defaults/values"].tolist()):
        assert repr(getattr(d, k)) == want, k
    assert d.checkpoints_path is None


@pytest.mark.parametrize("name", RUNS)
def test_config_name_and_path(name, golden, tmp_path):
    g = _run(golden, name)
    c = ft.TrainConfig(env=str(g["env_name"]), checkpoints_path=str(tmp_path))
    assert c.name[:-8] == str(g["config_name_prefix"]) and len(c.name) == len(str(g["config_name_prefix"])) + 8
    assert os.path.relpath(c.checkpoints_path, str(tmp_path)) == c.name
    assert c.name[:-8] == str(g["config_path_tail"])
    assert ft.TrainConfig(env=str(g["env_name"])).name != c.name  # a fresh uuid each time


@pytest.mark.parametrize("name", RUNS)
def test_modify_reward_matches_the_recording(name, golden):
    g = _run(golden, name)
    data = {k[len("dataset/"):]: v.copy() for k, v in g.items() if k.startswith("dataset/")}
    d = ft.modify_reward(data, str(g["env_name"]))
    assert sorted(d) == g["reward_mod_keys"].tolist()
    assert [d[k] for k in sorted(d)] == g["reward_mod_values"].tolist()
    np.testing.assert_array_equal(data["rewards"], g["dataset_rewards_modified"])
    # the online rewards: the environment's raw ones through modify_reward_online are the recorded additions
    raw = g["env/reward"][g["env/kind"] == 1]
    got = [ft.modify_reward_online(float(r), str(g["env_name"]), **d) for r in raw]
    assert got == g["added_reward"].tolist()


def test_modify_reward_leaves_other_environments_alone():
    data = {"rewards": np.arange(4, dtype=np.float32), "terminals": np.zeros(4)}
    assert ft.modify_reward(data, "pen-human-v1") == {}
    np.testing.assert_array_equal(data["rewards"], np.arange(4, dtype=np.float32))
    assert ft.modify_reward_online(0.25, "pen-human-v1") == 0.25


def test_is_goal_reached():
    assert ft.is_goal_reached(-1.0, {"goal_achieved": True}) is True
    assert ft.is_goal_reached(1.0, {"goal_achieved": False}) is False
    assert ft.is_goal_reached(0.5, {}) and not ft.is_goal_reached(0.0, {})


@pytest.mark.parametrize("name", RUNS)
def test_ring_arithmetic_over_a_wrap(name, golden):
    g = _run(golden, name)
    cap, n0 = int(golden["common/buffer_size"]), int(golden["common/n_dataset"])
    pointer, size = n0, n0  # fref:150-151
    seen = []
    for _ in range(int(golden["common/online_iterations"])):
        seen.append(pointer)
        pointer, size = ft.ring_advance(pointer, size, 1, cap)
    assert (pointer, size) == (int(g["buf_pointer"]), int(g["buf_size"]))
    assert max(seen) == cap - 1 and seen[cap - n0] == 0  # it wrapped
    assert ft.ring_advance(n0, n0, 60, cap) == (pointer, size)  # n at once = n times one
    assert ft.ring_advance(0, 1, 1, 1) == (0, 1) and ft.ring_advance(37, 37, 7, 40) == (4, 40)


@pytest.mark.parametrize("name", RUNS)
def test_bound_schedule(name, golden):
    g = _run(golden, name)
    cap, n0, n_on = int(golden["common/buffer_size"]), int(golden["common/n_dataset"]), 60
    hi = ft.bound_schedule(min(n0 + 1, cap), cap, n_on)
    assert hi.tolist() == [min(n0 + j + 1, cap) for j in range(n_on)]
    assert hi[-1] == cap and (hi == cap).sum() == n_on - (cap - n0) + 1  # saturates at capacity
    idx = g["idx"]
    assert (idx[:30] < n0).all() and (idx[30:] < hi[:, None]).all() and (idx >= 0).all()
    assert ft.bound_schedule(5, 5, 4).tolist() == [5] * 4 and ft.bound_schedule(3, 9, 3, growth=0).tolist() == [3] * 3
    assert ft.bound_schedule(1, 3, 5).tolist() == [1, 2, 3, 3, 3]


def test_cosine_bound_is_what_the_schedulers_differ_by():
    import torch
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=3e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 30)
    worst = 0.0
    for t in range(90):
        worst = max(worst, abs(opt.param_groups[0]["lr"] - ft.cosine_rate(3e-4, t, 30)))
        opt.step()
        sch.step()
    print(f"recursion vs closed form over 90 steps: {worst:.3e}")
    assert worst <= COSINE_BOUND


@pytest.mark.parametrize("name", RUNS)
def test_cosine_rate_beyond_t_max(name, golden):
    g = _run(golden, name)
    t_max = int(golden["common/offline_iterations"])
    got = np.asarray([ft.cosine_rate(3e-4, t, t_max) for t in range(len(g["actor_lr"]))])
    err = np.abs(got - g["actor_lr"]).max()
    print(f"{name}: closed form vs recorded rates: {err:.3e}")
    assert err <= COSINE_BOUND
    assert g["actor_lr"][t_max] == 0.0 and g["actor_lr"][t_max + 1] > 0
    assert abs(g["actor_lr"][2 * t_max] - 3e-4) <= COSINE_BOUND  # back at the base rate after a whole period
    assert math.isclose(got[t_max + 5], got[t_max - 5], rel_tol=1e-12)  # it climbs back as it fell
