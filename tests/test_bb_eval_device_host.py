"""The host side of the BB flavour's device evaluation (custom_offline_bb.bb_run_eval_device).  No GPU.

1. the drift table and the rewind: ONE rng.normal call of shape (L, n_obs) draws the values of L calls of
   size n_obs and leaves the generator in the same state, so the device path can draw the whole
   [max_horizon, n_obs] table up front and afterwards put the generator where the numpy loop leaves it;
2. the episode set-up exists once: bb_run_eval_IQL draws it through _episode_setup;
3. what is refused before any device is touched.
"""
import numpy as np
import pytest

from tests import bb_env

H, N_OBS = 50, 100


@pytest.fixture(scope="module")
def bb():
    from iqlpref_amd import custom_offline_bb
    return custom_offline_bb


def test_device_evaluation_is_there(bb):
    from iqlpref_amd.custom_offline_bb import DeviceEpisode, bb_run_eval_device  # noqa: F401
    assert callable(bb_run_eval_device)


def _same_state(a, b):
    assert a["bit_generator"] == b["bit_generator"] and a["state"] == b["state"]
    assert a["has_uint32"] == b["has_uint32"] and a["uinteger"] == b["uinteger"]


@pytest.mark.parametrize("length", [1, 37, H])
def test_table_draw_and_rewind_equal_the_per_step_draws(bb, length):
    ms = bb_env.MOVE_STATS
    step_rng = np.random.default_rng(11)
    bb._episode_setup(step_rng, 181)
    per_step = np.stack([step_rng.normal(ms[2], ms[3], N_OBS) for _ in range(length)])

    rng = np.random.default_rng(11)
    bb._episode_setup(rng, 181)
    saved = rng.bit_generator.state
    table = rng.normal(ms[2], ms[3], (H, N_OBS))
    np.testing.assert_array_equal(table[:length], per_step)
    bb._rewind_drift(rng, saved, ms, length, N_OBS)
    _same_state(rng.bit_generator.state, step_rng.bit_generator.state)
    assert rng.random() == step_rng.random()


def test_rewind_of_no_step_restores_the_saved_state(bb):
    rng = np.random.default_rng(3)
    saved = rng.bit_generator.state
    rng.normal(0.0, 1.0, (H, N_OBS))
    bb._rewind_drift(rng, saved, bb_env.MOVE_STATS, 0, N_OBS)
    _same_state(rng.bit_generator.state, saved)


def test_numpy_simulator_draws_its_setup_through_the_helper(bb, monkeypatch):
    seen = []
    real = bb._episode_setup

    def spy(rng, days):
        out = real(rng, days)
        seen.append(out)
        return out

    monkeypatch.setattr(bb, "_episode_setup", spy)
    actor = bb_env.ReplayActor(np.tile(np.array([[0.5, 10.0]], np.float32), (6, 1)))
    bb.bb_run_eval_IQL(actor, 2, bb_env.numpy_reward, bb_env.MOVE_STATS, max_horizon=3, seed=5)
    assert len(seen) == 2
    n_obs, ox, oy, oang, px, py, goal, tail = seen[0]
    assert n_obs in (50, 100, 150) and ox.shape == oy.shape == oang.shape == (n_obs,) and len(tail) == 4
    np.testing.assert_array_equal(actor.states[0][:2], [px, py])
    np.testing.assert_array_equal(actor.states[0][20:22], goal)
    # the helper alone on a fresh generator: the same first episode
    again = real(np.random.default_rng(5), 181)
    np.testing.assert_array_equal(again[1], ox)
    assert again[4:7] == (px, py, goal)


def test_train_refuses_an_unknown_eval_on_before_any_device(bb):
    with pytest.raises(ValueError, match="eval_on"):
        bb.train(bb.TrainConfig(), dataset=bb_env.synth_dataset(), reward_model=bb_env.numpy_reward,
                 move_stats=bb_env.MOVE_STATS, device="cuda:0", eval_on="bogus")


def test_plain_callable_is_refused_with_the_host_path_named(bb):
    with pytest.raises(TypeError, match="bb_run_eval_IQL"):
        bb.bb_run_eval_device(bb_env.ReplayActor([]), 1, bb_env.numpy_reward, bb_env.MOVE_STATS)
    with pytest.raises(TypeError, match="bb_run_eval_IQL"):
        bb.train(bb.TrainConfig(), dataset=bb_env.synth_dataset(), reward_model=bb_env.numpy_reward,
                 move_stats=bb_env.MOVE_STATS, device="cuda:0", eval_on="device")
