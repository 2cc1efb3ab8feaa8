"""The host side of the BB flavour (iqlpref_amd/custom_offline_bb.py) against
tests/golden/bb_train_run.npz, a run of the reference's own iql_bb.py (make_bb_fixture.py).  No GPU.

1. BlockEpochSampler: host indices and valid counts = the reference loader's batches, 12 steps;
2. BBDataset: statistics bit for bit, the transitions handed to the buffer, the refusals;
3. bb_run_eval_IQL fed the recorded actions: the recorded states, rewards and returns, exactly;
4. TrainConfig, and the errors train() raises without a reward model.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import bb_env


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bb_train_run.npz")))


@pytest.fixture(scope="module")
def bb():
    from iqlpref_amd import custom_offline_bb
    return custom_offline_bb


def _arrays(golden):
    return {k[5:]: v for k, v in golden.items() if k.startswith("data/")}


def test_fixture_inputs_are_the_helpers(golden):
    for k, v in bb_env.synth_dataset().items():
        np.testing.assert_array_equal(golden[f"data/{k}"], v)
    np.testing.assert_array_equal(golden["move_stats"], bb_env.MOVE_STATS)


def test_sampler_walks_the_reference_epochs(golden, bb):
    s = bb.BlockEpochSampler(bb_env.N_ROWS, bb_env.BATCH, perm=golden["perm"])
    assert len(s) == 6 and s.n_blocks == 5 and s.tail == 7
    idx, valid = s.host_indices(0, 12)
    assert idx.dtype == np.int64 and valid.dtype == np.int32 and idx.shape == (12, 32)
    np.testing.assert_array_equal(valid, golden["batch_len"])
    for t in range(12):
        np.testing.assert_array_equal(idx[t, :valid[t]], golden["batch_rows"][t, :valid[t]])
        assert (idx[t, valid[t]:] == bb_env.N_ROWS - 1).all()  # padding: a row of the buffer
    np.testing.assert_array_equal(idx[6:], idx[:6])  # every epoch repeats the order
    # any start step: the same walk
    for t0 in (5, 6, 11, 12 * 10 ** 9 + 5):
        i2, v2 = s.host_indices(t0, 3)
        np.testing.assert_array_equal(i2, np.concatenate([idx, idx])[t0 % 6:t0 % 6 + 3])
        np.testing.assert_array_equal(v2, np.concatenate([valid, valid])[t0 % 6:t0 % 6 + 3])


def test_sampler_draws_torch_randperm(golden, bb):
    torch.manual_seed(int(golden["perm_seed"]))
    np.testing.assert_array_equal(bb.BlockEpochSampler(bb_env.N_ROWS, bb_env.BATCH).perm.numpy(), golden["perm"])
    g = torch.Generator().manual_seed(int(golden["perm_seed"]))
    np.testing.assert_array_equal(bb.BlockEpochSampler(bb_env.N_ROWS, bb_env.BATCH, generator=g).perm.numpy(),
                                  golden["perm"])
    no_tail = bb.BlockEpochSampler(160, 32, perm=[4, 3, 2, 1, 0])
    assert len(no_tail) == 5 and (no_tail.host_indices(0, 10)[1] == 32).all()
    short = bb.BlockEpochSampler(7, 32)  # fewer rows than one batch: the tail is all there is
    i, v = short.host_indices(3, 2)
    assert len(short) == 1 and (v == 7).all() and (i[:, :7] == np.arange(7)).all() and (i[:, 7:] == 6).all()
    for bad in ([0, 1, 2, 3], [0, 1, 2, 3, 3], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            bb.BlockEpochSampler(bb_env.N_ROWS, bb_env.BATCH, perm=bad)


def test_dataset_statistics_bit_for_bit(golden, bb):
    d = bb.BBDataset(_arrays(golden))
    assert len(d) == bb_env.N_ROWS and d.shapes() == ((167, 26), (167, 2))
    for got, key in ((d.max_actions().numpy(), "max_actions"), (d.min_actions().numpy(), "min_actions"),
                     (d.state_mean(), "state_mean"), (d.state_std(), "state_std")):
        want = golden[f"stats/{key}"]
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), key
    assert d.state_mean().dtype == np.float64
    assert (d.state_mean()[-4:] == 0).all() and (d.state_std()[-4:] == 1).all()
    raw = bb.BBDataset(_arrays(golden), normalized_states=False)
    assert (raw.state_mean() == 0).all() and (raw.state_std() == 1).all()


def test_dataset_transitions(golden, bb):
    a = _arrays(golden)
    d = bb.BBDataset(a, normalized_rewards=False, reward_adjustment=0.25)
    t = d.transitions()
    assert all(v.dtype == np.float32 for v in t.values())
    want = ((a["states"] - golden["stats/state_mean"]) / golden["stats/state_std"]).astype(np.float32)
    np.testing.assert_array_equal(t["observations"], want)
    np.testing.assert_array_equal(t["observations"][:, -4:], a["states"][:, -4:])
    np.testing.assert_array_equal(t["rewards"], (a["rewards"] + 0.25).astype(np.float32))
    np.testing.assert_array_equal(t["terminals"], 1 - a["attn_mask"])
    np.testing.assert_array_equal(bb.BBDataset(a).transitions()["rewards"], a["n_rewards"])


def test_dataset_refusals(golden, bb):
    a = _arrays(golden)
    for value in (0.5, 2.0, -1.0, np.nan):
        bad = dict(a, attn_mask=a["attn_mask"].copy())
        bad["attn_mask"][11] = value
        with pytest.raises(ValueError, match="attn_mask"):
            bb.BBDataset(bad)
    with pytest.raises(KeyError):
        bb.BBDataset({k: v for k, v in a.items() if k != "n_rewards"})
    with pytest.raises(ValueError):
        bb.BBDataset(dict(a, actions=a["actions"][:-1]))
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            bb.BBDataset("/nonexistent/bb.hdf5")


def test_simulator_replays_the_reference(golden, bb):
    """Float64 numpy on the same generator calls: exact, no quantity needs a tolerance."""
    actor = bb_env.ReplayActor(golden["eval/actions"])
    rewards = []

    def r_model(s, a, t, m, training=False):
        out = bb_env.numpy_reward(s, a, t, m, training=training)
        rewards.append(out[0]["value"][:, 0, -1])
        return out

    returns = bb.bb_run_eval_IQL(actor, int(golden["eval/num_episodes"]), r_model, tuple(golden["move_stats"]),
                                 state_mean=golden["stats/state_mean"], state_std=golden["stats/state_std"],
                                 max_horizon=int(golden["eval/max_horizon"]), seed=int(golden["eval/seed"]))
    assert actor.mode == ["eval", "train"]
    np.testing.assert_array_equal(np.asarray(actor.states), golden["eval/states"])
    np.testing.assert_array_equal(np.asarray(rewards), golden["eval/rewards"])
    np.testing.assert_array_equal(returns, golden["eval/returns"])
    assert len(actor.states) == len(golden["eval/actions"])


def test_simulator_stops_at_the_goal(bb):
    """An actor that heads straight for the goal at full speed reaches it: the episode ends early, and its
    length is the distance over the speed."""
    class Homing(bb_env.ReplayActor):
        def act(self, state, device="cpu"):
            self.states.append(np.array(state))
            dx, dy = state[20] - state[0], state[21] - state[1]
            return np.array([2.0, np.degrees(np.arctan2(dy, dx)) % 360.0], np.float32)

    actor = Homing([])
    ret = bb.bb_run_eval_IQL(actor, 3, bb_env.numpy_reward, bb_env.MOVE_STATS, max_horizon=60, seed=1)
    assert ret.shape == (3, 1) and len(actor.states) < 3 * 25
    first = actor.states[0]
    dist = np.hypot(first[20] - first[0], first[21] - first[1])
    lengths = np.diff([i for i, s in enumerate(actor.states) if i == 0 or not np.array_equal(s[20:22], actor.states[i - 1][20:22])]
                      + [len(actor.states)])
    assert abs(lengths[0] - dist / 2.0) <= 1.5


def test_train_config_is_the_reference(bb):
    c = bb.TrainConfig()
    want = dict(project="IQL-pref", group="IQL-BB", gamma=0.99, tau=0.005, beta=3.0, iql_tau=0.7,
                iql_deterministic=False, vf_lr=3e-4, qf_lr=3e-4, actor_lr=3e-4, actor_dropout=None,
                dataset_id="bbway1", update_steps=1000000, batch_size=256, normalize_state=False,
                normalize_reward=False, eval_every=5000, eval_episodes=10, train_seed=0, eval_seed=0,
                checkpoints_path=None)
    got = dataclasses.asdict(c)
    assert {k: got[k] for k in want} == want
    assert c.name.startswith("iql-bbway1-") and len(c.name) == len("iql-bbway1-") + 8
    c2 = bb.TrainConfig(checkpoints_path="/tmp/x")
    assert c2.checkpoints_path == os.path.join("/tmp/x", c2.name)


def test_train_without_reward_model_raises(bb):
    with pytest.raises((ImportError, NotImplementedError), match="reward_model"):
        bb.train(bb.TrainConfig(), dataset=bb_env.synth_dataset(), move_stats=bb_env.MOVE_STATS, device="cuda:0")
