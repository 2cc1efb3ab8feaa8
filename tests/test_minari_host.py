"""The host side of ``minari_iql`` and ``minari_bc`` against what the reference itself computed
(tests/golden/minari_*_run.npz, make_minari_fixture.py): the any-percent selection, the two dataset builders, the
configs, the state-dict keys, the binding of the new entry points, the loop without best-model bookkeeping.
No GPU, no library load."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib, _offline_loop, custom_offline, minari_bc, minari_iql
from tests import helpers, minari_cases as mc, minari_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.45, 0.05, 0.3, 0.6, 1.0)


@pytest.fixture(scope="module")
def bc_golden(golden_dir):
    return mc.load(golden_dir, "minari_bc_run.npz")


@pytest.fixture(scope="module")
def iql_golden(golden_dir):
    return mc.load(golden_dir, "minari_iql_run.npz")


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_discounted_return_in_the_stored_dtype(bc_golden, dtype):
    ds = minari_env.MinariDataset(11, reward_dtype=dtype)
    want = bc_golden[f"select/{np.dtype(dtype).name}/returns"]
    got = [minari_bc.discounted_return(ep.rewards, 0.99) for ep in ds]
    assert all(np.asarray(r).dtype == dtype for r in got)
    np.testing.assert_array_equal(np.asarray(got, dtype), want)  # bit for bit: the same sums in the same order
    a, b = minari_env.TIE
    assert got[a] == got[b]
    # the float32 sums are not the float64 sums rounded: a float64 accumulation would be caught above
    if dtype == np.float32:
        wide = [minari_bc.discounted_return(ep.rewards.astype(np.float64), 0.99) for ep in ds]
        assert any(np.float32(w) != g for w, g in zip(wide, got))
    assert minari_bc.discounted_return(np.asarray([2.5], dtype), 0.99) == dtype(2.5)  # a one-step episode


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("fraction", FRACTIONS)
def test_selection_and_rows_are_the_references(bc_golden, dtype, fraction):
    ds = minari_env.MinariDataset(11, reward_dtype=dtype)
    tag = f"select/{np.dtype(dtype).name}/{fraction}"
    ids = minari_bc.best_trajectories_ids(ds, fraction, 0.99)
    np.testing.assert_array_equal(ids, bc_golden[f"{tag}/ids"])
    assert len(ids) == max(1, int(fraction * len(ds)))
    q = minari_bc.qlearning_dataset(ds, ids)
    assert set(q) == {"observations", "actions", "next_observations", "rewards", "terminals"}
    assert q["observations"].dtype == q["actions"].dtype == q["next_observations"].dtype == np.float32
    assert q["rewards"].dtype == dtype
    np.testing.assert_array_equal(q["rewards"], bc_golden[f"{tag}/rewards"])
    np.testing.assert_array_equal(q["terminals"], bc_golden[f"{tag}/terminals"])
    np.testing.assert_array_equal(q["actions"][0], bc_golden[f"{tag}/first_action"])
    assert q["observations"].astype(np.float64).sum() == bc_golden[f"{tag}/obs_sum"]
    # rows in the order of the ids, best first -- not in dataset order
    first = ds.episodes[ids[0]]
    np.testing.assert_array_equal(q["observations"][:len(first.actions)], first.observations[:-1].astype(np.float32))
    np.testing.assert_array_equal(q["next_observations"][0], first.observations[1].astype(np.float32))


def test_the_fixture_meets_the_awkward_cases(bc_golden):
    """A tie on the selection boundary (the stable sort keeps the earlier episode), a fractional count, and a
    fraction so small that one episode remains."""
    a, b = minari_env.TIE
    n = len(minari_env.LENGTHS)
    assert minari_env.TOP_FRACTION * n != int(minari_env.TOP_FRACTION * n)
    ids = list(bc_golden["select/float64/0.45/ids"])
    assert len(ids) == 3 and ids[-1] == a and b not in ids
    assert list(bc_golden["select/float64/0.6/ids"])[2:4] == [a, b]
    assert len(bc_golden["select/float64/0.05/ids"]) == 1
    assert sorted(bc_golden["select/float64/1.0/ids"]) == list(range(n))
    assert ids != sorted(ids)  # (best first differs from dataset order: the row layout is observable)
    # a plain list of episodes (no iterate_episodes) is looked up by id
    ds = minari_env.MinariDataset(11)
    q = minari_bc.qlearning_dataset(list(ds), ids)
    np.testing.assert_array_equal(q["rewards"], bc_golden["select/float64/0.45/rewards"])


def test_task_reward_dataset_is_the_references(iql_golden):
    ds = minari_env.MinariDataset(11)
    q = minari_iql.qlearning_dataset(ds)
    assert list(q) == ["observations", "actions", "next_observations", "rewards", "terminals"]
    np.testing.assert_array_equal(q["rewards"], iql_golden["select/rewards"])
    assert q["rewards"].dtype == np.float64  # as stored: the cast to float32 is the buffer's
    np.testing.assert_array_equal(q["terminals"], iql_golden["select/terminals"])
    assert q["observations"].astype(np.float64).sum() == iql_golden["select/obs_sum"]
    assert q["observations"].shape == (sum(minari_env.LENGTHS), 45) and q["actions"].shape[1] == 24
    as_dicts = [vars(ep) for ep in ds]
    np.testing.assert_array_equal(minari_iql.qlearning_dataset(as_dicts)["rewards"], q["rewards"])


def _defaults(cls):
    return {f.name: f.default for f in dataclasses.fields(cls)}


def test_config_fields_and_defaults():
    bc = _defaults(minari_bc.TrainConfig)
    assert bc == dict(project="CORL", group="BC-Minari", name="bc", gamma=0.99, top_fraction=0.1,
                      dataset_id="pen-human-v1", update_steps=1000000, buffer_size=2000000, batch_size=256,
                      normalize_state=True, eval_every=5000, eval_episodes=10, train_seed=0, eval_seed=0,
                      checkpoints_path=None)
    assert list(bc) == ["project", "group", "name", "gamma", "top_fraction", "dataset_id", "update_steps", "buffer_size",
                        "batch_size", "normalize_state", "eval_every", "eval_episodes", "train_seed", "eval_seed",
                        "checkpoints_path"]
    iql, custom = _defaults(minari_iql.TrainConfig), _defaults(custom_offline.TrainConfig)
    assert [k for k in custom if k not in ("reward_model_path", "query_length")] == list(iql)
    assert {k: v for k, v in iql.items() if k not in ("group", "name")} == \
        {k: v for k, v in custom.items() if k in iql and k not in ("group", "name")}
    assert (iql["group"], iql["name"], iql["dataset_id"]) == ("IQL-Minari", "iql", "D4RL/pen/human-v2")
    for cls, stem in ((minari_bc.TrainConfig, "bc-pen-human-v1-"), (minari_iql.TrainConfig, "iql-D4RL/pen/human-v2-")):
        cfg = cls(checkpoints_path="/tmp/x")
        assert cfg.name.startswith(stem) and len(cfg.name) == len(stem) + 8
        assert cfg.checkpoints_path == os.path.join("/tmp/x", cfg.name)


def test_bc_state_dict_has_the_references_keys(bc_golden):
    """``BC.state_dict`` on a trainer that has not stepped (nothing of it needs the device) against the key list
    of every checkpoint the reference wrote; the Actor's parameter names against the reference's."""
    actor = minari_bc.Actor(45, 24, 1.0)
    opt = torch.optim.Adam(actor.parameters(), lr=3e-4)
    shell = types.SimpleNamespace(actor=actor, actor_optimizer=opt, total_it=0, _handle=None)
    sd = minari_bc.BC.state_dict(shell)
    saved = [k for k in bc_golden if k.endswith("/keys")]
    assert len(saved) == 6  # three checkpoints of each of the two runs
    for k in saved:
        assert sorted(sd) == list(bc_golden[k]) == ["actor", "actor_optimizer"]
    fname, ref_sd = mc.bc_state_dict(mc.run_of(bc_golden, "raw"))
    assert fname == "checkpoint_14.pt"
    assert list(sd["actor"]) == list(ref_sd["actor"]) == list(mc.NAMES)
    assert {k: tuple(v.shape) for k, v in sd["actor"].items()} == {k: tuple(v.shape) for k, v in ref_sd["actor"].items()}
    # the reference's file goes into a torch Adam over these parameters as it is
    actor.load_state_dict(ref_sd["actor"])
    opt.load_state_dict(ref_sd["actor_optimizer"])
    assert float(opt.state[actor.net[0].weight]["step"]) == 15.0


def test_new_entry_points_are_bound_as_declared():
    with open(os.path.join(ROOT, "include", "iqlhip.h")) as f:
        header = helpers.parse_c_header(f.read())
    new = {n for n in header["functions"] if n.startswith("iqlhip_bc_")}
    assert new == {"iqlhip_bc_arena_layout", "iqlhip_bc_create", "iqlhip_bc_destroy", "iqlhip_bc_sync_weights",
                   "iqlhip_bc_set_step", "iqlhip_bc_set_lr", "iqlhip_bc_train_steps", "iqlhip_bc_copy_out",
                   "iqlhip_bc_group_create", "iqlhip_bc_group_destroy", "iqlhip_bc_group_train_steps"}
    assert new <= set(_lib.SYMBOLS)
    for n in new:
        assert len(_lib.SYMBOLS[n][1]) == len(header["functions"][n][1]), n
    assert {"iqlhip_bc", "iqlhip_bc_group"} <= header["opaque"]
    assert _lib.ABI_VERSION == 6  # entry points were added, nothing changed
    with open(os.path.join(ROOT, "iqlpref_amd", "csrc", "api.hip")) as f:
        assert "iqlhip_abi_version(void) { return 6; }" in f.read()


class _FakeTrainer:
    def __init__(self):
        self.saved = 0

    def state_dict(self):
        self.saved += 1
        return {"n": self.saved}


_half = lambda scores: 0.5 * scores


def _loop(tmp_path, recorder):
    records = []
    trainer = _FakeTrainer()
    os.makedirs(tmp_path)
    width = len(recorder.loss_names)
    steps = lambda group, active, t, n: [torch.arange(t, t + n, dtype=torch.float32)[:, None].repeat(1, width)]
    _offline_loop.run([trainer], [0], lambda active: None, 6, 3, 4, lambda d, step: records.append((step, dict(d))),
                      [str(tmp_path)], steps, lambda k, tr, step: np.asarray([1.0 + step, 3.0 + step]), recorder)
    return records, sorted(os.listdir(tmp_path))


def test_loop_without_best_model_bookkeeping(tmp_path):
    """``EvalRecords`` with one loss column: bcref's records and files, nothing else; ``BestModelRecords`` keeps
    the records and files of every other caller."""
    rec, files = _loop(tmp_path / "bc", _offline_loop.EvalRecords(_half, ("actor_loss",)))
    assert files == ["checkpoint_2.pt", "checkpoint_5.pt"]
    want = [(i, {"actor_loss": float(i)}) for i in range(3)] + [(2, {"evaluation_return": 4.0}), (2, {"normalized_score": 200.0})]
    want += [(i, {"actor_loss": float(i)}) for i in range(3, 6)] + [(5, {"evaluation_return": 7.0}), (5, {"normalized_score": 350.0})]
    assert rec == want
    rec, files = _loop(tmp_path / "iql", _offline_loop.BestModelRecords([str(tmp_path / "iql")], _half))
    assert files == ["best_model.pt", "checkpoint_2.pt", "checkpoint_5.pt"]
    assert rec[0] == (0, {"value_loss": 0.0, "q_loss": 0.0, "actor_loss": 0.0})
    assert [list(d)[0] for s, d in rec if s == 2][1:] == ["evaluation_return", "normalized_score", "best_score_so_far",
                                                        "best_step_so_far"]


def test_train_functions_check_their_arguments_first():
    """What is wrong with the call is reported before the device or the dataset is looked at."""
    for mod in (minari_bc, minari_iql):
        with pytest.raises(ValueError, match="sampler"):
            mod.train(mod.TrainConfig(), [], None, sampler="philox")
        with pytest.raises(ValueError, match="seeds_per_gpu"):
            mod.train(mod.TrainConfig(), [], None, seeds_per_gpu=17)
