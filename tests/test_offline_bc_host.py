"""offline_bc (algorithms/offline/any_percent_bc.py, "dbc") without a GPU: the host restatement of the selection
against tests/golden/offline_bc_select.npz (the reference's own keep_best_trajectories) bit for bit, the rule of
the scale table against the Python loop, the mirrored surface, train()'s bookkeeping on stub steppers, and the
choices make_offline_bc_fixture.py committed."""
import dataclasses
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib, minari_bc, offline_bc
from tests import helpers, minari_cases as mc, offline_bc_env as obe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "float64")


@pytest.fixture(scope="module")
def select(golden_dir):
    return mc.load(golden_dir, "offline_bc_select.npz")


@pytest.fixture(scope="module")
def run(golden_dir):
    return mc.load(golden_dir, "offline_bc_run.npz")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def python_loop(rewards, terminals, discount, max_len):
    """dbc:212-226 restated literally: (ids_by_trajectories, returns)."""
    ids, returns, cur_ids, cur_return, scale = [], [], [], 0, 1.0
    for i, (reward, done) in enumerate(zip(rewards, terminals)):
        cur_return += scale * reward
        cur_ids.append(i)
        scale *= discount
        if done == 1.0 or len(cur_ids) == max_len:
            ids.append(list(cur_ids))
            returns.append(cur_return)
            cur_ids, cur_return, scale = [], 0, 1.0
    return ids, returns


# --------------------------------------------------------------------------- #
# selection
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(obe.CASES))
def test_host_selection_is_the_references(select, name, dtype):
    n, max_len, term_rows, fracs, ordered = obe.CASES[name]
    g = mc.run_of(select, f"{name}/{dtype}")
    data = obe.selection_case(name, np.dtype(dtype))
    np.testing.assert_array_equal(bits(data["rewards"]), bits(g["in/rewards"]))  # the fixture's inputs are these
    np.testing.assert_array_equal(data["terminals"], g["in/terminals"])
    np.testing.assert_array_equal(data["actions"], g["in/actions"])
    if "raises" in g:
        assert name == "n1_open"
        with pytest.raises(IndexError):
            offline_bc.keep_best_trajectories(data, 1.0, float(select["discount"]), max_len)
        return
    starts, lengths = offline_bc.trajectory_bounds(data["terminals"], max_len)
    np.testing.assert_array_equal(starts, g["starts"])
    np.testing.assert_array_equal(lengths, g["lengths"])
    returns = offline_bc.trajectory_returns(data["rewards"], starts, lengths, float(select["discount"]))
    assert returns.dtype == g["returns"].dtype == np.dtype(dtype)
    np.testing.assert_array_equal(bits(returns), bits(g["returns"]))
    for frac in fracs:
        d = {k: v.copy() for k, v in data.items()}
        offline_bc.keep_best_trajectories(d, frac, float(select["discount"]), max_len)
        kept = max(1, int(frac * len(starts)))
        assert len(g[f"{frac}/top"]) == kept
        assert len(d["rewards"]) == (len(g[f"{frac}/rewards"]) if ordered else d["observations"].shape[0])
        if ordered:
            np.testing.assert_array_equal(offline_bc.rank_trajectories(returns, frac), g[f"{frac}/top"])
            for k in offline_bc.ARRAYS:
                assert d[k].dtype == g[f"{frac}/{k}"].dtype and d[k].shape == g[f"{frac}/{k}"].shape, k
                np.testing.assert_array_equal(d[k], g[f"{frac}/{k}"], err_msg=f"{frac}/{k}")
        else:  # equal returns: which trajectories are kept is the sorting host's; they are whole ones, `kept` of them
            rows = d["observations"][:, 0].astype(np.int64)
            cuts = np.flatnonzero(np.diff(rows) != 1) + 1
            pieces = np.split(rows, cuts)
            assert len(pieces) == kept and all(p[0] in starts and len(p) == lengths[list(starts).index(p[0])] for p in pieces)


def test_fixture_cases_are_what_the_issue_lists(select):
    assert list(select["cases"]) == sorted(obe.CASES)
    for name, (n, max_len, term_rows, fracs, ordered) in obe.CASES.items():
        if ordered and name != "n1_open":
            r = select[f"{name}/float32/returns"]
            assert len(set(r.tolist())) == len(r), name  # ORDER is compared on these: no equal returns
    assert not select["ties/float32/returns"].any() and len(select["ties/float32/returns"]) == 10
    # m7_n50: terminals on a cut (6, 16), between cuts (9), a one-row trajectory (17), the last 4 rows dropped
    np.testing.assert_array_equal(select["m7_n50/float32/starts"], [0, 7, 10, 17, 18, 25, 32, 39])
    np.testing.assert_array_equal(select["m7_n50/float32/lengths"], [7, 3, 7, 1, 7, 7, 7, 7])
    np.testing.assert_array_equal(select["term_at_cut/float32/lengths"], [10, 10, 10])
    np.testing.assert_array_equal(select["trailing/float32/lengths"], [11, 15])
    np.testing.assert_array_equal(select["chunks/float32/starts"], [0, 1000, 1501, 2501])
    np.testing.assert_array_equal(select["chunks/float32/lengths"], [1000, 501, 1000, 300])
    assert len(select["m1_n50/float32/top"] if "m1_n50/float32/top" in select else select["m1_n50/float32/1e-09/top"]) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_table_rule_is_the_python_loops(dtype):
    """1,000 random rewards at discount 0.99, cut at 1000 and at 37 rows: the restatement's returns equal the literal
    loop's bit for bit; the table is the Python float after k multiplications, rounded to the rewards' dtype."""
    rng = np.random.default_rng(5)
    rewards = rng.standard_normal(1000).astype(dtype)
    terminals = rng.uniform(size=1000) < 0.01
    terminals[-1] = True
    for max_len in (1000, 37):
        ids, want = python_loop(rewards, terminals, 0.99, max_len)
        starts, lengths = offline_bc.trajectory_bounds(terminals, max_len)
        assert [t[0] for t in ids] == starts.tolist() and [len(t) for t in ids] == lengths.tolist()
        got = offline_bc.trajectory_returns(rewards, starts, lengths, 0.99)
        assert got.dtype == np.asarray(want).dtype == np.dtype(dtype)
        np.testing.assert_array_equal(bits(got), bits(np.asarray(want)))
    table = offline_bc.return_scale_table(0.99, 1000)
    s, mine = 1.0, []
    for k in range(1000):
        mine.append(np.float32(s))
        s *= 0.99
    assert table.dtype == np.float32
    np.testing.assert_array_equal(bits(table), bits(np.asarray(mine)))
    t64, s = offline_bc.return_scale_table(0.99, 1000, np.float64), 1.0
    for k in range(1000):  # (float64 rewards see the Python float itself)
        assert t64[k] == s
        s *= 0.99


def test_selection_refuses_what_it_does_not_take():
    with pytest.raises(TypeError, match="float32"):
        offline_bc.select_best_trajectories(np.zeros((2, 1), np.float32), np.zeros((2, 1), np.float32),
                                            np.zeros((2, 1), np.float32), np.zeros(2), np.ones(2, bool), 1.0, 0.99,
                                            device="cuda:0")  # (said before the device is looked at)


# --------------------------------------------------------------------------- #
# the mirrored surface
# --------------------------------------------------------------------------- #
def test_config_fields_and_defaults():
    d = {f.name: f.default for f in dataclasses.fields(offline_bc.TrainConfig)}
    assert d == dict(project="CORL", group="BC-D4RL", name="BC", env="halfcheetah-medium-expert-v2",
                     max_timesteps=1000000, batch_size=256, buffer_size=2000000, frac=0.1, max_traj_len=1000,
                     normalize=True, discount=0.99, eval_freq=5000, n_episodes=10, checkpoints_path=None, load_model="",
                     seed=0, device="cuda")
    assert list(d) == ["project", "group", "name", "env", "max_timesteps", "batch_size", "buffer_size", "frac",
                       "max_traj_len", "normalize", "discount", "eval_freq", "n_episodes", "checkpoints_path",
                       "load_model", "seed", "device"]
    cfg = offline_bc.TrainConfig(checkpoints_path="/tmp/x")
    stem = "BC-halfcheetah-medium-expert-v2-"
    assert cfg.name.startswith(stem) and len(cfg.name) == len(stem) + 8
    assert cfg.checkpoints_path == os.path.join("/tmp/x", cfg.name)
    cfg = offline_bc.load_config(None, frac="0.25", eval_freq="1000", normalize="false", env="antmaze-umaze-v2")
    assert (cfg.frac, cfg.eval_freq, cfg.normalize, cfg.env) == (0.25, 1000, False, "antmaze-umaze-v2")
    with pytest.raises(ValueError, match="top_fraction"):
        offline_bc.load_config(None, top_fraction=0.1)


def test_state_dict_has_the_references_three_keys(run):
    actor = offline_bc.Actor(17, 6, 1.0)
    assert offline_bc.Actor is minari_bc.Actor and list(actor.state_dict()) == list(mc.NAMES)
    opt = torch.optim.Adam(actor.parameters(), lr=3e-4)
    shell = types.SimpleNamespace(actor=actor, actor_optimizer=opt, total_it=0, _handle=None)
    sd = offline_bc.BC.state_dict(shell)
    saved = [k for k in run if k.endswith("/keys")]
    assert len(saved) == 4  # three checkpoints of the run, one of the continuation
    for k in saved:
        assert sorted(sd) == list(run[k]) == ["actor", "actor_optimizer", "total_it"]
    whole = str(run["run/whole"])
    assert whole in list(run["run/save_name"]) and int(run[f"run/{whole}/total_it"]) == int(whole[11:-3]) + 1
    import inspect
    assert list(inspect.signature(offline_bc.BC.__init__).parameters)[:6] == \
        ["self", "max_action", "actor", "actor_optimizer", "discount", "device"]
    assert list(inspect.signature(offline_bc.eval_actor).parameters) == ["env", "actor", "device", "n_episodes", "seed"]
    assert list(inspect.signature(offline_bc.keep_best_trajectories).parameters) == \
        ["dataset", "frac", "discount", "max_episode_steps"]
    assert inspect.signature(offline_bc.keep_best_trajectories).parameters["max_episode_steps"].default == 1000


def test_replay_buffer_names_and_errors():
    rb = offline_bc.ReplayBuffer
    assert all(callable(getattr(rb, n)) for n in ("load_d4rl_dataset", "sample", "add_transition"))
    z = lambda n, w: torch.zeros((n, w))
    full = types.SimpleNamespace(_size=3, _buffer_size=10)
    with pytest.raises(ValueError, match="non-empty replay buffer"):
        rb.load_device_arrays(full, z(2, 4), z(2, 2), z(2, 1), z(2, 4), z(2, 1))
    small = types.SimpleNamespace(_size=0, _buffer_size=1)
    with pytest.raises(ValueError, match="smaller than the dataset"):
        rb.load_device_arrays(small, z(2, 4), z(2, 2), z(2, 1), z(2, 4), z(2, 1))
    with pytest.raises(NotImplementedError):
        rb.add_transition(full)


def test_new_entry_points_are_bound_as_declared():
    with open(os.path.join(ROOT, "include", "iqlhip.h")) as f:
        header = helpers.parse_c_header(f.read())
    new = {"iqlhip_prep_trajectory_returns", "iqlhip_prep_gather_trajectories"}
    assert new <= set(header["functions"]) and new <= set(_lib.SYMBOLS)
    for n in new:
        assert len(_lib.SYMBOLS[n][1]) == len(header["functions"][n][1]), n
    assert _lib.ABI_VERSION == 6  # entry points were added, nothing changed


# --------------------------------------------------------------------------- #
# train(): bookkeeping on stub steppers (no device)
# --------------------------------------------------------------------------- #
class _Buffer:
    made = []

    def __init__(self, state_dim, action_dim, buffer_size, device):
        self.n = None
        _Buffer.made.append(self)

    def load_d4rl_dataset(self, data):
        self.n, self.data = data["observations"].shape[0], data

    def index_bound(self):
        return self.n

    def draw_indices(self, batch_size, n_batches=None, rng=None):
        gen = np.random if rng is None else rng
        return np.stack([gen.randint(0, self.n, size=batch_size) for _ in range(n_batches)])


class _Actor:
    mode = "train"

    def eval(self):
        self.mode = "eval"

    def train(self):
        self.mode = "train"

    def act(self, state, device):
        assert self.mode == "eval"
        return np.zeros(6)


class _Trainer:
    def __init__(self):
        self.actor, self.total_it, self._dev = _Actor(), 0, "cpu"

    def state_dict(self):
        return {"total_it": self.total_it}

    def load_state_dict(self, sd):
        self.total_it = sd["total_it"]


class _Stepper:
    def __init__(self, trainers):
        self.trainers = trainers

    def train_steps(self, bufs, n, B, *, indices, return_losses=False):
        out = []
        for tr, idx in zip(self.trainers, indices):
            assert tuple(idx.shape) == (n, B)
            out.append(torch.arange(tr.total_it, tr.total_it + n, dtype=torch.float32)[:, None])
            tr.total_it += n
        return out

    def synchronize(self):
        pass

    def close(self):
        pass


def _stub_train(monkeypatch, tmp_path, seeds_per_gpu=1, **config_kw):
    _Buffer.made.clear()
    monkeypatch.setattr(offline_bc, "ReplayBuffer", _Buffer)
    monkeypatch.setattr(offline_bc, "_build_trainer", lambda *a, **k: _Trainer())
    monkeypatch.setattr(offline_bc, "stepper", lambda trainers: _Stepper(trainers))
    config = offline_bc.TrainConfig(env=obe.ENV, max_timesteps=7, eval_freq=3, batch_size=4, n_episodes=2, frac=obe.FRAC,
                                    checkpoints_path=str(tmp_path), **config_kw)
    records = []
    dataset = obe.make_dataset(11, np.float64)  # (float64 rewards: the host restatement, no device)
    out = offline_bc.train(config, dataset, obe.OfflineBCEnv(), logger=lambda d, step: records.append((step, dict(d))),
                           sampler="host", device="cpu", chunk=2, seeds_per_gpu=seeds_per_gpu)
    return config, records, out, dataset


def test_train_bookkeeping_on_stub_steppers(monkeypatch, tmp_path):
    config, records, trainer, dataset = _stub_train(monkeypatch, tmp_path, max_traj_len=7)
    # one record per step at step = total_it (one-based); the score right behind the step that ends a period
    keys = [(s, list(d)) for s, d in records]
    assert keys == [(1, ["actor_loss"]), (2, ["actor_loss"]), (3, ["actor_loss"]), (3, ["d4rl_normalized_score"]),
                    (4, ["actor_loss"]), (5, ["actor_loss"]), (6, ["actor_loss"]), (6, ["d4rl_normalized_score"]),
                    (7, ["actor_loss"])]
    assert [d["actor_loss"] for s, d in records if "actor_loss" in d] == [float(i) for i in range(7)]
    # checkpoints carry the zero-based t of the step that ended the period, beside config.yaml
    assert sorted(os.listdir(config.checkpoints_path)) == ["checkpoint_2.pt", "checkpoint_5.pt", "config.yaml"]
    assert torch.load(os.path.join(config.checkpoints_path, "checkpoint_5.pt"))["total_it"] == 6
    assert trainer.total_it == 7 and trainer.actor.mode == "train"
    # the score is get_normalized_score(mean) * 100 of eval_actor's returns at the run's seed
    env = offline_bc.wrap_env(obe.OfflineBCEnv(), 0.0, 1.0)
    actor = _Actor()
    want = env.get_normalized_score(offline_bc.eval_actor(env, actor, "cpu", 2, config.seed).mean()) * 100.0
    assert actor.mode == "train"
    # (observations are normalised for the actor only; the stub ignores them, so the returns are the same)
    assert [d["d4rl_normalized_score"] for s, d in records if "d4rl_normalized_score" in d] == [want, want]
    # max_traj_len = 7 was ignored: the buffer holds the selection cut at 1000 rows, best first
    ref = obe.make_dataset(11, np.float64)
    offline_bc.keep_best_trajectories(ref, obe.FRAC, config.discount)
    assert _Buffer.made[0].n == len(ref["rewards"]) == 1000 + 47 + 33 + 55
    np.testing.assert_array_equal(dataset["rewards"], ref["rewards"])  # (the host path rewrites the dict, as dbc does)
    cut7 = obe.make_dataset(11, np.float64)
    offline_bc.keep_best_trajectories(cut7, obe.FRAC, config.discount, 7)
    assert len(cut7["rewards"]) != len(ref["rewards"])


def test_group_records_carry_their_seed_and_no_other_key(monkeypatch, tmp_path):
    """K = 2: what reaches the logger is an ``actor_loss`` or a ``d4rl_normalized_score`` record under the seed of
    its member, the score that of the member's own evaluation seed."""
    config, records, trainers, _ = _stub_train(monkeypatch, tmp_path, seeds_per_gpu=2)
    seeds = [config.seed, config.seed + 1]
    assert len(trainers) == 2 and sorted(os.listdir(config.checkpoints_path)) == ["config.yaml", "seed_0", "seed_1"]
    assert all(set(d) <= {"actor_loss", "d4rl_normalized_score", "seed"} and d["seed"] in seeds for s, d in records)
    env = offline_bc.wrap_env(obe.OfflineBCEnv(), 0.0, 1.0)
    wants = []
    for seed in seeds:
        mine = [(s, d) for s, d in records if d["seed"] == seed]
        assert [s for s, d in mine if "actor_loss" in d] == list(range(1, 8))
        want = env.get_normalized_score(offline_bc.eval_actor(env, _Actor(), "cpu", 2, seed).mean()) * 100.0
        assert [(s, d["d4rl_normalized_score"]) for s, d in mine if "actor_loss" not in d] == [(3, want), (6, want)]
        wants.append(want)
    assert wants[0] != wants[1]  # (the evaluation seed is the member's: a record under the wrong seed would show)
    assert [(s, d["seed"]) for s, d in records if "actor_loss" not in d] == [(3, 0), (3, 1), (6, 0), (6, 1)]


def test_train_continues_a_loaded_models_count(monkeypatch, tmp_path):
    path = tmp_path / "model.pt"
    torch.save({"total_it": 40}, path)
    config, records, trainer, _ = _stub_train(monkeypatch, tmp_path / "run", load_model=str(path))
    assert [s for s, d in records] == [41, 42, 43, 43, 44, 45, 46, 46, 47] and trainer.total_it == 47
    assert sorted(f for f in os.listdir(config.checkpoints_path) if f.endswith(".pt")) == ["checkpoint_2.pt", "checkpoint_5.pt"]


def test_train_checks_its_arguments_first():
    with pytest.raises(ValueError, match="sampler"):
        offline_bc.train(offline_bc.TrainConfig(), {}, None, sampler="philox")
    with pytest.raises(ValueError, match="seeds_per_gpu"):
        offline_bc.train(offline_bc.TrainConfig(), {}, None, seeds_per_gpu=17)
    with pytest.raises(ValueError, match="load_model"):
        offline_bc.train(offline_bc.TrainConfig(load_model="x.pt"), {}, None, seeds_per_gpu=2)


def test_eval_actor_seeds_once_and_chains_episodes():
    env, actor = obe.OfflineBCEnv(), _Actor()
    seeds = []
    real = env.seed
    env.seed = lambda s: (seeds.append(s), real(s))[1]
    a = offline_bc.eval_actor(env, actor, "cpu", 3, 5)
    b = offline_bc.eval_actor(env, actor, "cpu", 3, 5)
    assert seeds == [5, 5] and a.shape == (3,) and a.dtype == np.float64
    np.testing.assert_array_equal(a, b)  # seeded again: the same three chained episodes
    assert len(set(a.tolist())) == 3     # (chained: not one episode three times)


def test_awacs_eval_actor_is_the_same_object(monkeypatch):
    from iqlpref_amd import _d4rl, awac
    assert awac.eval_actor is _d4rl.eval_actor and offline_bc.eval_actor is _d4rl.eval_actor
    monkeypatch.setattr(offline_bc, "eval_actor", awac.eval_actor)  # (the test above, through awac's name)
    test_eval_actor_seeds_once_and_chains_episodes()


# --------------------------------------------------------------------------- #
# the generator's committed choices
# --------------------------------------------------------------------------- #
def test_fixture_run_is_what_the_generator_would_choose_again(run):
    spec = importlib.util.spec_from_file_location(
        "make_offline_bc_fixture", os.path.join(ROOT, "tests", "golden", "make_offline_bc_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for k, v in gen.COMMON.items():
        assert run[f"common/{k}"] == v, k
    assert (gen.RTOL, gen.ATOL, gen.EVAL_TOL) == (2e-5, 2e-8, 1e-5)  # tests/test_gpu_minari_bc.py's bounds
    steps, every = gen.COMMON["max_timesteps"], gen.COMMON["eval_freq"]
    tried, ok = run["run/candidates"], run["run/candidate_ok"]
    assert tried[0] == run["common/first_seed"] == gen.FIRST_SEED and list(tried) == list(range(tried[0], tried[0] + len(tried)))
    assert ok[-1] and not ok[:-1].any() and run["run/train_seed"] == tried[-1]
    # the reference alone stays inside the bounds for twice the recorded length
    assert run["run/f64_gap_of_bound"].shape == (2 * steps,) and run["run/f64_gap_of_bound"].max() < 1
    assert run["run/f64_eval_gap_of_bound"].shape == (2 * steps // every,) and run["run/f64_eval_gap_of_bound"].max() < 1
    assert run["run/f64_measured_steps"] >= 2 * steps
    assert run["run/f64_first_step_beyond"] == -1 or run["run/f64_first_step_beyond"] >= 2 * steps
    # no recorded step on a relu kink that another fp32 summation order could take the other way (kink_margin)
    assert run["common/kink_sigmas"] == gen.KINK_SIGMAS == 4.0 and run["run/kink_margin"] > 1
    # the continuation: from the first of the run's checkpoints that keeps both margins, for CONT_STEPS steps
    ctried, cok = list(run["cont/candidates"]), run["cont/candidate_ok"]
    assert ctried == list(run["run/save_name"])[:len(ctried)] and cok[-1] and not cok[:-1].any()
    assert str(run["run/whole"]) == ctried[-1] and run["cont/kink_margin"] > 1 and run["cont/steps"] == gen.CONT_STEPS
    assert run["cont/f64_gap_of_bound"].shape == (2 * gen.CONT_STEPS,) and run["cont/f64_gap_of_bound"].max() < 1
    assert run["cont/f64_eval_gap_of_bound"].max() < 1
    it0 = int(run[f"run/{ctried[-1]}/total_it"])
    ckeys = run["cont/rec_key"]
    np.testing.assert_array_equal(run["cont/rec_step"][ckeys == "actor_loss"], np.arange(it0 + 1, it0 + gen.CONT_STEPS + 1))
    # the run itself: 45 losses at steps 1 .. 45, a score at 15 / 30 / 45, checkpoints named by the zero-based step
    keys, rsteps = run["run/rec_key"], run["run/rec_step"]
    np.testing.assert_array_equal(rsteps[keys == "actor_loss"], np.arange(1, steps + 1))
    np.testing.assert_array_equal(rsteps[keys == "d4rl_normalized_score"], [15, 30, 45])
    assert set(keys) == {"actor_loss", "d4rl_normalized_score"}
    assert list(run["run/save_name"]) == ["checkpoint_14.pt", "checkpoint_29.pt", "checkpoint_44.pt"]
    lo, hi = obe.SCORE_RANGE
    np.testing.assert_allclose(run["run/rec_value"][keys == "d4rl_normalized_score"],
                               (run["run/eval_returns"].mean(1) - lo) / (hi - lo) * 100.0, rtol=1e-15)
    # the training rows: our host restatement selects what the reference selected
    d = obe.make_dataset(int(run["common/data_seed"]))
    starts, lengths = offline_bc.trajectory_bounds(d["terminals"], 1000)
    returns = offline_bc.trajectory_returns(d["rewards"], starts, lengths, 0.99)
    np.testing.assert_array_equal(bits(returns), bits(run["select/returns"]))
    np.testing.assert_array_equal(offline_bc.rank_trajectories(returns, obe.FRAC), run["select/top"])
    assert list(lengths[run["select/top"]]) == [1000, 47, 33, 55]
    offline_bc.keep_best_trajectories(d, obe.FRAC, 0.99)
    np.testing.assert_array_equal(bits(d["rewards"]), bits(run["select/rewards"]))
    assert np.float64(d["observations"].astype(np.float64).sum()) == run["select/obs_sum"]
