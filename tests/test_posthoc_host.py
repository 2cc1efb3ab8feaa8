"""Host side of the post-hoc checkpoint evaluation (no GPU): the lock-step scheduler of
``posthoc.evaluate_many`` against a sequential restatement of the two reference loops, in this process and
in worker processes; ``expand_eval_sweep``; the three writers; the iqlhip_mlp_set symbols and every refusal
of ``iqlhip_mlp_set_create`` / ``_forward`` that returns before a HIP call.

The pointers handed to the library here are made-up non-null addresses: a refused call dereferences none."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests.fake_envs import FakeGymEnv, FakeGymnasiumEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FAKE = 0x10000
NAME = "halfcheetah-medium-v2"  # 17 -> 6
M, EPISODES, SEED = 3, 7, 40


# ---- environments whose episode length depends on the seed (fake_envs) AND on the actions: the episode
# ---- also ends at the first step from the third on whose first action component is positive
class EarlyGymnasiumEnv(FakeGymnasiumEnv):
    def step(self, action):
        obs, r, term, trunc, info = super().step(action)
        if self.t >= 3 and float(np.asarray(action).reshape(-1)[0]) > 0 and not (term or trunc):
            trunc = True
        return obs, r, term, trunc, info


class EarlyGymEnv(FakeGymEnv):
    def step(self, action):
        obs, r, done, info = super().step(action)
        return obs, r, bool(done or (self.t >= 3 and float(np.asarray(action).reshape(-1)[0]) > 0)), info


def stub(m, obs):
    """Actor m's action for one observation [S] -> [A] (numpy, float32 like the device's)."""
    obs = np.asarray(obs, dtype=np.float64)
    w = np.sin(np.arange(1, 7)[:, None] * (m + 1) + np.arange(obs.shape[0])[None, :])
    return np.tanh(w @ obs / 3 + 0.3 * m - 0.2).astype(np.float32)


def stub_many(obs):
    return np.stack([np.stack([stub(m, o) for o in obs[m]]) for m in range(obs.shape[0])])


MEAN = np.linspace(-0.5, 0.5, 17)
STD = np.linspace(0.5, 1.5, 17)


def sequential_reset(m):
    """evaluation/minari/iql_eval.py:evaluate with the stub as the actor."""
    env = EarlyGymnasiumEnv(NAME)
    out = []
    for i in range(EPISODES):
        done = False
        state, _ = env.reset(seed=SEED + i)
        state = (state - MEAN) / STD
        episode_reward = 0.0
        while not done:
            state, reward, terminated, truncated, _ = env.step(stub(m, state))
            state = (state - MEAN) / STD
            done = terminated or truncated
            episode_reward += reward
        out.append(episode_reward)
    return np.asarray(out)


def sequential_chain(m):
    """evaluation/d4rl/iql_eval_median.py:evaluate with the stub as the actor."""
    env = EarlyGymEnv(NAME)
    env.seed(SEED)
    out = []
    for _ in range(EPISODES):
        state, done = env.reset(), False
        state = (state - MEAN) / STD
        episode_reward = 0.0
        while not done:
            state, reward, done, _ = env.step(stub(m, state))
            state = (state - MEAN) / STD
            episode_reward += reward
        out.append(episode_reward)
    return np.asarray(out)


@pytest.fixture(scope="module")
def want():
    got = {"reset": np.stack([sequential_reset(m) for m in range(M)]),
           "chain": np.stack([sequential_chain(m) for m in range(M)])}
    # the environment does what the test needs: lengths differ by seed and by actor
    assert len({tuple(r) for r in got["reset"]}) == M and len(set(got["reset"][0])) == EPISODES
    return got


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("lanes", (1, 3, 9))
@pytest.mark.parametrize("mode", ("reset", "chain"))
def test_scheduler_equals_the_sequential_loops(want, mode, lanes):
    from iqlpref_amd import posthoc
    make = functools.partial(EarlyGymnasiumEnv if mode == "reset" else EarlyGymEnv, NAME)
    calls = []

    def fn(obs):
        calls.append(obs.shape)
        return stub_many(obs)
    got = posthoc.evaluate_many(make, [None] * M, EPISODES, SEED, episode_seeding=mode, lanes=lanes,
                                state_mean=MEAN, state_std=STD, actions_fn=fn)
    assert got.dtype == np.float64 and got.shape == (M, EPISODES)
    np.testing.assert_array_equal(_bits(got), _bits(want[mode]))
    R = 1 if mode == "chain" else min(lanes, EPISODES)
    assert set(calls) == {(M, R, 17)}  # one call per lock step, all actors and lanes in it


def test_a_swapped_row_would_show(want):
    """The yardstick is sharp: handing actor 0's rows to actor 1 changes the result."""
    from iqlpref_amd import posthoc
    got = posthoc.evaluate_many(functools.partial(EarlyGymnasiumEnv, NAME), [None] * M, EPISODES, SEED, lanes=3,
                                state_mean=MEAN, state_std=STD, actions_fn=lambda obs: stub_many(obs)[[1, 0, 2]])
    assert not np.array_equal(got, want["reset"])


@pytest.mark.parametrize("mode", ("reset", "chain"))
def test_worker_processes_give_the_same_numbers(want, mode):
    """workers=2, with the stub forward and no GPU."""
    from iqlpref_amd import posthoc
    make = functools.partial(EarlyGymnasiumEnv if mode == "reset" else EarlyGymEnv, NAME)
    got = posthoc.evaluate_many(make, [None] * M, EPISODES, SEED, episode_seeding=mode, lanes=3, workers=2,
                                state_mean=MEAN, state_std=STD, actions_fn=stub_many)
    np.testing.assert_array_equal(_bits(got), _bits(want[mode]))


class ProbeEnv:
    """Reports, as its first observation, what the process that holds it has imported."""

    def reset(self, seed=None):
        import sys
        mods = [m for m in sys.modules if m == "iqlpref_amd" or m.startswith("iqlpref_amd.")]
        return np.array([float(len(mods)), float("torch" in sys.modules), float("iqlpref_amd._lib" in sys.modules)]), {}

    def step(self, action):
        return np.zeros(3), 0.0, True, False, {}


def test_workers_hold_environments_only():
    """A worker is a fresh interpreter that runs _env_worker.py by path: it imports nothing of the package --
    so neither torch nor the binding, and the library and the device are out of its reach -- and is gone
    after close().  (Unpickling ProbeEnv imports this test module, which imports the package only inside its
    test functions.)"""
    from iqlpref_amd import _env_worker, posthoc
    lanes = posthoc._WorkerLanes(ProbeEnv, 3, 2, 0.0, 1.0)
    try:
        assert len(lanes.procs) == 2
        got = lanes.reset([(0, 1), (1, 2), (2, 3)])
        assert [list(o) for o in got] == [[0.0, 0.0, 0.0]] * 3
    finally:
        lanes.close()
    assert all(p.poll() == 0 for p in lanes.procs)
    # the module itself needs nothing beyond the standard library
    import ast
    tree = ast.parse(open(_env_worker.__file__).read())
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | \
               {n.module.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 0}
    assert imported <= {"sys", "pickle", "traceback", "multiprocessing"}
    assert not any(isinstance(n, ast.ImportFrom) and n.level for n in ast.walk(tree))
    # one wrapper for the training loops and the workers
    import iqlpref_amd as ia
    assert ia.wrap_env is _env_worker.wrap_env


def test_workers_refuse_an_unpicklable_factory_and_report_a_failing_one():
    from iqlpref_amd import posthoc
    with pytest.raises(TypeError, match="picklable make_env"):
        posthoc._WorkerLanes(lambda: ProbeEnv(), 1, 1, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="KeyError"):  # fake_envs.DIMS has no such name: raised in the worker
        posthoc._WorkerLanes(functools.partial(FakeGymnasiumEnv, "no-such-env"), 1, 1, 0.0, 1.0)


def test_the_default_factories_are_picklable_and_never_fetch(monkeypatch, tmp_path):
    """What run() hands to the workers when it looks the environment up by name, with minari / gym / d4rl
    stubbed: both factories pickle (by name, without the dataset), the Minari one never calls
    download_dataset, and the d4rl one refuses a dataset file that is not cached rather than let
    env.get_dataset() fetch it."""
    import pickle
    import sys
    import types
    from iqlpref_amd import posthoc
    calls = []

    class Episode:
        observations = np.arange(12, dtype=np.float64).reshape(4, 3)

    class Dataset(list):
        def recover_environment(self):
            calls.append("recover")
            return "minari-env"
    minari = types.ModuleType("minari")
    minari.load_dataset = lambda name: calls.append(("load", name)) or Dataset([Episode(), Episode()])
    minari.download_dataset = lambda name: calls.append("download")
    minari.get_normalized_score = lambda dataset, scores: scores / 2
    monkeypatch.setitem(sys.modules, "minari", minari)
    make, observations, norm = posthoc._minari_source("D4RL/pen/cloned-v2")
    assert observations.shape == (6, 3) and observations.dtype == np.float32 and norm(np.array([4.0]))[0] == 2.0
    again = pickle.loads(pickle.dumps(make))
    assert again() == "minari-env" and "download" not in calls and calls.count(("load", "D4RL/pen/cloned-v2")) == 2

    cached = tmp_path / "cached.hdf5"

    class Env:
        dataset_url = "http://host/cached.hdf5"
        closed = 0

        @property
        def unwrapped(self):
            return self

        def get_dataset(self, h5path=None):
            assert h5path == str(cached), "get_dataset() without a path would fetch"
            return {"observations": np.ones((5, 2), np.float32)}

        def close(self):
            Env.closed += 1
    gym = types.ModuleType("gym")
    gym.make = lambda name: Env()
    d4rl = types.ModuleType("d4rl")
    d4rl.qlearning_dataset = lambda env, dataset=None: dataset
    offline_env = types.ModuleType("d4rl.offline_env")
    offline_env.filepath_from_url = lambda url: str(tmp_path / url.split("/")[-1])
    d4rl.offline_env = offline_env
    for name, mod in (("gym", gym), ("d4rl", d4rl), ("d4rl.offline_env", offline_env)):
        monkeypatch.setitem(sys.modules, name, mod)
    with pytest.raises(FileNotFoundError, match="never fetches"):
        posthoc._d4rl_source("antmaze-large-play-v2")
    assert Env.closed == 1
    cached.write_bytes(b"")
    make, observations, norm = posthoc._d4rl_source("antmaze-large-play-v2")
    assert observations.shape == (5, 2) and norm is None and Env.closed == 2
    assert isinstance(pickle.loads(pickle.dumps(make))(), Env)


def test_run_writes_finished_rows_before_a_later_group_fails(tmp_path, monkeypatch):
    """Rows go out in file order as soon as every run before them is done: the first group's rows are in the
    file when the second group's evaluation raises."""
    from iqlpref_amd import posthoc
    spec = {"program": "evaluation/minari/iql_eval_median.py", "method": "grid",
            "parameters": {"eval_csv": {"value": str(tmp_path / "out.csv")}, "normalize_state": {"value": False},
                           "eval_episodes": {"value": 3}, "iql_deterministic": {"values": [False, True]},
                           "actor_path": {"values": ["r/run-aa/checkpoint_1.pt", "r/run-aa/checkpoint_2.pt"]}}}
    configs = posthoc.expand_eval_sweep(spec)
    assert posthoc.plan(configs) == [[0, 1], [2, 3]]

    class Spaces(ProbeEnv):
        observation_space = type("B", (), {"shape": (3,)})()
        action_space = type("B", (), {"shape": (2,), "high": np.ones(2)})()
    monkeypatch.setattr(posthoc, "load_actor", lambda path, *a, **k: path)
    groups = []

    def evaluate_many(make_env, actors, num_episodes, seed, **kw):
        groups.append(list(actors))
        if len(groups) == 2:
            raise RuntimeError("second group")
        return np.array([[1.0, 2.0, 6.0], [3.0, 4.0, 5.0]])
    monkeypatch.setattr(posthoc, "evaluate_many", evaluate_many)
    with pytest.raises(RuntimeError, match="second group"):
        posthoc.run(configs, make_env=Spaces, log=lambda s: None)
    assert open(tmp_path / "out.csv").read().splitlines() == [
        "dataset,model_id,checkpoint_id,median_score,num_episodes",
        "D4RL/pen/human-v2,aa,1,2.0,3", "D4RL/pen/human-v2,aa,2,4.0,3"]
    # --only leaves gaps that do not hold later rows back
    groups.clear()
    os.remove(tmp_path / "out.csv")
    got = posthoc.run(configs, make_env=Spaces, log=lambda s: None, only=[1, 0])
    assert got[2] is None and got[3] is None and len(open(tmp_path / "out.csv").read().splitlines()) == 3


def test_evaluate_many_argument_checks():
    from iqlpref_amd import posthoc
    make = functools.partial(EarlyGymnasiumEnv, NAME)
    with pytest.raises(ValueError, match="episode_seeding"):
        posthoc.evaluate_many(make, [None], 1, 0, episode_seeding="other", actions_fn=stub_many)
    with pytest.raises(ValueError, match="at least one"):
        posthoc.evaluate_many(make, [], 1, 0, actions_fn=stub_many)


# ---- grid files
def test_expand_eval_sweep():
    from iqlpref_amd import posthoc, sweep
    path = os.path.join(GOLDEN, "posthoc_eval_sweep.yaml")
    cfgs = posthoc.expand_eval_sweep(path)
    assert len(cfgs) == 4
    assert [c.actor_path for c in cfgs] == [f"~/runs/pen/cloned-v2-reduce_50/checkpoint_{t}.pt"
                                            for t in (4999, 9999, 14999, 19999)]
    for c in cfgs:
        assert c.program == "evaluation/minari/iql_eval_median.py" and (c.library, c.kind) == ("minari", "median")
        assert c.dataset_id == "D4RL/pen/cloned-v2" and c.dataset == "D4RL/pen/cloned-v2"
        assert c.eval_episodes == 5000 and isinstance(c.eval_episodes, int)
        assert c.eval_seed == 10 and c.normalize_state is True and c.iql_deterministic is False
        assert c.actor_dropout == 0.1 and c.eval_csv == "~/runs/pen/pen_cloned_eval_median.csv"
    assert posthoc.plan(cfgs) == [[0, 1, 2, 3]]
    # the training side keeps refusing such a file
    with pytest.raises(ValueError):
        sweep.expand_sweep(path)
    spec = sweep.load_sweep(path)
    d4rl = dict(spec, program="evaluation/d4rl/iql_eval_median.py",
                parameters={"env": {"value": "antmaze-large-play-v2"}, "eval_episodes": {"value": "500"},
                            "iql_deterministic": {"values": [False, True]},
                            "actor_path": {"values": ["a/IQL-x-1f/checkpoint_1.pt", "a/IQL-x-1f/checkpoint_2.pt"]}})
    cfgs = posthoc.expand_eval_sweep(d4rl)
    assert [(c.iql_deterministic, c.actor_path[-4:]) for c in cfgs] == [(False, "1.pt"), (False, "2.pt"),
                                                                        (True, "1.pt"), (True, "2.pt")]
    assert all(c.library == "d4rl" and c.dataset == "antmaze-large-play-v2" and c.eval_episodes == 500 for c in cfgs)
    assert posthoc.plan(cfgs) == [[0, 1], [2, 3]]
    text = posthoc.describe(cfgs)
    assert "4 runs" in text and "group 1" in text and "run 3: a/IQL-x-1f/checkpoint_2.pt" in text


def test_expand_eval_sweep_refusals():
    from iqlpref_amd import posthoc, sweep
    spec = sweep.load_sweep(os.path.join(GOLDEN, "posthoc_eval_sweep.yaml"))
    with pytest.raises(ValueError, match="only 'grid'"):
        posthoc.expand_eval_sweep(dict(spec, method="bayes"))
    bad = dict(spec, parameters=dict(spec["parameters"], learning_rate={"value": 1e-3}, beta={"value": 3.0}))
    with pytest.raises(ValueError, match="unknown sweep parameters") as e:
        posthoc.expand_eval_sweep(bad)
    assert "learning_rate" in str(e.value) and "beta" in str(e.value) and "eval_csv" not in str(e.value)
    for program in ("algorithms/custom_offline/iql.py", "algorithms/offline/iql.py", None):
        with pytest.raises(ValueError, match="none of the evaluation programs"):
            posthoc.expand_eval_sweep(dict(spec, program=program))
    with pytest.raises(ValueError, match="value"):
        posthoc.expand_eval_sweep(dict(spec, parameters={"actor_path": {"min": 0, "max": 1}}))
    with pytest.raises(ValueError, match="program"):
        posthoc.EvalConfig(program="evaluation/other.py")


def test_cli_list_touches_no_device(capsys):
    from iqlpref_amd import _lib, posthoc
    before = _lib._lib
    assert posthoc.main([os.path.join(GOLDEN, "posthoc_eval_sweep.yaml"), "--list", "--lanes", "4"]) == 0
    out = capsys.readouterr().out
    assert "4 runs" in out and "4 checkpoints x 5000 episodes" in out and "4 lanes each, 1 set batch" in out
    assert _lib._lib is before
    with pytest.raises(SystemExit):
        posthoc.main([os.path.join(GOLDEN, "posthoc_eval_sweep.yaml"), "--list", "--only", "4"])


def test_set_batches():
    from iqlpref_amd import _lib, posthoc
    pen = posthoc._image_floats([45, 256, 256, 24])
    assert pen == 48 * 256 + 256 + 256 * 256 + 256 + 256 * 32 + 32
    assert [list(b) for b in posthoc.set_batches(5, pen)] == [[0, 1, 2, 3, 4]]
    assert [len(b) for b in posthoc.set_batches(2500, pen)] == [1024, 1024, 452] and _lib.MLP_SET_MAX == 1024
    deep = posthoc._image_floats([256] * 9)  # 2 MiB a member: the byte bound cuts first
    assert [len(b) for b in posthoc.set_batches(1000, deep)] == [posthoc.SET_BYTES // (4 * deep)] * 1 + \
        [1000 - posthoc.SET_BYTES // (4 * deep)]


# ---- writers
SCORES = np.array([1.5, -2.25, 4.0, 0.125, 3.0])
PATH = "~/iqlpref/cloned_pen_models_pref/iql-p-D4RL/pen/cloned-v2-reduce_50/checkpoint_4999.pt"


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def test_path_ids():
    from iqlpref_amd import posthoc
    assert posthoc.path_ids(PATH) == ("reduce_50", "4999")
    assert posthoc.path_ids("~/x/IQL-antmaze-large-play-v2-4f562dfb/checkpoint_999999.pt") == ("4f562dfb", "999999")
    assert posthoc.path_ids("~/m/human-v2-0f6ecda0/best_model.pt") == ("0f6ecda0", "model")


def test_writers_byte_exact(tmp_path):
    from iqlpref_amd import posthoc
    mean_csv, median_csv, stats_csv = (str(tmp_path / n) for n in ("mean.csv", "median.csv", "stats.csv"))
    row = posthoc.write_mean_row(mean_csv, "D4RL/pen/cloned-v2", PATH, SCORES)
    assert row["std_score"] == float(np.std(SCORES, ddof=1)) != float(np.std(SCORES))
    assert row["mean_score"] == 1.275 and row["num_episodes"] == 5 and row["normalized_mean_score"] is None
    # the append case, with the normalised columns filled: normalised = (score + 3) / 10, times 100
    second = PATH.replace("4999", "9999")
    row = posthoc.write_mean_row(mean_csv, "D4RL/pen/cloned-v2", second, 2 * SCORES, lambda s: (s + 3) / 10)
    assert row["normalized_mean_score"] == float(((2 * SCORES + 3) / 10 * 100).mean())
    assert row["normalized_std_score"] == float(((2 * SCORES + 3) / 10 * 100).std(ddof=1))
    assert open(mean_csv, "rb").read() == _golden("posthoc_mean.csv")
    posthoc.write_median_row(median_csv, "D4RL/pen/cloned-v2", PATH, SCORES)
    posthoc.write_median_row(median_csv, "D4RL/pen/cloned-v2", second, 2 * SCORES)
    assert open(median_csv, "rb").read() == _golden("posthoc_median.csv")
    posthoc.write_stats(stats_csv, SCORES)
    assert open(stats_csv, "rb").read() == _golden("posthoc_stats.csv")
    posthoc.write_stats(stats_csv, SCORES)  # np.savetxt replaces
    assert open(stats_csv, "rb").read() == _golden("posthoc_stats.csv")
    # write_result routes by program
    cfg = posthoc.EvalConfig(program="evaluation/minari/iql_stats.py", eval_csv=stats_csv, actor_path=PATH)
    posthoc.write_result(cfg, SCORES)
    assert open(stats_csv, "rb").read() == _golden("posthoc_stats.csv")


# ---- the C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from iqlpref_amd import _lib
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    P, PD = C.c_void_p, C.POINTER(C.POINTER(_lib.MlpDesc))
    want = {
        # (descs[M], M, out, stream)
        "iqlhip_mlp_set_create": (C.c_int, [PD, C.c_int32, C.POINTER(P), P]),
        "iqlhip_mlp_set_destroy": (C.c_int, [P]),
        # (set, x, R, x_stride, out, out_stride, stream)
        "iqlhip_mlp_set_forward": (C.c_int, [P, P, C.c_int32, C.c_int32, P, C.c_int32, P]),
    }
    for name, (res, args) in want.items():
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args
    assert re.search(r"#define IQLHIP_MLP_SET_MAX 1024\b", header) and _lib.MLP_SET_MAX == 1024
    assert "typedef struct iqlhip_mlp_set iqlhip_mlp_set;" in header
    assert _lib.ABI_VERSION == 6 and lib.iqlhip_abi_version() == 6
    import iqlpref_amd as ia
    assert ia.posthoc.MlpSet is not None and not hasattr(ia, "MlpSet") and not hasattr(ia, "evaluate_many")
    from iqlpref_amd import build
    assert "mlp_f32.hip" in build.SOURCES


def _desc(dims, hidden_act=0, out_act=1, dropout_p=0.0, w_in_out=0):
    from iqlpref_amd import _lib
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, w in enumerate(dims):
        d.dims[i] = w
    for i in range(d.n_layers):
        d.weights[i], d.biases[i] = FAKE, FAKE
    d.hidden_act, d.out_act, d.dropout_p, d.w_in_out = hidden_act, out_act, dropout_p, w_in_out
    return d


def _create(lib, descs, n=None, null_out=False):
    from iqlpref_amd import _lib
    K = len(descs)
    arr = (C.POINTER(_lib.MlpDesc) * max(K, 1))(*[C.pointer(d) if d is not None else C.POINTER(_lib.MlpDesc)()
                                                  for d in descs])
    out = C.c_void_p()
    rc = lib.iqlhip_mlp_set_create(arr, K if n is None else n, None if null_out else C.byref(out), None)
    return rc, lib.iqlhip_last_error().decode(), out.value


def test_create_refusals_before_any_hip_call(lib):
    from iqlpref_amd import _lib
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    good = _desc([45, 256, 256, 24])
    nine = _desc([8, 8, 8])
    nine.n_layers = 9
    null_w = _desc([45, 64, 24])
    null_w.biases[1] = None
    many = [good] * 1025
    cases = [
        ("M = 0", _create(lib, [good], n=0), INV, "M = 0"),
        ("M = 1025", _create(lib, many), INV, "M = 1025"),
        ("other width", _create(lib, [good, _desc([45, 256, 128, 24])]), INV, "member 1 differs"),
        ("other depth", _create(lib, [good, good, _desc([45, 256, 24])]), INV, "member 2 differs"),
        ("other activation", _create(lib, [good, _desc([45, 256, 256, 24], hidden_act=1)]), INV, "member 1 differs"),
        ("other output activation", _create(lib, [good, _desc([45, 256, 256, 24], out_act=0)]), INV, "differs"),
        ("other layout", _create(lib, [good, _desc([45, 256, 256, 24], w_in_out=1)]), INV, "differs"),
        ("width 257", _create(lib, [_desc([45, 257, 24])]), UNS, "257 > 256"),
        ("input 257", _create(lib, [_desc([257, 16, 2])]), UNS, "257 > 256"),
        ("output 300", _create(lib, [_desc([8, 16, 300])] * 2), UNS, "300 > 256"),
        ("width 0", _create(lib, [_desc([8, 0, 2])]), INV, "width 0"),
        ("dropout", _create(lib, [good, _desc([45, 256, 256, 24], dropout_p=0.1)]), UNS, "member 1: dropout_p > 0"),
        ("9 layers", _create(lib, [nine]), INV, "n_layers"),
        ("activation code 5", _create(lib, [_desc([8, 8, 2], hidden_act=5)]), INV, "activation code 5"),
        ("null member", _create(lib, [good, None]), INV, "member 1: null descriptor"),
        ("null weight", _create(lib, [null_w]), INV, "null weight pointer"),
        ("null out", _create(lib, [good], null_out=True), INV, "null argument"),
    ]
    for what, (rc, msg, out), code, text in cases:
        assert rc == code and text in msg, (what, rc, msg)
        assert out is None, what  # *out stays null
    out = C.c_void_p()
    assert lib.iqlhip_mlp_set_create(None, 1, C.byref(out), None) == INV and out.value is None
    assert lib.iqlhip_mlp_set_destroy(None) == INV


def test_forward_refuses_null_arguments(lib):
    from iqlpref_amd import _lib
    assert lib.iqlhip_mlp_set_forward(None, FAKE, 1, 8, FAKE, 8, None) == _lib.ERR_INVALID
    assert "null" in lib.iqlhip_last_error().decode()
