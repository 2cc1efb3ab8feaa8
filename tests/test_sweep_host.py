"""Sweep grids (iqlpref_amd.sweep) on the host: expanding W&B grid files into configs, the checks
train_runs makes before any device work, launch batches and the rank share.  No GPU."""
import os

import pytest
import yaml

from iqlpref_amd import TrainConfig
from iqlpref_amd import sweep as sw


def _write(path, obj):
    path.write_text(yaml.safe_dump(obj, sort_keys=False))
    return str(path)


@pytest.fixture
def base(tmp_path):
    """A base config as the reference's configs/offline/iql/*.yaml write them (3e-4 and false for
    typed fields)."""
    (tmp_path / "cfgs").mkdir()
    _write(tmp_path / "cfgs" / "antmaze.yaml",
           {"env": "antmaze-medium-play-v2", "batch_size": 256, "beta": 10.0, "iql_tau": 0.9,
            "normalize_reward": 1, "max_timesteps": 1000000.0, "qf_lr": "3e-4", "eval_freq": 100000,
            "iql_deterministic": "false", "name": "IQL"})
    return tmp_path


def test_grid_order_last_parameter_fastest(base):
    spec = {"project": "IQL-pref", "program": "algorithms/offline/iql.py", "method": "grid",
            "parameters": {"config_path": {"value": "cfgs/antmaze.yaml"},
                           "seed": {"values": [1, 2, 3]},
                           "normalize_reward": {"values": [0, 7]},
                           "beta": {"value": 3.0}}}
    cfgs = sw.expand_sweep(_write(base / "s.yaml", spec), config_root=str(base))
    assert len(cfgs) == 6
    assert [(c.seed, c.normalize_reward) for c in cfgs] == [(1, 0), (1, 7), (2, 0), (2, 7), (3, 0), (3, 7)]
    assert [c.sweep_label for c in cfgs[:2]] == ["seed=1,normalize_reward=0", "seed=1,normalize_reward=7"]
    for c in cfgs:
        assert c.env == "antmaze-medium-play-v2" and c.batch_size == 256 and c.iql_tau == 0.9
        assert c.beta == 3.0  # the sweep's single value overrides the base YAML's 10.0
        assert c.max_timesteps == 1_000_000 and isinstance(c.max_timesteps, int)
        assert c.qf_lr == 3e-4 and c.iql_deterministic is False
    # a mapping works as well as a path
    assert [c.seed for c in sw.expand_sweep(spec, config_root=str(base))] == [1, 1, 2, 2, 3, 3]


def test_overrides_beat_sweep_and_base_and_are_coerced(base):
    spec = {"method": "grid", "parameters": {"config_path": {"value": "cfgs/antmaze.yaml"},
                                             "seed": {"values": [0, 1]}, "beta": {"value": 3.0}}}
    cfgs = sw.expand_sweep(spec, config_root=str(base), beta="5", max_timesteps="40", normalize="false",
                           seed="9")
    assert len(cfgs) == 2  # the grid's shape stays; the override fixes the value
    for c in cfgs:
        assert c.beta == 5.0 and c.max_timesteps == 40 and c.normalize is False and c.seed == 9
        assert c.sweep_label == ""  # nothing varies any more


def test_config_path_as_a_list_of_values(base):
    _write(base / "cfgs" / "pen.yaml", {"env": "pen-human-v1", "actor_dropout": 0.1, "batch_size": 128})
    spec = {"method": "grid", "parameters": {"config_path": {"values": ["cfgs/antmaze.yaml", "cfgs/pen.yaml"]},
                                             "seed": {"values": [4, 5]}}}
    cfgs = sw.expand_sweep(spec, config_root=str(base))
    assert [(c.env, c.seed) for c in cfgs] == [("antmaze-medium-play-v2", 4), ("antmaze-medium-play-v2", 5),
                                               ("pen-human-v1", 4), ("pen-human-v1", 5)]
    assert cfgs[2].actor_dropout == 0.1 and cfgs[2].batch_size == 128 and cfgs[0].actor_dropout is None
    assert cfgs[3].sweep_label == "config_path=cfgs/pen.yaml,seed=5"


def test_no_config_path_uses_the_defaults():
    cfgs = sw.expand_sweep({"method": "grid", "parameters": {"iql_tau": {"values": [0.7, 0.9]}}})
    assert [c.iql_tau for c in cfgs] == [0.7, 0.9] and cfgs[0].env == TrainConfig.env


def test_reward_model_root_times_seeds():
    spec = {"method": "grid", "parameters": {"reward_model_root": {"value": "~/mr/antmaze_mr_eval"},
                                             "query_length": {"value": 1}, "seed": {"values": [1, 2, 3]},
                                             "normalize_reward": {"value": 7}}}
    cfgs = sw.expand_sweep(spec)
    assert [c.reward_model_path for c in cfgs] == [f"~/mr/antmaze_mr_eval_{s}" for s in (1, 2, 3)]
    assert {c.normalize_reward for c in cfgs} == {7}


@pytest.mark.parametrize("spec, words", [
    ({"method": "random", "parameters": {"seed": {"values": [1]}}}, ["random", "grid"]),
    ({"method": "bayes", "parameters": {"seed": {"values": [1]}}}, ["bayes"]),
    ({"parameters": {"seed": {"values": [1]}}}, ["None"]),
    ({"method": "grid", "parameters": {"beta": {"distribution": "uniform", "min": 1, "max": 3}}}, ["beta"]),
    ({"method": "grid", "parameters": {"beta": {"min": 1, "max": 3}}}, ["beta"]),
    ({"method": "grid", "parameters": {"beta": {"values": [1.0], "distribution": "uniform"}}}, ["beta"]),
    ({"method": "grid", "parameters": {"opt": {"parameters": {"lr": {"value": 1}}}}}, ["opt"]),
    ({"method": "grid", "parameters": {"seed": {"values": []}}}, ["seed"]),
    ({"method": "grid", "parameters": {"seed": 3}}, ["seed"]),
    ({"method": "grid", "early_terminate": {"type": "hyperband"}, "parameters": {}}, ["early_terminate"]),
])
def test_unsupported_sweeps_raise(spec, words):
    with pytest.raises(ValueError) as e:
        sw.expand_sweep(spec)
    for w in words:
        assert w in str(e.value)


def test_unknown_names_are_listed_together():
    spec = {"method": "grid", "parameters": {"seed": {"values": [1, 2]}, "learning_rate": {"value": 1e-3},
                                             "beta": {"value": 3.0}, "eval_episodes": {"value": 10}}}
    with pytest.raises(ValueError) as e:
        sw.expand_sweep(spec)
    assert "learning_rate" in str(e.value) and "eval_episodes" in str(e.value) and "beta" not in str(e.value)
    with pytest.raises(ValueError, match="not_a_field"):
        sw.expand_sweep({"method": "grid", "parameters": {}}, not_a_field=1)


def test_labels_and_ignored_top_level_keys():
    spec = {"method": "grid", "project": "p", "program": "x.py", "name": "n", "description": "d",
            "metric": {"name": "mean_score", "goal": "maximize"}, "command": ["${env}", "python"],
            "parameters": {"seed": {"values": [0, 1]}}}
    assert [c.seed for c in sw.expand_sweep(spec)] == [0, 1]


def _cfg(**kw):
    return TrainConfig(device="cuda", **kw)


def test_duplicate_checkpoints_path_and_bad_runs_per_gpu_raise_before_device_work(tmp_path):
    a, b = _cfg(seed=0), _cfg(seed=1)
    a.checkpoints_path = b.checkpoints_path = str(tmp_path / "same")
    with pytest.raises(ValueError, match="checkpoints_path"):
        sw.train_runs([a, b], env=object(), dataset={})
    ok = [_cfg(seed=0, checkpoints_path=str(tmp_path)), _cfg(seed=1, checkpoints_path=str(tmp_path))]
    assert ok[0].checkpoints_path != ok[1].checkpoints_path  # (TrainConfig appends the run's unique name)
    sw.check_runs(ok, 8)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="runs_per_gpu"):
            sw.train_runs([_cfg()], env=object(), dataset={}, runs_per_gpu=k)
        with pytest.raises(ValueError, match="runs_per_gpu"):
            sw.plan_batches([_cfg()], [(29, 8)], k)
    with pytest.raises(ValueError, match="evaluate"):
        sw.train_runs([_cfg(), _cfg()], env=object(), dataset={}, evaluate=[lambda a, t: None])


def test_start_runs_checks_in_order_and_deals_the_configs(tmp_path, monkeypatch):
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    cfgs = [_cfg(seed=s) for s in range(5)]
    assert sw.start_runs(cfgs, 8, None, False) == ([0, 1, 2, 3, 4], [1, 3])
    assert sw.start_runs(cfgs, 8, ["7", 8, 9, 10, 11], False) == ([7, 8, 9, 10, 11], [1, 3])
    with pytest.raises(ValueError, match="run_ids"):
        sw.start_runs(cfgs, 8, [0, 1], False)
    with pytest.raises(ValueError, match="runs_per_gpu"):  # ahead of the run_ids check
        sw.start_runs(cfgs, 0, [0, 1], False)
    with pytest.raises(ValueError, match="checkpoints_path"):  # resume: every config needs a directory
        sw.start_runs(cfgs, 8, [0, 1], True)


def test_batch_cache_builds_on_first_need_and_drops_after_the_last_batch():
    batches = [[0, 1], [2], [3, 4]]
    keys = {0: "a", 1: "b", 2: "a", 3: "c", 4: "b"}  # a: batches 0-1, b: 0-2, c: 2
    cache, built = sw.BatchCache(batches, keys.__getitem__), []
    assert cache.key_of == keys

    def get(i):
        return cache.get(i, lambda: built.append(keys[i]) or [keys[i]])

    held = []
    for bi, batch in enumerate(batches):
        values = [get(i) for i in batch]
        assert [v[0] for v in values] == [keys[i] for i in batch]
        assert get(batch[0]) is values[0]  # the same object for every run of the key
        cache.batch_done(bi)
        held.append([k for k in "abc" if k in cache])
    assert built == ["a", "b", "c"]  # each once, in the order first needed
    assert held == [["a", "b"], ["b"], []]  # gone right after the last batch that uses it


def test_one_env_object_for_two_env_names_raises():
    cfgs = [_cfg(env="antmaze-medium-play-v2"), _cfg(env="antmaze-large-play-v2")]
    with pytest.raises(ValueError, match="environments"):
        sw.train_runs(cfgs, env=object(), dataset={})
    e1, e2 = object(), object()
    assert sw._resolve_envs(cfgs, [0, 1], {"antmaze-medium-play-v2": e1, "antmaze-large-play-v2": e2}) == \
        {"antmaze-medium-play-v2": e1, "antmaze-large-play-v2": e2}


def test_plan_batches_splits_on_every_shape_field_and_caps_size():
    same = [_cfg(seed=s) for s in range(5)]
    assert sw.plan_batches(same, [(29, 8)] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert sw.plan_batches(same, [(29, 8)] * 5, 8) == [[0, 1, 2, 3, 4]]
    assert sw.plan_batches(same, [(29, 8)] * 5, 1) == [[0], [1], [2], [3], [4]]
    # everything that is not shape stays inside one batch
    mixed = [_cfg(seed=1, normalize_reward=3, beta=1.0, iql_tau=0.6, discount=0.9, tau=0.01, vf_lr=1e-4,
                  qf_lr=2e-4, actor_lr=5e-4, actor_dropout=0.25, max_timesteps=10, log_freq=5, eval_freq=7,
                  reward_model_path="x"),
             _cfg(seed=2, actor_dropout=0.1)]
    assert sw.plan_batches(mixed, [(45, 24)] * 2, 8) == [[0, 1]]
    variants = {
        "dims": ({}, (17, 6)),
        "batch_size": ({"batch_size": 128}, None),
        "iql_deterministic": ({"iql_deterministic": True}, None),
        "dropout": ({"actor_dropout": 0.1}, None),
        "n_critics": ({"n_critics": 4}, None),
        "device": ({"device": "cuda:1"}, None),
    }
    for what, (kw, dims) in variants.items():
        kw = dict(kw)
        dev = kw.pop("device", "cuda")
        cfgs = [_cfg(), TrainConfig(device=dev, **kw), _cfg(), TrainConfig(device=dev, **kw)]
        d = [(29, 8), dims or (29, 8), (29, 8), dims or (29, 8)]
        assert sw.plan_batches(cfgs, d, 8) == [[0, 2], [1, 3]], what
    # precision is part of the key as well
    assert sw.shape_key(_cfg(), (29, 8), "bf16") != sw.shape_key(_cfg(), (29, 8), "fp32")
    # a mapping env name -> dims; unknown dims fall back to the env name
    cfgs = [_cfg(env="antmaze-medium-play-v2"), _cfg(env="pen-human-v1"), _cfg(env="antmaze-large-play-v2")]
    assert sw.plan_batches(cfgs, {"antmaze-medium-play-v2": (29, 8), "pen-human-v1": (45, 24),
                                  "antmaze-large-play-v2": (29, 8)}, 8) == [[0, 2], [1]]
    assert sw.plan_batches(cfgs, [None] * 3, 8) == [[0], [1], [2]]


def test_configs_are_dealt_over_ranks():
    assert sw.rank_share(10, 0, 1) == list(range(10))
    assert sw.rank_share(10, 0, 3) == [0, 3, 6, 9]
    assert sw.rank_share(10, 1, 3) == [1, 4, 7]
    assert sw.rank_share(10, 2, 3) == [2, 5, 8]
    assert sw.rank_share(2, 3, 4) == []
    dealt = sorted(i for r in range(4) for i in sw.rank_share(13, r, 4))
    assert dealt == list(range(13))


def test_rank_world_from_the_environment(monkeypatch):
    monkeypatch.setenv("RANK", "2")
    monkeypatch.setenv("WORLD_SIZE", "3")
    assert sw._rank_world() == (2, 3)


def test_main_list(base, capsys, monkeypatch):
    monkeypatch.delenv("AGENTS_PER_GPU", raising=False)
    _write(base / "cfgs" / "pen.yaml", {"env": "pen-human-v1", "actor_dropout": 0.1, "batch_size": 256})
    spec = {"project": "IQL-pref", "method": "grid",
            "parameters": {"config_path": {"values": ["cfgs/antmaze.yaml", "cfgs/pen.yaml"]},
                           "seed": {"value": 0}, "normalize_reward": {"values": [0, 1, 2]}}}
    path = _write(base / "sweep_x.yaml", spec)
    sw.main([path, "--config_root", str(base), "--list", "--runs_per_gpu", "2"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split("\t") for ln in lines] == [
        ["0", "config_path=cfgs/antmaze.yaml,normalize_reward=0", "batch 0"],
        ["1", "config_path=cfgs/antmaze.yaml,normalize_reward=1", "batch 0"],
        ["2", "config_path=cfgs/antmaze.yaml,normalize_reward=2", "batch 1"],
        ["3", "config_path=cfgs/pen.yaml,normalize_reward=0", "batch 2"],
        ["4", "config_path=cfgs/pen.yaml,normalize_reward=1", "batch 2"],
        ["5", "config_path=cfgs/pen.yaml,normalize_reward=2", "batch 3"]]
    # --only, an override (batch_size splits the antmaze runs off the pen runs anyway), the default K = 8
    sw.main([path, "--config_root", str(base), "--list", "--only", "1,4,5", "--batch_size", "64"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split("\t")[0::2] for ln in lines] == [["1", "batch 0"], ["4", "batch 1"], ["5", "batch 1"]]
    # AGENTS_PER_GPU is the default of --runs_per_gpu
    monkeypatch.setenv("AGENTS_PER_GPU", "1")
    sw.main([path, "--config_root", str(base), "--list", "--only", "0,1"])
    assert [ln.split("\t")[2] for ln in capsys.readouterr().out.strip().splitlines()] == ["batch 0", "batch 1"]
    with pytest.raises(ValueError, match="runs_per_gpu"):
        sw.main([path, "--config_root", str(base), "--list", "--runs_per_gpu", "17"])


def test_package_exports():
    import iqlpref_amd as ia
    assert ia.expand_sweep is sw.expand_sweep and ia.train_runs is sw.train_runs
    assert os.path.basename(sw.__file__) == "sweep.py"
