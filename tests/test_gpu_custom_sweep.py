"""custom_offline.train_runs: the runs of a pen sweep grid packed into seed groups.  -m gpu.

Every run is compared with ``custom_offline.train()`` of its config alone, in this process, on a fresh
dataset and a fresh copy of its reward model.  "Equal" is exact: ``torch.equal`` on parameters, target, Adam
moments and every tensor of every checkpoint file, ``==`` on ``total_it``, the actor learning rate, the
scheduler state and the logged records (as a sequence of (record without ``run``, step)).

Pen dims (the flavour fixes 2 x 256 nets), batch 32 (two 16-row slabs), episodes of 23 + 17 + 30 steps,
at most 60 update steps with an evaluation of two episodes every 20.
"""
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch
import yaml

from tests import custom_train_env as cte

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, A = 45, 24
LENGTHS = (23, 17, 30)
# a dataset id whose rewards modify_reward() rewrites (antmaze: -1), so that normalize_reward changes the buffer
SHIFTED_ID = "standin/antmaze-rewards/pen-v0"
# the four runs of tests 1 and 5: (reward-model seed, config fields); three models, one train_seed
FOUR = [(5, {}),
        (6, {"beta": 5.0, "iql_tau": 0.9}),
        (7, {"update_steps": 40}),
        (5, {"normalize_reward": True, "dataset_id": SHIFTED_ID})]


def _dataset(seed=11, lengths=LENGTHS):
    return cte.MinariDataset(seed, lengths)


def _qmlp(seed):
    from iqlpref_amd import custom_offline as co
    return co.QMLP(S, A, (32,), "relu", "none").load_flax_params(cte.reward_layers(seed, S, A)).to(DEV)


def _pt(seed):
    from iqlpref_amd.relabel import RewardPT
    torch.manual_seed(seed)
    return RewardPT(S, A, 50, embd_dim=64, num_heads=4, intermediate_dim=256, num_layers=1, max_pos=64).to(DEV)


def _config(tmp, path, **kw):
    from iqlpref_amd import custom_offline as co
    base = dict(update_steps=60, eval_every=20, batch_size=32, eval_episodes=2, eval_seed=4, train_seed=3,
                actor_dropout=0.1, reward_model_path=path, checkpoints_path=str(tmp))
    base.update(kw)
    return co.TrainConfig(**base)


def _normalized(ds, returns):
    return 0.5 + 2.0 * np.asarray(returns)


def _files(config):
    """Every checkpoint file of a run, loaded: {name: state dict}."""
    names = sorted(f for f in os.listdir(config.checkpoints_path) if f.endswith(".pt"))
    return {f: torch.load(os.path.join(config.checkpoints_path, f), weights_only=True) for f in names}


def _result(config, records, trainer):
    return {"config": config, "records": records, "trainer": trainer, "files": _files(config)}


def _solo(config, dataset, model, **kw):
    from iqlpref_amd import custom_offline as co
    records = []
    trainer = co.train(config, dataset, model, logger=lambda d, step: records.append((dict(d), int(step))),
                       normalized_score=_normalized, device=DEV, **kw)
    return _result(config, records, trainer)


def _runs(configs, dataset, models, **kw):
    from iqlpref_amd import custom_offline as co
    records = [[] for _ in configs]

    def logger(d, step):
        d = dict(d)
        records[d.pop("run")].append((d, int(step)))

    trainers = co.train_runs(configs, dataset, models, logger=logger, normalized_score=_normalized, **kw)
    assert len(trainers) == len(configs)
    return [_result(c, r, t) for c, r, t in zip(configs, records, trainers)]


def _same(a, b, where):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}/{i}")
    else:
        assert a == b, where


def _assert_equal_runs(got, want, what):
    a, b = got["trainer"], want["trainer"]
    assert a.total_it == b.total_it == got["config"].update_steps, what
    _same(a.state_dict(), b.state_dict(), f"{what}: state")  # nets, Adam moments and steps, scheduler
    for p, q in zip(a.q_target.parameters(), b.q_target.parameters()):
        assert torch.equal(p, q), f"{what}: target"
    assert a.actor_optimizer.param_groups[0]["lr"] == b.actor_optimizer.param_groups[0]["lr"], what
    assert len(got["records"]) == len(want["records"]), what
    assert got["records"] == want["records"], f"{what}: records"
    assert list(got["files"]) == list(want["files"]) and "best_model.pt" in got["files"], what
    n_evals = got["config"].update_steps // got["config"].eval_every
    assert len(got["files"]) == 1 + n_evals, what
    _same(got["files"], want["files"], f"{what}: files")


def _four_configs(tmp, paths=("m5", "m6", "m7", "m5")):
    return [_config(tmp / f"run{i}", path, **kw) for i, (path, (_, kw)) in enumerate(zip(paths, FOUR))]


@pytest.fixture(scope="module")
def solo4(tmp_path_factory):
    """The four runs of FOUR, each through train() alone (the reference of tests 1 and 5)."""
    tmp = tmp_path_factory.mktemp("solo4")
    return [_solo(cfg, _dataset(), _qmlp(seed)) for cfg, (seed, _) in zip(_four_configs(tmp), FOUR)]


@pytest.fixture(scope="module")
def group4(tmp_path_factory):
    """The same four as one launch batch with handed-in models."""
    tmp = tmp_path_factory.mktemp("group4")
    return _runs(_four_configs(tmp), _dataset(), {f"m{s}": _qmlp(s) for s in (5, 6, 7)}, runs_per_gpu=8)


def test_four_runs_equal_their_solo_runs(solo4, group4, tmp_path):
    """Three reward models at one train_seed; one run differs in beta and iql_tau, one ends at step 40 (the
    group is rebuilt once), one normalises its rewards.  As one batch of four and as two batches of two."""
    assert len({id(r["trainer"]) for r in group4}) == 4
    for i, (g, s) in enumerate(zip(group4, solo4)):
        _assert_equal_runs(g, s, f"run {i}, one batch")
    # the runs do differ from one another: what is compared is not one result four times
    assert group4[0]["records"] != group4[1]["records"] and group4[0]["records"] != group4[3]["records"]
    assert len([r for r in group4[2]["records"] if "value_loss" in r[0]]) == 40
    assert [s for r, s in group4[0]["records"] if "value_loss" in r] == list(range(60))
    two = _runs(_four_configs(tmp_path), _dataset(), {f"m{s}": _qmlp(s) for s in (5, 6, 7)}, runs_per_gpu=2)
    for i, (g, s) in enumerate(zip(two, solo4)):
        _assert_equal_runs(g, s, f"run {i}, two batches")


def test_relabel_and_buffer_sharing(tmp_path, monkeypatch):
    from iqlpref_amd import custom_offline as co
    calls = {"relabel": 0, "load": 0}
    real_relabel, real_load = co.qlearning_dataset, co.ReplayBuffer.load_dataset

    def relabel(*a, **k):
        calls["relabel"] += 1
        return real_relabel(*a, **k)

    def load(self, data):
        calls["load"] += 1
        return real_load(self, data)

    monkeypatch.setattr(co, "qlearning_dataset", relabel)
    monkeypatch.setattr(co.ReplayBuffer, "load_dataset", load)

    def configs(tmp, **last):
        cs = [_config(tmp / f"r{i}", path, beta=beta, update_steps=20) for i, (path, beta) in
              enumerate((("m5", 3.0), ("m5", 5.0), ("m6", 3.0), ("m6", 5.0)))]
        for k, v in last.items():
            setattr(cs[-1], k, v)
        return cs

    models = {"m5": _qmlp(5), "m6": _qmlp(6)}
    out = _runs(configs(tmp_path / "a"), _dataset(), models)
    assert calls == {"relabel": 2, "load": 2}
    assert out[0]["records"] != out[1]["records"]  # (beta tells the two runs of one buffer apart)
    calls.update(relabel=0, load=0)
    out2 = _runs(configs(tmp_path / "b", normalize_state=False), _dataset(), models)
    assert calls == {"relabel": 2, "load": 3}
    for i in range(3):  # the runs whose preparation did not change train as before
        assert out2[i]["records"] == out[i]["records"], i
    assert out2[3]["records"] != out[3]["records"]


def test_two_datasets_in_one_batch_each_below_its_own_bound(tmp_path, monkeypatch):
    from iqlpref_amd import custom_offline as co
    ids = ("D4RL/pen/human-v2", "D4RL/pen/expert-v2")
    lengths = {ids[0]: LENGTHS, ids[1]: (40, 9, 25, 31)}
    data = lambda: {ids[0]: _dataset(11, lengths[ids[0]]), ids[1]: _dataset(12, lengths[ids[1]])}
    spec = [(ids[0], 5, {}), (ids[1], 6, {}), (ids[1], 5, {"train_seed": 4})]

    def configs(tmp):
        return [_config(tmp / f"r{i}", f"m{seed}", dataset_id=d, update_steps=40, **kw)
                for i, (d, seed, kw) in enumerate(spec)]

    solo = [_solo(cfg, data()[d], _qmlp(seed)) for cfg, (d, seed, _) in zip(configs(tmp_path / "solo"), spec)]
    drawn = []
    real_draw = co.NumpyIndexStream.draw

    def draw(self, hi, n_batches, batch_size, generators=None):
        out = real_draw(self, hi, n_batches, batch_size, generators)
        drawn.append(([int(h) for h in hi], [int(t.max()) for t in out], [int(t.min()) for t in out]))
        return out

    monkeypatch.setattr(co.NumpyIndexStream, "draw", draw)
    models = lambda: {"m5": _qmlp(5), "m6": _qmlp(6)}
    dev = _runs(configs(tmp_path / "dev"), data(), models(), sampler="device")
    monkeypatch.setattr(co.NumpyIndexStream, "draw", real_draw)
    assert drawn and all(his == [70, 105, 105] for his, _, _ in drawn)  # one K = 3 draw per call, unequal bounds
    for his, tops, lows in drawn:
        assert all(0 <= lo and top < hi for hi, top, lo in zip(his, tops, lows))
    assert max(t[1] for _, t, _ in drawn) >= 70  # the longer dataset is drawn from beyond the shorter one's end
    host = _runs(configs(tmp_path / "host"), data(), models(), sampler="host")
    for i in range(3):
        _assert_equal_runs(dev[i], solo[i], f"run {i}, device sampler")
        _assert_equal_runs(host[i], solo[i], f"run {i}, host sampler")
    assert dev[1]["records"] != dev[2]["records"]


def test_preference_transformer_relabel_in_one_batch(tmp_path):
    """query_length 5: the per-episode window relabel of two small RewardPTs (one block, embd_dim 64)."""
    def configs(tmp):
        return [_config(tmp / f"r{i}", f"pt{seed}", query_length=5, update_steps=20) for i, seed in enumerate((1, 2))]

    solo = [_solo(cfg, _dataset(), _pt(seed)) for cfg, seed in zip(configs(tmp_path / "solo"), (1, 2))]
    both = _runs(configs(tmp_path / "both"), _dataset(), {"pt1": _pt(1), "pt2": _pt(2)})
    for i in range(2):
        _assert_equal_runs(both[i], solo[i], f"run {i}")
    assert both[0]["records"] != both[1]["records"]


def test_models_read_from_npz_files_beside_the_checkpoint_path(group4, tmp_path):
    from iqlpref_amd import custom_offline as co
    for seed in (5, 6, 7):
        co.save_reward_params(tmp_path / f"m{seed}.ckpt.npz", "qmlp", cte.reward_layers(seed, S, A), hidden_dims=[32],
                              activations="relu", activation_final="none")
    paths = [str(tmp_path / f"m{seed}.ckpt") for seed, _ in FOUR]
    assert not any(os.path.exists(p) for p in paths)
    out = _runs(_four_configs(tmp_path / "runs", paths), _dataset(), None)
    for i, (g, want) in enumerate(zip(out, group4)):
        _assert_equal_runs(g, want, f"run {i}")
    # train() alone takes the same route
    cfg = _four_configs(tmp_path / "solo", paths)[1]
    _assert_equal_runs(_solo(cfg, _dataset(), None), group4[1], "train() from the file")


def test_fixture_sweep_file_end_to_end(golden_dir, tmp_path):
    from iqlpref_amd import custom_offline as co
    from iqlpref_amd import sweep as sw
    root = os.path.join(golden_dir, "pen_sweeps")
    configs = sw.expand_sweep(os.path.join(root, "sweep_pen_human_pref.yaml"), config_root=root, update_steps=20,
                              eval_every=20, batch_size=32, checkpoints_path=str(tmp_path))
    assert len(configs) == 10 and len({c.reward_model_path for c in configs}) == 10
    models = {c.reward_model_path: _qmlp(20 + i) for i, c in enumerate(configs)}
    records = []
    trainers = co.train_runs(configs, _dataset(), models, logger=lambda d, step: records.append((d, step)),
                             normalized_score=_normalized)
    assert len(trainers) == 10 and len({id(t) for t in trainers}) == 10
    assert len({c.checkpoints_path for c in configs}) == 10
    for i, (cfg, tr) in enumerate(zip(configs, trainers)):
        assert tr.total_it == 20
        assert os.path.commonpath([cfg.checkpoints_path, str(tmp_path)]) == str(tmp_path)
        with open(os.path.join(cfg.checkpoints_path, "config.yaml")) as f:
            assert yaml.safe_load(f) == asdict(cfg)
        assert sorted(f for f in os.listdir(cfg.checkpoints_path)) == ["best_model.pt", "checkpoint_19.pt", "config.yaml"]
        mine = [(d, s) for d, s in records if d["run"] == i]
        assert [s for d, s in mine if "value_loss" in d] == list(range(20))
        assert [next(iter(set(d) - {"run"})) for d, s in mine[20:]] == \
            ["evaluation_return", "normalized_score", "best_score_so_far", "best_step_so_far"]
    finals = [[d for d, _ in records if d["run"] == i and "value_loss" in d][-1]["value_loss"] for i in range(10)]
    assert len(set(finals)) == 10  # ten reward models, ten different runs
