"""Host side of the general step's seed groups and graph replay (no GPU): the two new C entry points are
declared, exported and bound without an ABI bump; ``group_mode`` is validated before any device work;
the sweep CLI prints the mode per batch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("iqlhip_trainer_launch_counts", "iqlhip_group_launch_counts")


def test_launch_count_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 6 and lib.iqlhip_abi_version() == 6
    # null handles are refused, not dereferenced
    assert lib.iqlhip_trainer_launch_counts(None, None, None) == _lib.ERR_INVALID
    assert lib.iqlhip_group_launch_counts(None, None, None) == _lib.ERR_INVALID


def test_python_surface():
    import iqlpref_amd as ia
    from iqlpref_amd import multi
    assert callable(ia.ImplicitQLearning.launch_counts) and callable(ia.SeedGroup.launch_counts)
    assert multi.GROUP_MODES == ("group", "split", "streams", "general")
    for mode in (None, "group", "split", "streams", "general"):
        assert multi.check_group_mode(mode) == mode
    with pytest.raises(ValueError, match="group_mode"):
        multi.check_group_mode("grouped")
    cfg = ia.TrainConfig()
    assert (cfg.hidden_dim, cfg.n_hidden) == (256, 2)  # the reference's defaults: the tuned step


def test_group_mode_is_validated_before_any_device_work():
    import iqlpref_amd as ia
    cfg = ia.TrainConfig(env="antmaze-medium-diverse-v2", max_timesteps=10)
    with pytest.raises(ValueError, match="group_mode"):
        ia.train(cfg, group_mode="fastest", state_dim=29, action_dim=8, max_action=1.0, dataset={})
    with pytest.raises(ValueError, match="group_mode"):
        ia.train_runs([cfg], object(), {}, group_mode="fastest")
    # ("general" passing validation: multi.check_group_mode in test_python_surface)


def test_shape_key_separates_depth_and_width():
    import iqlpref_amd as ia
    from iqlpref_amd import sweep as sw
    mk = lambda **kw: ia.TrainConfig(env="antmaze-medium-diverse-v2", **kw)
    cfgs = [mk(hidden_dim=96, n_hidden=3), mk(), mk(hidden_dim=96, n_hidden=3, beta=10.0), mk(hidden_dim=96, n_hidden=4)]
    assert sw.plan_batches(cfgs, [(29, 8)] * 4, 8) == [[0, 2], [1], [3]]
    assert sw.planned_mode(cfgs[0], "general") == "general" and sw.planned_mode(cfgs[1], "general") == "default"
    assert sw.planned_mode(cfgs[0], None) == "default" and sw.planned_mode(cfgs[1], "split") == "split"


def test_sweep_list_prints_the_mode_per_batch(tmp_path, capsys, monkeypatch):
    import yaml
    from iqlpref_amd import sweep as sw
    monkeypatch.delenv("AGENTS_PER_GPU", raising=False)
    spec = {"method": "grid", "parameters": {"env": {"value": "antmaze-medium-diverse-v2"},
                                             "hidden_dim": {"values": [96, 256]}, "n_hidden": {"values": [2, 3]},
                                             "beta": {"values": [3.0, 10.0]}}}
    path = tmp_path / "sweep.yaml"
    path.write_text(yaml.safe_dump(spec, sort_keys=False))
    sw.main([str(path), "--list", "--group_mode", "general"])
    rows = [ln.split("\t") for ln in capsys.readouterr().out.strip().splitlines()]
    assert [r[0] for r in rows] == [str(i) for i in range(8)]
    assert [r[2] for r in rows] == ["batch 0", "batch 0", "batch 1", "batch 1", "batch 2", "batch 2", "batch 3", "batch 3"]
    # 2 x 96 and 3 x 96 / 3 x 256 run on the general step; 2 x 256 is the tuned step: the default mode
    assert [r[3] for r in rows] == ["mode general"] * 4 + ["mode default"] * 2 + ["mode general"] * 2
    # without the flag the lines are what they were
    sw.main([str(path), "--list"])
    assert all(len(ln.split("\t")) == 3 for ln in capsys.readouterr().out.strip().splitlines())
    with pytest.raises(SystemExit):
        sw.main([str(path), "--list", "--group_mode", "fastest"])


def test_solo_forwards_to_its_one_trainer_and_stepper_picks(monkeypatch):
    import torch
    from iqlpref_amd import multi
    calls = []

    class Trainer:
        def train_steps(self, *args, **kw):
            calls.append((args, kw))
            return "losses" if kw["return_losses"] else None

    tr, buf, idx, keep, valid = Trainer(), object(), object(), object(), torch.zeros(5, dtype=torch.int32)
    solo = multi.Solo(tr)
    assert solo.trainers == [tr] and len(solo) == 1 and solo.mode == "solo" and solo.close() is None
    # every argument unchanged, in one call; a list of one losses back
    assert solo.train_steps([buf], 5, 32, indices=[idx], dropout_keep=[keep], return_losses=True, graph_unroll=7,
                            n_valid=[valid]) == ["losses"]
    assert solo.train_steps(buf, 5, 32, n_valid=valid) is None
    want = [((buf, 5, 32), dict(indices=idx, dropout_keep=keep, return_losses=True, graph_unroll=7, n_valid=valid)),
            ((buf, 5, 32), dict(indices=None, dropout_keep=None, return_losses=False, graph_unroll=None, n_valid=valid))]
    assert len(calls) == 2 and all(got[0] == exp[0] and list(got[1]) == list(exp[1]) and
                                   all(got[1][n] is exp[1][n] for n in exp[1]) for got, exp in zip(calls, want))
    # lists of another length: SeedGroup.train_steps' errors, and no call
    for kw, words in ((dict(indices=[idx, idx]), "indices / dropout_keep"), (dict(dropout_keep=[]), "indices / dropout_keep"),
                      (dict(n_valid=[valid, valid]), "n_valid: one tensor")):
        with pytest.raises(ValueError, match=words):
            solo.train_steps(buf, 5, 32, **kw)
    with pytest.raises(ValueError, match="one replay buffer per trainer"):
        solo.train_steps([buf, buf], 5, 32)
    assert len(calls) == 2
    # stepper: Solo for one trainer, SeedGroup with the mode and keywords for several (no library load)
    monkeypatch.setattr(multi, "SeedGroup", lambda trainers, **kw: ("group", trainers, kw))
    one = multi.stepper([tr], mode="group")
    assert isinstance(one, multi.Solo) and one.trainers == [tr]
    assert multi.stepper([tr, tr], mode="general", chunk=9) == ("group", [tr, tr], {"mode": "general", "chunk": 9})
    assert multi.stepper([tr, tr]) == ("group", [tr, tr], {"mode": None})
