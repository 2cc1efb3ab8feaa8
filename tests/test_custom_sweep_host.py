"""Sweep grids of the Minari custom-offline flavour (the six pen sweeps) on the host: expanding the files
into ``custom_offline.TrainConfig``s, launch batches, the checks ``custom_offline.train_runs`` makes before
any device work, the ``.npz`` reward-model interchange and ``sweep --list``.  No GPU.

The fixtures under tests/golden/pen_sweeps/ are copies of the reference's six pen sweep files and of the
three base files under configs/custom_offline/iql/pen/ (settings only).  The flavour's TrainConfig has no
``device`` field (cref:44-78), so the "before any device work" checks are shown by running where no GPU is."""
import os

import numpy as np
import pytest
import torch
import yaml

from iqlpref_amd import TrainConfig as OfflineConfig
from iqlpref_amd import custom_offline as co
from iqlpref_amd import sweep as sw
from tests import custom_train_env as cte

FILES = ["sweep_pen_human_pref.yaml", "sweep_pen_expert_pref.yaml", "sweep_pen_cloned_pref.yaml",
         "sweep_pen_human_pt.yaml", "sweep_pen_expert_pt.yaml", "sweep_pen_cloned_pt.yaml"]


@pytest.fixture(scope="module")
def root(golden_dir):
    return os.path.join(golden_dir, "pen_sweeps")


@pytest.mark.parametrize("fname", FILES)
def test_pen_sweep_files_expand_to_ten_custom_configs(fname, root):
    with open(os.path.join(root, fname)) as f:
        spec = yaml.safe_load(f)
    par = spec["parameters"]
    with open(os.path.join(root, par["config_path"]["value"])) as f:
        base = yaml.safe_load(f)
    cfgs = sw.expand_sweep(os.path.join(root, fname), config_root=root)
    assert len(cfgs) == 10 and all(type(c) is co.TrainConfig for c in cfgs)
    paths = par["reward_model_path"]["values"]
    assert len(paths) == 10 and [c.reward_model_path for c in cfgs] == paths
    for c, path in zip(cfgs, paths):
        assert c.train_seed == par["train_seed"]["value"] and c.dataset_id == par["dataset_id"]["value"]
        assert c.eval_episodes == par["eval_episodes"]["value"]
        assert c.query_length == par.get("query_length", {"value": base["query_length"]})["value"]
        assert c.group == par.get("group", {"value": base["group"]})["value"]
        # TrainConfig appends the run's unique name to the directory the file gives
        # (the name holds the dataset id, slashes and all, as in the reference)
        assert c.checkpoints_path == os.path.join(par["checkpoints_path"]["value"], c.name)
        assert c.name.startswith(par.get("name", {"value": base["name"]})["value"] + "-" + c.dataset_id + "-")
        assert c.iql_tau == base["iql_tau"] and c.actor_dropout == base["actor_dropout"]
        assert c.batch_size == base["batch_size"] and c.update_steps == int(base["update_steps"])
        assert c.sweep_label == f"reward_model_path={path}"
    assert len({c.checkpoints_path for c in cfgs}) == 10
    assert ("_pt" in fname) == (cfgs[0].query_length == 100)


def _spec(**params):
    return {"program": "algorithms/custom_offline/iql.py", "method": "grid",
            "parameters": {k: ({"values": v} if isinstance(v, list) else {"value": v}) for k, v in params.items()}}


def test_flavour_is_told_from_the_program_key():
    assert sw.is_custom_sweep(_spec()) and sw.is_custom_sweep({"program": "/x/algorithms/custom_offline/iql.py"})
    for program in ("algorithms/offline/iql.py", "x.py", "algorithms/custom_offline/iql_bb.py", None):
        assert not sw.is_custom_sweep({"program": program})
    assert not sw.is_custom_sweep({})
    # the same names under another program are an offline sweep, which does not know them
    spec = dict(_spec(train_seed=[0, 1]), program="algorithms/offline/iql.py")
    with pytest.raises(ValueError, match="train_seed"):
        sw.expand_sweep(spec)
    assert type(sw.expand_sweep({"method": "grid", "parameters": {"seed": {"values": [0]}}})[0]) is OfflineConfig


def test_offline_names_are_unknown_to_a_custom_sweep_and_listed_together():
    with pytest.raises(ValueError) as e:
        sw.expand_sweep(_spec(seed=[1, 2], env="pen-human-v1", beta=3.0, train_seed=0))
    msg = str(e.value)
    assert "seed" in msg.replace("train_seed", "") and "env" in msg and "beta" not in msg and "train_seed" not in msg
    with pytest.raises(ValueError, match="max_timesteps"):
        sw.expand_sweep(_spec(train_seed=0), max_timesteps=5)


def test_overrides_are_coerced_and_beat_the_file(root):
    cfgs = sw.expand_sweep(os.path.join(root, FILES[0]), config_root=root, update_steps="40", eval_every="20",
                           normalize_reward="true", actor_dropout="0.25", train_seed="3")
    assert len(cfgs) == 10
    for c in cfgs:
        assert c.update_steps == 40 and isinstance(c.update_steps, int) and c.eval_every == 20
        assert c.normalize_reward is True and c.actor_dropout == 0.25 and c.train_seed == 3
    c = co.load_config(os.path.join(root, "configs/custom_offline/iql/pen/expert_v1.yaml"), qf_lr="1e-4")
    assert c.qf_lr == 1e-4 and c.dataset_id == "D4RL/pen/expert-v2" and c.checkpoints_path is None
    with pytest.raises(ValueError, match="max_timesteps"):
        co.load_config(None, max_timesteps=3)


def test_planning():
    cfgs = [co.TrainConfig(reward_model_path=f"m{i}", beta=1.0 + i, train_seed=i % 3, update_steps=10 + i,
                           eval_every=5 + i, normalize_reward=bool(i & 1), actor_dropout=0.1 + 0.01 * i)
            for i in range(10)]
    dims = [(45, 24)] * 10
    assert co.plan_batches(cfgs, dims, 8) == [list(range(8)), [8, 9]]
    assert co.plan_batches(cfgs, dims, 16) == [list(range(10))]
    assert co.plan_batches(cfgs[:3], dims[:3], 1) == [[0], [1], [2]]
    for kw in ({"batch_size": 128}, {"iql_deterministic": True}, {"actor_dropout": None}):
        other = [cfgs[0], co.TrainConfig(**{"actor_dropout": 0.1, **kw}), cfgs[1]]
        assert co.plan_batches(other, dims[:3], 8) == [[0, 2], [1]], kw
    assert co.plan_batches(cfgs[:2], [(45, 24), (39, 28)], 8) == [[0], [1]]
    assert co.shape_key(cfgs[0], (45, 24), "cuda:0") != co.shape_key(cfgs[0], (45, 24), "cuda:1")
    # unknown dims: the dataset id stands in
    two = [co.TrainConfig(dataset_id="a/b-v0"), co.TrainConfig(dataset_id="a/c-v0"), co.TrainConfig(dataset_id="a/b-v0")]
    assert co.plan_batches(two, [None] * 3, 8) == [[0, 2], [1]]
    # the offline planner keeps its signature and behaviour
    off = [OfflineConfig(device="cuda", seed=s) for s in range(3)]
    assert sw.plan_batches(off, [(29, 8)] * 3, 2) == [[0, 1], [2]]
    assert sw.plan_batches(off, [(29, 8)] * 3, 2, "fp32") == [[0, 1], [2]]
    for k in (0, 17):
        with pytest.raises(ValueError, match="runs_per_gpu"):
            co.plan_batches(cfgs, dims, k)


def _qmlp(seed=5):
    return co.QMLP(45, 24, (32,), "relu", "none").load_flax_params(cte.reward_layers(seed, 45, 24))


def test_checks_come_before_any_device_work(tmp_path):
    ds = cte.MinariDataset(11, (23, 17))
    a, b = co.TrainConfig(reward_model_path="m0"), co.TrainConfig(reward_model_path="m1")
    a.checkpoints_path = b.checkpoints_path = str(tmp_path / "same")
    with pytest.raises(ValueError, match="checkpoints_path"):
        co.train_runs([a, b], ds, {"m0": _qmlp(), "m1": _qmlp()})
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="runs_per_gpu"):
            co.train_runs([co.TrainConfig(reward_model_path="m0")], ds, {"m0": _qmlp()}, runs_per_gpu=k)
    cfgs = [co.TrainConfig(reward_model_path=p) for p in ("m0", "~/nowhere/best_model.ckpt", str(tmp_path / "no.ckpt"))]
    with pytest.raises(ValueError) as e:
        co.train_runs(cfgs, ds, {"m0": _qmlp()})
    assert "~/nowhere/best_model.ckpt" in str(e.value) and str(tmp_path / "no.ckpt") in str(e.value)
    assert "'m0'" not in str(e.value) and "save_reward_params" in str(e.value)
    with pytest.raises(ValueError, match="nowhere"):
        co.train_runs(cfgs[1:2], ds, None)
    with pytest.raises(TypeError, match="RewardPT"):
        co.train_runs([co.TrainConfig(reward_model_path="m0", query_length=5)], ds, {"m0": _qmlp()})
    co.save_reward_params(tmp_path / "q.ckpt.npz", "qmlp", cte.reward_layers(5, 45, 24))
    with pytest.raises(TypeError, match="RewardPT"):
        co.train_runs([co.TrainConfig(reward_model_path=str(tmp_path / "q.ckpt"), query_length=5)], ds, None)
    with pytest.raises(ValueError, match="sampler"):
        co.train_runs([co.TrainConfig(reward_model_path="m0")], ds, {"m0": _qmlp()}, sampler="gpu")
    with pytest.raises(ValueError, match="run_ids"):
        co.train_runs([co.TrainConfig(reward_model_path="m0")], ds, {"m0": _qmlp()}, run_ids=[0, 1])
    # paths are matched as written and after expanduser
    home = os.path.expanduser("~/m/best_model.ckpt")
    src = co._model_sources([co.TrainConfig(reward_model_path="~/m/best_model.ckpt")], {home: "model"})
    assert list(src.values()) == ["model"]


def test_reward_params_round_trip_qmlp(tmp_path):
    layers = cte.reward_layers(7, 45, 24)
    path = co.save_reward_params(tmp_path / "best_model.ckpt.npz", "qmlp", layers, hidden_dims=[32],
                                 activations="tanh", activation_final="softplus")
    assert path == str(tmp_path / "best_model.ckpt.npz") and os.path.isfile(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["0/bias", "0/kernel", "1/bias", "1/kernel", "__meta__"]
    m = co.load_reward_model(path, 45, 24, "cpu")
    assert isinstance(m, co.QMLP) and (m.activations, m.activation_final) == ("tanh", "softplus")
    assert len(m.kernels) == 2
    for k, b, l in zip(m.kernels, m.biases, layers):
        assert torch.equal(k.detach(), torch.from_numpy(l["kernel"])) and torch.equal(b.detach(), torch.from_numpy(l["bias"]))
    # the hidden sizes are read off the arrays when the constructor arguments leave them out
    m2 = co.load_reward_model(co.save_reward_params(tmp_path / "b.npz", "qmlp", layers), 45, 24, "cpu")
    assert (m2.activations, m2.activation_final) == ("relu", "none") and tuple(m2.kernels[0].shape) == (69, 32)
    # which file a reward_model_path is read from
    assert co.reward_model_file(str(tmp_path / "best_model.ckpt")) == path
    assert co.reward_model_file(str(tmp_path / "x.npz")) == str(tmp_path / "x.npz")
    assert co.reward_model_file(str(tmp_path / "other.ckpt")) is None
    with pytest.raises(ValueError, match="kind"):
        co.save_reward_params(tmp_path / "c.npz", "mlp", layers)
    np.savez(tmp_path / "plain.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="__meta__"):
        co.load_reward_model(tmp_path / "plain.npz", 45, 24, "cpu")


def test_reward_params_round_trip_pt_tree(tmp_path):
    """A PT tree goes in and comes out key for key (the model itself needs the GPU only to run)."""
    from iqlpref_amd.relabel import RewardPT
    torch.manual_seed(0)
    ref = RewardPT(45, 24, 30, embd_dim=64, num_heads=4, intermediate_dim=128, num_layers=1)
    lin = lambda m: {"kernel": m.weight.detach().numpy().T.copy(), "bias": m.bias.detach().numpy().copy()}
    ln = lambda m: {"scale": m.weight.detach().numpy().copy(), "bias": m.bias.detach().numpy().copy()}
    tree = {}
    for name, mod in ref.named_modules():
        if isinstance(mod, (torch.nn.Linear, torch.nn.LayerNorm, torch.nn.Embedding)):
            node = tree
            *parents, leaf = name.split(".")
            for p in parents:
                node = node.setdefault(p, {})
            node[leaf] = (lin(mod) if isinstance(mod, torch.nn.Linear) else ln(mod) if isinstance(mod, torch.nn.LayerNorm)
                          else {"embedding": mod.weight.detach().numpy().copy()})
    path = co.save_reward_params(tmp_path / "pt.ckpt.npz", "pt", tree, max_episode_steps=30, embd_dim=64,
                                 num_heads=4, intermediate_dim=128, num_layers=1)
    m = co.load_reward_model(path, 45, 24, "cpu")
    assert isinstance(m, RewardPT)
    want = ref.state_dict()
    for k, v in m.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_main_list(root, capsys, monkeypatch):
    monkeypatch.delenv("AGENTS_PER_GPU", raising=False)
    path = os.path.join(root, "sweep_pen_human_pt.yaml")
    sw.main([path, "--config_root", root, "--list"])
    lines = [ln.split("\t") for ln in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 10
    assert [ln[0] for ln in lines] == [str(i) for i in range(10)]
    assert [ln[2] for ln in lines] == ["batch 0"] * 8 + ["batch 1"] * 2
    assert lines[3][1] == "reward_model_path=~/iqlpref/pen_labels/pt_pen/pt_reduce_30/best_model.ckpt"
    sw.main([path, "--config_root", root, "--list", "--only", "1,4,5", "--runs_per_gpu", "2", "--update_steps", "40"])
    lines = [ln.split("\t") for ln in capsys.readouterr().out.strip().splitlines()]
    assert [ln[0::2] for ln in lines] == [["1", "batch 0"], ["4", "batch 0"], ["5", "batch 1"]]
    with pytest.raises(SystemExit, match="group_mode"):
        sw.main([path, "--config_root", root, "--list", "--group_mode", "general"])
    with pytest.raises(ValueError, match="runs_per_gpu"):
        sw.main([path, "--config_root", root, "--list", "--runs_per_gpu", "17"])
    assert sw._list_dims_custom("D4RL/pen/human-v2") == (45, 24) and sw._list_dims_custom("mujoco/ant/x-v0") is None


def _loop(totals, everys, chunk):
    """_offline_loop.run over stand-in trainers: what was stepped, logged and evaluated, and the members of every
    group that was built."""
    from iqlpref_amd import _offline_loop
    K = len(totals) if isinstance(totals, list) else 2
    calls = []

    def steps(group, active, t, n):
        assert group is None
        calls.append(("steps", t, n, tuple(active)))
        return [torch.full((n, 3), float(k)) + torch.arange(t, t + n, dtype=torch.float32)[:, None] for k in active]

    def make_group(active):
        calls.append(("make_group", tuple(active)))
        return None

    records = []
    _offline_loop.run([object()] * K, list(range(K)), make_group, totals, everys, chunk,
                      lambda d, s: records.append((d, s)), [None] * K, steps,
                      lambda k, tr, step: calls.append(("eval", k, step)) or np.asarray([1.0 * k]),
                      _offline_loop.BestModelRecords([None] * K), tagged=lambda rec, k: dict(rec, run=k))
    return calls, records


def test_loop_per_member_totals_and_periods():
    calls, records = _loop([6, 4], [3, 2], 100)
    assert calls == [("make_group", (0, 1)), ("steps", 0, 2, (0, 1)), ("eval", 1, 1), ("steps", 2, 1, (0, 1)),
                     ("eval", 0, 2), ("steps", 3, 1, (0, 1)), ("eval", 1, 3), ("make_group", (0,)),
                     ("steps", 4, 2, (0,)), ("eval", 0, 5)]
    for k, total in ((0, 6), (1, 4)):
        mine = [(d, s) for d, s in records if d["run"] == k and "value_loss" in d]
        assert [s for _, s in mine] == list(range(total))
        assert [d["value_loss"] for d, _ in mine] == [float(k + s) for s in range(total)]
    # the chunk bounds a call as well; a member of no steps never enters
    calls, _ = _loop([5, 0], [10, 10], 2)
    assert calls == [("make_group", (0,)), ("steps", 0, 2, (0,)), ("steps", 2, 2, (0,)), ("steps", 4, 1, (0,))]
    # scalars: every member to the end, one group for all of it
    calls, records = _loop(4, 2, 100)
    assert calls == [("make_group", (0, 1)), ("steps", 0, 2, (0, 1)), ("eval", 0, 1), ("eval", 1, 1), ("steps", 2, 2, (0, 1)), ("eval", 0, 3),
                     ("eval", 1, 3)]
    assert len(records) == 2 * 4 + 2 * 2 * 3


def test_package_surface():
    assert callable(co.train_runs) and callable(co.load_config) and callable(co.save_reward_params)
    assert "global generator" in co.train_runs.__doc__
