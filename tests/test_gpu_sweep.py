"""Sweep grids on one GPU (iqlpref_amd.sweep.train_runs): runs of DIFFERENT configs packed into
seed groups must each equal their solo ``train(config)`` bit for bit -- the logged records, every
evaluation call, every checkpoint file and the final parameters, target and Adam moments.  -m gpu."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def synth(n, S, A, seed=0):
    rng = np.random.default_rng(seed)
    return {
        "observations": (rng.standard_normal((n, S)) * 2 + 0.5).astype(np.float32),
        "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
        "rewards": (rng.uniform(size=n) < 0.05).astype(np.float32),
        "next_observations": (rng.standard_normal((n, S)) * 2 + 0.5).astype(np.float32),
        "terminals": (rng.uniform(size=n) < 0.01).astype(np.float32),
    }


class Env:
    """The fields train() reads from an environment: the two spaces and the episode length."""

    def __init__(self, S, A, max_episode_steps=1000):
        self.observation_space = SimpleNamespace(shape=(S,))
        self.action_space = SimpleNamespace(shape=(A,), high=np.ones(A, np.float32))
        self._max_episode_steps = max_episode_steps


def recorder():
    """An evaluation callable whose answer depends on the actor it gets, and the list of its calls."""
    calls = []

    def evaluate(actor, t):
        w = actor.net.linears()[2].weight
        calls.append((t, float(w.detach().double().sum())))
        return np.array([float(w[0, 0]), 1.0]), [t]
    return evaluate, calls


def same(a, b, where=""):
    """Exact equality of nested checkpoint contents (tensors bit for bit)."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{k}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, where


def solo(cfg, env, data, *, precision="bf16", host_prep=False, raw=False):
    import iqlpref_amd as ia
    logs = []
    evaluate, evals = recorder()
    src = {k: np.array(v) for k, v in data.items()}
    tr = ia.train(cfg, env=env, dataset=None if raw else src, raw_dataset=src if raw else None,
                  logger=lambda d, step: logs.append((step, dict(d))), evaluate=evaluate, precision=precision,
                  host_prep=host_prep)
    return tr, logs, evals


def grouped(cfgs, env, data, *, precision="bf16", host_prep=False, raw=False, **kw):
    import iqlpref_amd as ia
    logs = []
    recs = [recorder() for _ in cfgs]
    src = {k: np.array(v) for k, v in data.items()}
    trs = ia.train_runs(cfgs, env, None if raw else src, raw_dataset=src if raw else None,
                        logger=lambda d, step: logs.append((step, dict(d))), evaluate=[r[0] for r in recs],
                        precision=precision, host_prep=host_prep, **kw)
    # the source dataset is untouched (every preparation works on its own copy or on the device)
    for k in data:
        assert np.array_equal(src[k], data[k]), k
    per_run = []
    for i, cfg in enumerate(cfgs):
        mine = [(st, {n: v for n, v in d.items() if n not in ("run", "seed")}) for st, d in logs if d["run"] == i]
        assert all(d["seed"] == cfg.seed for _, d in logs if d["run"] == i)
        per_run.append((mine, recs[i][1]))
    return trs, per_run


def assert_equal_runs(cfg_s, tr_s, logs_s, evals_s, cfg_g, tr_g, logs_g, evals_g):
    n_logs = cfg_s.max_timesteps // cfg_s.log_freq
    n_evals = cfg_s.max_timesteps // cfg_s.eval_freq
    assert len(logs_s) == n_logs + n_evals and logs_g == logs_s  # equal floats, equal steps
    assert len(evals_s) == n_evals and evals_g == evals_s
    assert tr_g.total_it == tr_s.total_it == cfg_s.max_timesteps
    for name in ("_params", "_target", "_exp_avg", "_exp_avg_sq"):
        assert torch.equal(getattr(tr_g, name), getattr(tr_s, name)), name
    if cfg_s.checkpoints_path is None:
        return
    files = sorted(os.listdir(cfg_s.checkpoints_path))
    assert files == sorted(os.listdir(cfg_g.checkpoints_path))
    ckpts = sorted(f"checkpoint_{(k + 1) * cfg_s.eval_freq - 1}.pt" for k in range(n_evals))
    assert files == sorted(ckpts + ["config.yaml"])
    for f in ckpts:
        a = torch.load(os.path.join(cfg_g.checkpoints_path, f), weights_only=True)
        b = torch.load(os.path.join(cfg_s.checkpoints_path, f), weights_only=True)
        same(a, b, f)
    import yaml
    ya = yaml.safe_load(open(os.path.join(cfg_g.checkpoints_path, "config.yaml")))
    yb = yaml.safe_load(open(os.path.join(cfg_s.checkpoints_path, "config.yaml")))
    for k in ("name", "checkpoints_path"):  # (every TrainConfig draws its own unique name)
        ya.pop(k), yb.pop(k)
    assert ya == yb


ANT = "antmaze-medium-diverse-v2"
# four runs that differ in everything but shape
ANT_RUNS = [
    dict(seed=3, normalize_reward=1, beta=10.0, iql_tau=0.9, max_timesteps=60, log_freq=10, eval_freq=30),
    dict(seed=4, normalize_reward=3, beta=3.0, iql_tau=0.7, discount=0.95, tau=0.01, vf_lr=1e-4, qf_lr=2e-4,
         actor_lr=5e-4, max_timesteps=40, log_freq=8, eval_freq=20),
    dict(seed=5, normalize_reward=5, beta=5.0, iql_tau=0.8, discount=0.97, tau=0.002, vf_lr=4e-4, qf_lr=1e-4,
         actor_lr=2e-4, max_timesteps=60, log_freq=15, eval_freq=25),
    dict(seed=6, normalize_reward=7, beta=1.0, iql_tau=0.6, discount=0.9, tau=0.02, actor_lr=1e-3,
         max_timesteps=40, log_freq=10, eval_freq=40),
]


def _ant_cfg(tmp_path, sub, i, **kw):
    import iqlpref_amd as ia
    return ia.TrainConfig(env=ANT, batch_size=64, device=DEV, buffer_size=10_000_000,
                          checkpoints_path=str(tmp_path / sub), **dict(ANT_RUNS[i], **kw))


@pytest.mark.parametrize("mode", ["group", None])
def test_runs_of_different_configs_equal_their_solo_runs(tmp_path, mode):
    S, A = 29, 8
    data, env = synth(3000, S, A), Env(S, A)
    cfgs = [_ant_cfg(tmp_path, f"grid{i}", i) for i in range(4)]
    trs, per_run = grouped(cfgs, env, data, group_mode=mode)
    assert [t._seed for t in trs] == [3, 4, 5, 6]
    for i in range(4):
        cfg_s = _ant_cfg(tmp_path, f"solo{i}", i)
        tr_s, logs_s, evals_s = solo(cfg_s, env, data)
        assert_equal_runs(cfg_s, tr_s, logs_s, evals_s, cfgs[i], trs[i], *per_run[i])
    # the runs did train differently
    assert not torch.equal(trs[0]._params, trs[1]._params)


def test_pen_runs_with_two_dropout_rates_in_one_group(tmp_path):
    import iqlpref_amd as ia
    S, A = 45, 24
    data, env = synth(2000, S, A, seed=1), Env(S, A)

    def cfg(sub, seed, p):
        return ia.TrainConfig(env="pen-human-v1", seed=seed, actor_dropout=p, batch_size=64, max_timesteps=30,
                              log_freq=10, eval_freq=15, device=DEV, checkpoints_path=str(tmp_path / sub))
    cfgs = [cfg("g0", 11, 0.1), cfg("g1", 12, 0.25)]
    assert ia.plan_batches(cfgs, [(S, A)] * 2, 8) == [[0, 1]]
    trs, per_run = grouped(cfgs, env, data, group_mode="group")
    for i, (seed, p) in enumerate(((11, 0.1), (12, 0.25))):
        c = cfg(f"s{i}", seed, p)
        tr_s, logs_s, evals_s = solo(c, env, data)
        assert_equal_runs(c, tr_s, logs_s, evals_s, cfgs[i], trs[i], *per_run[i])


def test_mixed_batch_sizes_and_policy_kinds_split_into_batches(tmp_path):
    import iqlpref_amd as ia
    S, A = 29, 8
    data, env = synth(2000, S, A, seed=2), Env(S, A)
    kinds = [dict(batch_size=64), dict(batch_size=32), dict(batch_size=64, iql_deterministic=True),
             dict(batch_size=64, seed=30, normalize_reward=0)]

    def cfg(sub, i):
        kw = dict(seed=7 + i, normalize_reward=1, max_timesteps=24, log_freq=6, eval_freq=12)
        kw.update(kinds[i])
        return ia.TrainConfig(env=ANT, device=DEV, checkpoints_path=str(tmp_path / sub), **kw)
    cfgs = [cfg(f"g{i}", i) for i in range(4)]
    assert ia.plan_batches(cfgs, [(S, A)] * 4, 8, "fp32") == [[0, 3], [1], [2]]
    trs, per_run = grouped(cfgs, env, data, precision="fp32", host_prep=True)
    for i in range(4):
        c = cfg(f"s{i}", i)
        tr_s, logs_s, evals_s = solo(c, env, data, precision="fp32", host_prep=True)
        assert_equal_runs(c, tr_s, logs_s, evals_s, cfgs[i], trs[i], *per_run[i])


def _mr_dir(path, S, A, seed):
    path.mkdir()
    (path / "config.yaml").write_text("activations: relu\n")
    w = [np.random.default_rng(seed).standard_normal(s).astype(np.float32) * 0.4
         for s in ((S + A, 16), (16,), (16, 16), (16,), (16, 1), (1,))]
    torch.save({"net": {"layers.0.W": torch.from_numpy(w[0]), "layers.0.b": torch.from_numpy(w[1]),
                        "layers.linear_1.W": torch.from_numpy(w[2]), "layers.linear_1.b": torch.from_numpy(w[3]),
                        "output.W": torch.from_numpy(w[4]), "output.b": torch.from_numpy(w[5])}},
               path / "best_model.pt")
    return str(path)


def test_two_reward_models_times_two_normalisations_relabel_twice(tmp_path, monkeypatch):
    import iqlpref_amd as ia
    S, A, N = 29, 8, 2000
    rng = np.random.default_rng(3)
    raw = {"observations": rng.standard_normal((N, S)).astype(np.float32),
           "actions": rng.uniform(-1, 1, (N, A)).astype(np.float32),
           "rewards": np.zeros(N, np.float32), "terminals": rng.uniform(size=N) < 0.002,
           "timeouts": np.zeros(N, bool)}
    raw["timeouts"][[499, 999, 1499]] = True
    env = Env(S, A, max_episode_steps=500)
    mr = [_mr_dir(tmp_path / "mr_a", S, A, 1), _mr_dir(tmp_path / "mr_b", S, A, 2)]
    grid = [(0, 1), (0, 3), (1, 1), (1, 3)]

    def cfg(sub, k):
        m, nr = grid[k]
        return ia.TrainConfig(env=ANT, reward_model_path=mr[m], normalize_reward=nr, seed=20 + k, batch_size=32,
                              max_timesteps=20, log_freq=5, eval_freq=10, device=DEV,
                              checkpoints_path=str(tmp_path / sub))
    cfgs = [cfg(f"g{k}", k) for k in range(4)]
    T = sys.modules["iqlpref_amd.train"]
    calls, real = [], T.build_dataset
    monkeypatch.setattr(T, "build_dataset", lambda c, e, d=None: calls.append(c.reward_model_path) or real(c, e, d))
    trs, per_run = grouped(cfgs, env, raw, raw=True)
    monkeypatch.setattr(T, "build_dataset", real)
    assert sorted(calls) == sorted(mr)
    for k in range(4):
        c = cfg(f"s{k}", k)
        tr_s, logs_s, evals_s = solo(c, env, raw, raw=True)
        assert_equal_runs(c, tr_s, logs_s, evals_s, cfgs[k], trs[k], *per_run[k])
    assert not torch.equal(trs[0]._params, trs[2]._params)


def test_one_run_equals_train(tmp_path):
    import iqlpref_amd as ia
    S, A = 29, 8
    data, env = synth(3000, S, A), Env(S, A)
    cfg_g = _ant_cfg(tmp_path, "one", 1)
    logs = []
    evaluate, evals = recorder()
    (tr_g,) = ia.train_runs([cfg_g], env, {k: v.copy() for k, v in data.items()}, evaluate=evaluate,
                            logger=lambda d, step: logs.append((step, dict(d))))
    assert {(d["run"], d["seed"]) for _, d in logs} == {(0, 4)}
    logs = [(st, {n: v for n, v in d.items() if n not in ("run", "seed")}) for st, d in logs]
    cfg_s = _ant_cfg(tmp_path, "solo", 1)
    tr_s, logs_s, evals_s = solo(cfg_s, env, data)
    assert_equal_runs(cfg_s, tr_s, logs_s, evals_s, cfg_g, tr_g, logs, evals)
