"""Resumed runs are the uninterrupted runs, bit for bit.  -m gpu.

Every test runs one config (or list of configs) twice: once to the end, and once cut by a host-side
exception from an injected callback and started again with ``resume=True``.  There are no tolerances: the
logger records from the resume step on (the records of the first part up to its last committed generation,
followed by the resumed part's, are the uninterrupted run's), every file under the checkpoint directories
(loaded, tensors with ``torch.equal``) and the returned trainers' ``resume_state()`` must be equal.  The one
exception is the wall-clock field ``steps_per_sec`` (and the ``steps_per_sec_total`` made of it).

Shapes are the smallest that exercise every saved item: S = 5, A = 3, batch 16 (one slab), 40 steps with an
evaluation every 10 and a loss window of 4 (so a window is half full at steps 10 and 30), a Gaussian actor
with dropout 0.1, whose in-step masks are keyed by the step and whose stand-alone train-mode forward -- the
injected evaluation runs one -- draws its masks by the module's call counter.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from tests import custom_train_env as cte

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, A = 5, 3


class Cut(Exception):
    """The host-side interruption."""


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    return {"observations": (rng.standard_normal((n, S)) * 2 + 0.5).astype(np.float32),
            "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "rewards": rng.uniform(size=n).astype(np.float32),
            "next_observations": (rng.standard_normal((n, S)) * 2 + 0.5).astype(np.float32),
            "terminals": (rng.uniform(size=n) < 0.05).astype(np.float32)}


ENV = SimpleNamespace(observation_space=SimpleNamespace(shape=(S,)),
                      action_space=SimpleNamespace(shape=(A,), high=np.ones(A, np.float32)), _max_episode_steps=1000)
PROBE = torch.linspace(-1, 1, 4 * S).reshape(4, S)


def make_evaluate(cut_at=None):
    """``evaluate(actor, t)``: the scores are a TRAIN-mode forward of the actor (dropout masks by the
    module's call counter); raises ``Cut`` at step ``cut_at``."""
    calls = []

    def evaluate(actor, t):
        if t == cut_at:
            raise Cut(f"in the evaluation at step {t}")
        assert actor.training
        out = actor.net(PROBE.to(DEV)).double().sum(dim=1).cpu().numpy()
        calls.append((t, out.tolist()))
        return out, [t]
    return evaluate, calls


def strip(x):
    """Nested contents without the wall-clock fields."""
    if isinstance(x, dict):
        return {k: strip(v) for k, v in x.items() if not str(k).startswith("steps_per_sec")}
    if isinstance(x, (list, tuple)):
        return [strip(v) for v in x]
    return x


def same(a, b, where=""):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


def tree(root):
    """Every file under a checkpoint directory, loaded: {relative name: contents}; config.yaml without the
    run's own name and path."""
    out = {}
    for d, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            path = os.path.join(d, f)
            if f == "config.yaml":
                with open(path) as fh:
                    c = yaml.safe_load(fh)
                out[os.path.relpath(path, root)] = {k: v for k, v in c.items() if k not in ("name", "checkpoints_path")}
            else:
                out[os.path.relpath(path, root)] = strip(torch.load(path, weights_only=True))
    return out


def same_trees(a, b, what):
    ta, tb = tree(a), tree(b)
    assert list(ta) == list(tb), what
    assert any(f.startswith("resume_") or "/resume_" in f for f in ta), what
    same(ta, tb, what)


def same_trainers(a, b, what):
    a, b = (a if isinstance(a, list) else [a]), (b if isinstance(b, list) else [b])
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        same(x.resume_state(), y.resume_state(), f"{what}: trainer {k}")


def upto(records, step):
    return [(s, d) for s, d in records if s <= step]


# --------------------------------------------------------------------------- #
# offline train()
# --------------------------------------------------------------------------- #
def offline_config(path, **kw):
    import iqlpref_amd as ia
    base = dict(env="resume-fake-v0", batch_size=16, device=DEV, hidden_dim=64, n_hidden=2, max_timesteps=40,
                eval_freq=10, log_freq=4, actor_dropout=0.1, normalize_reward=0, seed=3, checkpoints_path=str(path))
    base.update(kw)
    return ia.TrainConfig(**base)


def offline_run(cfg, data, *, cut_at=None, resume=True, **kw):
    """-> (trainers or None when cut, records [(step, record without wall-clock fields)], evaluation calls)."""
    import iqlpref_amd as ia
    records = []
    evaluate, calls = make_evaluate(cut_at)
    trainers = None
    try:
        trainers = ia.train(cfg, env=ENV, dataset={k: np.array(v) for k, v in data.items()},
                            logger=lambda d, step: records.append((int(step), strip(dict(d)))), evaluate=evaluate,
                            resume=resume, **kw)
    except Cut:
        assert cut_at is not None
    return trainers, records, calls


def cut_and_resume(tmp_path, data, tamper=None, **kw):
    """The uninterrupted run, and the run cut in the evaluation at step 20 and resumed (from generation 10)."""
    train_kw = {k: kw.pop(k) for k in ("precision", "seeds_per_gpu") if k in kw}
    whole_cfg = offline_config(tmp_path / "whole", **kw)
    whole = offline_run(whole_cfg, data, **train_kw)
    cfg = offline_config(tmp_path / "cut", **kw)
    first = offline_run(cfg, data, cut_at=20, **train_kw)
    assert first[0] is None and [t for t, _ in first[2]] == [10] * train_kw.get("seeds_per_gpu", 1)
    if tamper is not None:
        tamper(cfg)
    second = offline_run(cfg, data, **train_kw)
    return whole_cfg, whole, cfg, first, second


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["one_seed", "three_seeds", "general_step", "end_off_the_eval_grid"])
def test_offline_train_resumed_is_the_uninterrupted_run(tmp_path, shape, precision):
    """``end_off_the_eval_grid``: 34 steps, no multiple of ``eval_freq``: the run still ends with a generation at
    its last step, written when its seeds leave the loop, and that generation says finished."""
    from iqlpref_amd import _resume
    kw = {"one_seed": {}, "three_seeds": {"seeds_per_gpu": 3}, "general_step": {"n_hidden": 3, "hidden_dim": 40},
          "end_off_the_eval_grid": {"max_timesteps": 34}}[shape]
    data = synth(300)
    whole_cfg, whole, cfg, first, second = cut_and_resume(tmp_path, data, precision=precision, **kw)
    K = kw.get("seeds_per_gpu", 1)
    total = cfg.max_timesteps
    assert total == kw.get("max_timesteps", 40)
    trainers = second[0] if K > 1 else [second[0]]
    assert trainers[0].step_kind(16) == ("general" if shape == "general_step" else "tuned")
    assert all(t.total_it == total for t in trainers)
    # the resumed part starts behind step 10: its first record is the window that ends at step 12
    evaluated = [t for t in range(cfg.eval_freq, total + 1, cfg.eval_freq) if t >= 20]  # (cut in the one at 20)
    assert second[1][0][0] == 12 and [t for t, _ in second[2]] == [t for t in evaluated for _ in range(K)]
    assert upto(first[1], 10) + second[1] == whole[1]
    assert first[2][:K] + second[2] == whole[2]  # what the evaluations saw: the dropout call counter went on
    same_trees(cfg.checkpoints_path, whole_cfg.checkpoints_path, shape)
    same_trainers(second[0], whole[0], shape)
    seed_dirs = [os.path.join(cfg.checkpoints_path, f"seed_{3 + k}") for k in range(K)]
    for d in [cfg.checkpoints_path] if K == 1 else seed_dirs:
        assert _resume.steps_in(d) == [total] and _resume.status(d) == "done"  # one generation, at the last step
    # a finished run started again trains and evaluates nothing and returns the same trainers
    third = offline_run(cfg, data, precision=precision, **({"seeds_per_gpu": K} if K > 1 else {}))
    assert third[1] == [] and third[2] == []
    same_trainers(third[0], whole[0], f"{shape}, started again")


def test_a_resume_that_forgot_the_target_network_is_caught(tmp_path):
    """The generation's target entry replaced by a copy of ``qf`` -- what ``load_model`` does (ref:679) --
    gives another run: the comparison above would catch a resume that did not save the target."""
    from iqlpref_amd import _resume

    def tamper(cfg):
        p = _resume.read(cfg.checkpoints_path, 10)
        assert not any(torch.equal(p["trainer"]["q_target"][k], v) for k, v in p["trainer"]["state_dict"]["qf"].items())
        p["trainer"]["q_target"] = {k: v.clone() for k, v in p["trainer"]["state_dict"]["qf"].items()}
        _resume.write(cfg.checkpoints_path, 10, p)

    whole_cfg, whole, cfg, first, second = cut_and_resume(tmp_path, synth(300), tamper=tamper, precision="fp32")
    assert second[0].total_it == 40 and len(second[1]) == len(whole[1]) - len(upto(first[1], 10))
    assert upto(first[1], 10) + second[1] != whole[1]
    assert not torch.equal(second[0]._target, whole[0]._target)
    assert not torch.equal(second[0]._params, whole[0]._params)


def test_resume_state_round_trip_on_a_fresh_trainer(tmp_path):
    """``load_resume_state`` on a freshly built trainer, before it joins a SeedGroup: the next steps are the
    source's next steps, alone and as members of a group; ``state_dict()`` keeps the reference's 8 keys."""
    import importlib
    from iqlpref_amd.multi import SeedGroup
    T = importlib.import_module("iqlpref_amd.train")  # (the package exports the function under this name)
    cfg = offline_config(tmp_path, checkpoints_path=None)
    buf, _, _ = T._prepare_replay(cfg, synth(300), S, A, False)
    build = lambda seed: T._build_trainer(cfg, seed, S, A, 1.0, "bf16")
    src = [build(3), build(4)]
    for tr in src:
        tr.train_steps(buf, 7, 16)
        tr.actor.net(PROBE.to(DEV))  # one stand-alone train-mode forward: the call counter is at 1
    assert list(src[0].state_dict()) == ["qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer",
                                         "actor_lr_schedule", "total_it"]
    states = [tr.resume_state() for tr in src]
    assert states[0]["dropout"] == {"actor.net": [3, 1]} and states[0]["total_it"] == 7
    want = [(tr.train_steps(buf, 5, 16).clone(), tr.actor.net(PROBE.to(DEV)).clone()) for tr in src]
    fresh = [build(3), build(4)]
    for tr, st in zip(fresh, states):
        tr.load_resume_state(st)
        same(tr.resume_state(), st, "round trip")
    group = SeedGroup(fresh)
    losses = group.train_steps(buf, 5, 16, return_losses=True)
    group.synchronize()
    group.close()
    for k in range(2):
        assert torch.equal(losses[k], want[k][0]) and torch.equal(fresh[k].actor.net(PROBE.to(DEV)), want[k][1])
        same(fresh[k].resume_state(), src[k].resume_state(), f"seed {k} after the next steps")


# --------------------------------------------------------------------------- #
# sweep.train_runs
# --------------------------------------------------------------------------- #
SWEEP_RUNS = [dict(seed=3, max_timesteps=20, eval_freq=10), dict(seed=4, max_timesteps=40, eval_freq=10, beta=5.0),
              dict(seed=5, max_timesteps=40, eval_freq=20, log_freq=5), dict(seed=6, max_timesteps=30, eval_freq=10)]


def sweep_run(cfgs, data, cut_after=None):
    """-> (trainers or None, per-run records, per-run evaluation calls).  ``cut_after``: the logger raises at
    the first record behind that step (the boundary at that step is complete then)."""
    import iqlpref_amd as ia
    records = [[] for _ in cfgs]
    evs = [make_evaluate() for _ in cfgs]

    def logger(d, step):
        if cut_after is not None and step > cut_after:
            raise Cut(f"behind step {cut_after}")
        records[d["run"]].append((int(step), strip(dict(d))))

    trainers = None
    try:
        trainers = ia.train_runs(cfgs, ENV, {k: np.array(v) for k, v in data.items()}, runs_per_gpu=4, logger=logger,
                                 evaluate=[e[0] for e in evs], resume=True)
    except Cut:
        assert cut_after is not None
    return trainers, records, [e[1] for e in evs]


def test_sweep_train_runs_resumes_a_regrouped_batch(tmp_path, monkeypatch):
    from iqlpref_amd import _resume, multi
    data = synth(300)
    whole_cfgs = [offline_config(tmp_path / f"whole{i}", **kw) for i, kw in enumerate(SWEEP_RUNS)]
    whole = sweep_run(whole_cfgs, data)
    cfgs = [offline_config(tmp_path / f"cut{i}", **kw) for i, kw in enumerate(SWEEP_RUNS)]
    first = sweep_run(cfgs, data, cut_after=20)
    assert first[0] is None
    assert [_resume.status(c.checkpoints_path) for c in cfgs] == ["done", "at step 20", "at step 20", "at step 20"]
    groups = []
    real_init = multi.SeedGroup.__init__

    def init(self, trainers, *a, **k):
        groups.append([t._seed for t in trainers])
        real_init(self, trainers, *a, **k)

    monkeypatch.setattr(multi.SeedGroup, "__init__", init)
    second = sweep_run(cfgs, data)
    monkeypatch.setattr(multi.SeedGroup, "__init__", real_init)
    assert [g for g in groups if len(g) == 3][0] == [4, 5, 6] and not any(3 in g for g in groups)
    assert second[1][0] == [] and second[2][0] == []  # the first run: done, neither trained nor evaluated again
    for i in range(4):
        assert upto(first[1][i], 20) + second[1][i] == whole[1][i], i
        assert [c for c in first[2][i] if c[0] <= 20] + second[2][i] == whole[2][i], i
        same_trees(cfgs[i].checkpoints_path, whole_cfgs[i].checkpoints_path, f"run {i}")
        assert second[0][i].total_it == SWEEP_RUNS[i]["max_timesteps"]
    same_trainers(second[0], whole[0], "sweep")


# --------------------------------------------------------------------------- #
# custom_offline.train / train_runs
# --------------------------------------------------------------------------- #
CS, CA = 45, 24
CUSTOM_RUNS = [(5, 3), (6, 4), (7, 5)]  # (reward-model seed, train_seed)


def qmlp(seed):
    from iqlpref_amd import custom_offline as co
    return co.QMLP(CS, CA, (32,), "relu", "none").load_flax_params(cte.reward_layers(seed, CS, CA)).to(DEV)


def custom_config(path, model_seed, train_seed):
    from iqlpref_amd import custom_offline as co
    return co.TrainConfig(update_steps=30, eval_every=10, batch_size=32, eval_episodes=2, eval_seed=4,
                          train_seed=train_seed, actor_dropout=0.1, reward_model_path=f"m{model_seed}",
                          checkpoints_path=str(path))


def custom_logger(records, cut_from=None):
    def logger(d, step):
        if cut_from is not None and step >= cut_from:
            raise Cut(f"at step {cut_from}")
        d = dict(d)
        records[d.pop("run", 0)].append((int(step), d))
    return logger


@pytest.mark.parametrize("sampler", ["device", "host"])
def test_custom_offline_train_resumed_is_the_uninterrupted_run(tmp_path, sampler, request):
    from iqlpref_amd import custom_offline as co
    normalized = lambda ds, returns: 0.5 + 2.0 * np.asarray(returns)
    entered = np.random.get_state()
    request.addfinalizer(lambda: np.random.set_state(entered))  # this flavour trains on numpy's global generator
    for model_seed, train_seed in CUSTOM_RUNS:
        def run(cfg, cut_from=None):
            records = [[]]
            try:
                tr = co.train(cfg, cte.MinariDataset(11, (23, 17, 30)), qmlp(model_seed), sampler=sampler, device=DEV,
                              logger=custom_logger(records, cut_from), normalized_score=normalized, resume=True)
            except Cut:
                tr = None
            return tr, records[0], np.random.get_state()

        whole_cfg = custom_config(tmp_path / f"whole{train_seed}", model_seed, train_seed)
        whole = run(whole_cfg)
        cfg = custom_config(tmp_path / f"cut{train_seed}", model_seed, train_seed)
        first = run(cfg, cut_from=10)  # the first record of step 10 comes when generation 10 is committed
        assert first[0] is None and os.path.isfile(os.path.join(cfg.checkpoints_path, "resume_10.pt"))
        np.random.seed(12345)  # (whatever the process did in between)
        second = run(cfg)
        assert second[1][0][0] == 10 and [s for s, d in first[1] if "value_loss" in d] == list(range(10))
        assert first[1] + second[1] == whole[1], train_seed
        same_trees(cfg.checkpoints_path, whole_cfg.checkpoints_path, f"seed {train_seed}")
        same_trainers(second[0], whole[0], f"seed {train_seed}")
        # numpy's global generator -- this flavour's index stream -- stands where the uninterrupted run's does
        assert second[2][0] == whole[2][0] and np.array_equal(second[2][1], whole[2][1]) and second[2][2:] == whole[2][2:]


@pytest.mark.parametrize("sampler", ["device", "host"])
def test_custom_offline_train_runs_resumed_is_the_uninterrupted_run(tmp_path, sampler):
    from iqlpref_amd import _resume
    from iqlpref_amd import custom_offline as co
    normalized = lambda ds, returns: 0.5 + 2.0 * np.asarray(returns)

    def run(cfgs, cut_from=None):
        records = [[] for _ in cfgs]
        try:
            trs = co.train_runs(cfgs, cte.MinariDataset(11, (23, 17, 30)), {f"m{s}": qmlp(s) for s, _ in CUSTOM_RUNS},
                                sampler=sampler, logger=custom_logger(records, cut_from), normalized_score=normalized,
                                resume=True)
        except Cut:
            trs = None
        return trs, records

    whole_cfgs = [custom_config(tmp_path / f"whole{i}", *r) for i, r in enumerate(CUSTOM_RUNS)]
    whole = run(whole_cfgs)
    cfgs = [custom_config(tmp_path / f"cut{i}", *r) for i, r in enumerate(CUSTOM_RUNS)]
    first = run(cfgs, cut_from=10)
    assert first[0] is None and [_resume.status(c.checkpoints_path) for c in cfgs] == ["at step 10"] * 3
    second = run(cfgs)
    for i in range(3):
        assert first[1][i] + second[1][i] == whole[1][i], i
        same_trees(cfgs[i].checkpoints_path, whole_cfgs[i].checkpoints_path, f"run {i}")
        # every run's generator state after the resumed run is the uninterrupted run's
        a = _resume.read(cfgs[i].checkpoints_path, 30)["sampler"]
        b = _resume.read(whole_cfgs[i].checkpoints_path, 30)["sampler"]
        assert torch.equal(a["key"], b["key"]) and a["pos"] == b["pos"]
        want = np.random.RandomState(CUSTOM_RUNS[i][1])
        for _ in range(30):
            want.randint(0, 70, size=32)
        assert np.array_equal(a["key"].numpy().astype(np.uint32), want.get_state()[1]) and a["pos"] == want.get_state()[2]
    assert whole[1][0] != whole[1][1]
    same_trainers(second[0], whole[0], "custom sweep")


# --------------------------------------------------------------------------- #
# two ranks
# --------------------------------------------------------------------------- #
def test_two_ranks_resume_their_own_seeds_from_a_common_generation(tmp_path):
    """Two rank processes of ``train(seeds_per_gpu=2, resume=True)`` on one GPU (gloo), both cut in the evaluation
    at step 30 and started again: they hold two generations (10 and 20), agree on step 20, and every rank's
    records and final files are those of the uninterrupted two-rank job."""
    import json
    import socket
    import subprocess
    import sys
    from iqlpref_amd import _resume
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    ports = set()

    def start(name, ckpt, cut_at):
        out = tmp_path / name
        out.mkdir()
        port = None
        while port is None or port in ports:  # (two jobs at a time: never one port for both)
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
        ports.add(port)
        base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK")}
        base.update(WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                    IQL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        return out, [subprocess.Popen([sys.executable, os.path.join(root, "tests", "resume_rank_child.py"), str(out),
                                       str(tmp_path / ckpt), str(cut_at)], env=dict(base, RANK=str(r), LOCAL_RANK=str(r)),
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]

    def finish(started, cut):
        out, procs = started
        try:
            outs = [p.communicate(timeout=300) for p in procs]
        finally:  # (whatever happened: no child stays behind on the GPU)
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        for p, (_, se) in zip(procs, outs):
            assert (p.returncode != 0) == cut, se[-3000:]
        return [json.load(open(out / f"rank{r}.json")) for r in range(2)]

    # (the uninterrupted job and the job that is cut run side by side: four processes, two rendezvous)
    whole_job, first_job = start("whole", "ck_whole", 0), start("first", "ck_cut", 30)
    try:
        whole = finish(whole_job, False)
    finally:
        first = finish(first_job, True)
    for r in range(2):  # ranks keep the generation before too: whatever moment a rank dies at, both have one in common
        assert [_resume.steps_in(str(tmp_path / "ck_cut" / f"rank{r}" / f"seed_{100 + 2 * r + k}")) for k in range(2)] \
            == [[10, 20]] * 2
    second = finish(start("second", "ck_cut", 0), False)
    for r in range(2):
        assert second[r]["seeds"] == whole[r]["seeds"] == [100 + 2 * r, 101 + 2 * r]
        assert second[r]["total_it"] == [40, 40] and second[r]["param_sum"] == whole[r]["param_sum"]
        assert second[r]["logs"][0][0] == 24
        assert [rec for rec in first[r]["logs"] if rec[0] <= 20] + second[r]["logs"] == whole[r]["logs"], r
        same_trees(str(tmp_path / "ck_cut" / f"rank{r}"), str(tmp_path / "ck_whole" / f"rank{r}"), f"rank {r}")
    assert len({ps for rec in whole for ps in rec["param_sum"]}) == 4
