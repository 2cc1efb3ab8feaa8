"""minari_iql.train() (algorithms/minari/iql.py, "mref") on the HIP path.  -m gpu.

1. replays tests/golden/minari_iql_run.npz -- two runs of the reference's own train() on the CPU
   (make_minari_fixture.py) -- record for record, the best-model records included;
2. its best_model.pt loads through posthoc's actor loader and acts as the trainer's actor does;
3. resume=True after a cut at the second evaluation boundary gives the uninterrupted run's files, bit for bit.
The bounds are those of tests/test_gpu_custom_train.py's replay (the fixture's length was chosen under them).
"""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import minari_cases as mc, minari_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ("value_loss", "q_loss", "actor_loss")
STEPS, EVERY = 45, 15


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load(golden_dir, "minari_iql_run.npz")


def _normalizer(affine):
    def f(ds, returns):
        if affine is None:
            raise ValueError("no reference scores for this dataset")
        return affine[0] + affine[1] * np.asarray(returns)
    return f


def _config(tmp, train_seed):
    from iqlpref_amd import minari_iql
    return minari_iql.TrainConfig(update_steps=STEPS, eval_every=EVERY, batch_size=64, eval_episodes=2, eval_seed=4,
                                  train_seed=train_seed, checkpoints_path=str(tmp))


def _run(config, affine=None, logger=None, **kw):
    """Our train() on the fixture's inputs; returns (records, saves, trainer)."""
    from iqlpref_amd import minari_iql
    records, saves = [], []
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0] if records else -1, os.path.relpath(path, config.checkpoints_path)))
        real_save(obj, path)

    if logger is None:
        logger = lambda d, step: records.extend((int(step), k, v) for k, v in d.items())
    torch.save = save
    try:
        out = minari_iql.train(config, minari_env.MinariDataset(11), logger=logger, normalized_score=_normalizer(affine),
                               device=DEV, **kw)
    finally:
        torch.save = real_save
    return records, saves, out


@pytest.mark.parametrize("name", ["raw", "norm"])
def test_replays_reference_train(name, golden, tmp_path):
    from iqlpref_amd import posthoc
    g = mc.run_of(golden, name)
    affine = None if np.isnan(g["affine"]).any() else tuple(g["affine"])
    config = _config(tmp_path, int(g["train_seed"]))
    records, saves, tr = _run(config, affine)
    steps = np.asarray([r[0] for r in records])
    keys = np.asarray([r[1] for r in records])
    vals = np.asarray([r[2] for r in records], np.float64)
    np.testing.assert_array_equal(keys, g["rec_key"])
    np.testing.assert_array_equal(steps, g["rec_step"])
    loss = np.isin(keys, LOSSES)
    assert loss.sum() == 3 * STEPS and (keys == "best_score_so_far").sum() == 3
    np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=2e-5, atol=2e-8)
    exact = keys == "best_step_so_far"
    np.testing.assert_array_equal(vals[exact], g["rec_value"][exact])
    rest = ~loss & ~exact
    np.testing.assert_allclose(vals[rest], g["rec_value"][rest], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
    np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])
    st = np.random.get_state()  # numpy's global generator: where the reference's 45 host draws left it
    np.testing.assert_array_equal(st[1], g["np_key"])
    assert st[2] == g["np_pos"] and st[3] == g["np_has_gauss"] and st[4] == g["np_cached"]
    last = [s[1] for s in saves if s[1].startswith("checkpoint_")][-1]
    for tag, fname in (("best", "best_model.pt"), ("last", last)):
        sd = torch.load(os.path.join(config.checkpoints_path, fname), weights_only=True)
        assert set(sd) == {"qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer", "actor_lr_scheduler"}
        for net, full in (("actor", "net.net.4.weight"), ("vf", "v.net.4.weight"), ("qf", "q1.net.4.weight")):
            np.testing.assert_allclose(sd[net][full].cpu().numpy(), g[f"{tag}/{net}/{full}"], atol=5e-6, rtol=0,
                                       err_msg=f"{tag}/{net}/{full}")
            for k, v in sd[net].items():
                np.testing.assert_allclose(v.double().sum().item(), g[f"{tag}/{net}/{k}/sum"], rtol=1e-5,
                                           atol=2e-6 * v.numel(), err_msg=f"{tag}/{net}/{k}")
        for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
            for i, s in sd[opt]["state"].items():
                assert float(s["step"]) == g[f"{tag}/{opt}/{i}/step"]
                for k in ("exp_avg", "exp_avg_sq"):
                    np.testing.assert_allclose(s[k].double().sum().item(), g[f"{tag}/{opt}/{i}/{k}/sum"],
                                               rtol=1e-3, atol=1e-6 * s[k].numel(), err_msg=f"{tag}/{opt}/{i}/{k}")
        assert sd["actor_lr_scheduler"]["last_epoch"] == g[f"{tag}/actor_lr_scheduler/last_epoch"]
    # the config on disk carries this program's group and no reward model
    with open(os.path.join(config.checkpoints_path, "config.yaml")) as f:
        written = yaml.safe_load(f)
    assert written["group"] == "IQL-Minari" and "reward_model_path" not in written and "query_length" not in written
    # posthoc reads the best model: the policy it builds acts as the checkpoint's tensors say
    path = os.path.join(config.checkpoints_path, "best_model.pt")
    actor = posthoc.load_actor(path, 45, 24, 1.0, False, DEV)
    best = torch.load(path, weights_only=True)["actor"]
    for k, v in actor.state_dict().items():
        assert torch.equal(v.cpu(), best[k].cpu()), k
    obs = np.random.default_rng(5).standard_normal(45)
    assert np.all(np.isfinite(actor.act(obs, DEV))) and actor.act(obs, DEV).shape == (24,)


class Cut(Exception):
    pass


def _tree(root):
    out = {}
    for d, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            path = os.path.join(d, f)
            if f == "config.yaml":
                with open(path) as fh:
                    c = yaml.safe_load(fh)
                out[f] = {k: v for k, v in c.items() if k not in ("name", "checkpoints_path")}
            else:
                out[os.path.relpath(path, root)] = torch.load(path, weights_only=True)
    return out


def _same(a, b, where=""):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            if not str(k).startswith("steps_per_sec"):  # (wall-clock fields)
                _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


def test_resumed_after_a_cut_is_the_uninterrupted_run(tmp_path, request):
    """The run is killed by its logger at the first record of step 30 -- inside the chunk after the second
    evaluation boundary, whose generation (step 30) is then the newest complete one -- and started again."""
    entered = np.random.get_state()
    request.addfinalizer(lambda: np.random.set_state(entered))  # this program trains on numpy's global generator

    def run(cfg, cut_from=None):
        records = []

        def logger(d, step):
            if cut_from is not None and step >= cut_from:
                raise Cut(f"at step {cut_from}")
            records.append((int(step), dict(d)))
        try:
            _, _, tr = _run(cfg, (2.0, 0.5), logger=logger, resume=True)
        except Cut:
            tr = None
        return tr, records, np.random.get_state()

    whole_cfg = _config(tmp_path / "whole", 7)
    whole = run(whole_cfg)
    cfg = _config(tmp_path / "cut", 7)
    first = run(cfg, cut_from=2 * EVERY)
    assert first[0] is None and os.path.isfile(os.path.join(cfg.checkpoints_path, f"resume_{2 * EVERY}.pt"))
    np.random.seed(12345)  # (whatever the process did in between)
    second = run(cfg)
    assert second[1][0][0] == 2 * EVERY
    assert first[1] + second[1] == whole[1]
    ta, tb = _tree(cfg.checkpoints_path), _tree(whole_cfg.checkpoints_path)
    assert list(ta) == list(tb) and any(f.startswith("resume_") for f in ta)
    _same(ta, tb, "files")
    _same(second[0].resume_state(), whole[0].resume_state(), "trainer")
    assert np.array_equal(second[2][1], whole[2][1]) and second[2][2:] == whole[2][2:]
