"""custom_offline_br.train() (bref = algorithms/custom_offline/iql_br.py:625-778) on the HIP path.  -m gpu.

Replays tests/golden/br_train_run.npz -- one run of the reference's own train() on the CPU
(make_br_fixture.py): the relabel is the median of 10 posterior draws taken from numpy's global
generator BEFORE set_seed(train_seed), and the normalized score falls as the return rises, so the step
bref keeps as best (by mean return) is not the one the custom flavour's rule would keep.  Bounds and step
count are those of tests/test_gpu_custom_train.py (2e-5 on the fp32 losses, 60 steps).
"""
import os

import numpy as np
import pytest
import torch

from tests import br_env
from tests import custom_train_env as cte

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ("value_loss", "q_loss", "actor_loss")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "br_train_run.npz")))


def _run(tmp, g, reward_model, **kw):
    from iqlpref_amd import custom_offline_br as br
    dataset = cte.MinariDataset(int(g["common/data_seed"]), tuple(g["common/lengths"]))
    config = br.TrainConfig(update_steps=int(g["common/update_steps"]), eval_every=int(g["common/eval_every"]),
                            batch_size=int(g["common/batch_size"]), eval_episodes=int(g["common/eval_episodes"]),
                            eval_seed=int(g["common/eval_seed"]), train_seed=int(g["train_seed"]),
                            checkpoints_path=str(tmp), reward_type=int(g["reward_type"]), n_samples=int(g["n_samples"]))
    records, saves = [], []
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.relpath(path, config.checkpoints_path)))
        real_save(obj, path)

    a, b = g["affine"]
    logger = lambda d, step: records.extend((int(step), k, v) for k, v in d.items())
    np.random.seed(int(g["relabel_seed"]))
    torch.save = save
    try:
        out = br.train(config, dataset, reward_model, logger=logger,
                       normalized_score=lambda ds, r: a + b * np.asarray(r), device=DEV, **kw)
    finally:
        torch.save = real_save
    return config, records, saves, out


@pytest.mark.parametrize("sampler", ["device", "host"])
def test_replays_reference_train(golden, tmp_path, sampler):
    g = golden
    assert g["best_by_return"] != g["best_by_normalized"]  # the run on which the two best-model rules part
    # the reference's predictions to the bit (the median then is too): 287 rows at batch 64 overfit fast,
    # and last-ulp differences of the rewards would grow with the steps (as in test_gpu_custom_train.py)
    model = br_env.RecordedPosterior(g["preds"], None, DEV)
    config, records, saves, _ = _run(tmp_path, g, model, sampler=sampler)
    steps = np.asarray([r[0] for r in records])
    keys = np.asarray([r[1] for r in records])
    vals = np.asarray([r[2] for r in records], np.float64)
    np.testing.assert_array_equal(keys, g["rec_key"])
    np.testing.assert_array_equal(steps, g["rec_step"])
    loss = np.isin(keys, LOSSES)
    assert loss.sum() == 3 * 60
    print("max rel loss error", np.abs(vals[loss] / g["rec_value"][loss] - 1).max())
    np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=2e-5, atol=2e-8)
    exact = keys == "best_step_so_far"
    np.testing.assert_array_equal(vals[exact], g["rec_value"][exact])
    assert vals[exact][-1] == g["best_by_return"]
    rest = ~loss & ~exact
    np.testing.assert_allclose(vals[rest], g["rec_value"][rest], rtol=1e-5, atol=1e-5)
    assert "normalized_score" in keys  # still logged
    np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
    np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])
    st = np.random.get_state()
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


def test_train_with_networks_on_the_device(golden, tmp_path):
    """The same run with the posterior networks themselves on the device (predictions by the HIP MLP,
    within 2e-5 of the stand-in's): the relabel consumes the same stream, so numpy's generator ends where
    the reference left it and the same files are written."""
    from iqlpref_amd import custom_offline_br as br
    g = golden
    env = cte.MinariEnv()
    sets = br_env.posterior_layers(int(g["post_seed"]), int(g["n_post"]), env.S, env.A, int(g["hidden"]))
    model = br.PosteriorRewardNet(sets, None, "relu", DEV)
    _, records, saves, trainer = _run(tmp_path, g, model)
    assert isinstance(trainer, br.ImplicitQLearning)
    np.testing.assert_array_equal([r[1] for r in records], g["rec_key"])
    # (which evaluations improve on the best may turn on the last bits of the rewards: periodic files only)
    assert [s[1] for s in saves if s[1].startswith("checkpoint_")] == \
        [n for n in g["save_name"] if n.startswith("checkpoint_")]
    st = np.random.get_state()
    np.testing.assert_array_equal(st[1], g["np_key"])
    assert st[2] == g["np_pos"]
