"""custom_offline.train() (cref:597-749) on the HIP path.  -m gpu.

1. replays tests/golden/custom_train_run.npz -- two runs of the reference's own train() on the CPU
   (make_custom_train_fixture.py) -- record for record;
2. ImplicitQLearning.train_on_buffer: sampler="device" equals sampler="host" bit for bit;
3. seeds_per_gpu=3 equals three runs of one seed, bit for bit.
"""
import os

import numpy as np
import pytest
import torch

from tests import custom_train_env as cte

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ("value_loss", "q_loss", "actor_loss")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "custom_train_run.npz")))


def _normalizer(affine):
    def f(ds, returns):
        if affine is None:
            raise ValueError("no reference scores for this dataset")
        return affine[0] + affine[1] * np.asarray(returns)
    return f


def _run(tmp, train_seed, affine=None, seeds_per_gpu=1, sampler="device", update_steps=60, eval_every=20, qmlp=True,
         **kw):
    """Our train() on the fixture's inputs; returns (config, records, saves, trainer(s)).  ``qmlp=False``
    relabels with the fixture's own numpy reward function instead of a QMLP on the GPU."""
    from iqlpref_amd import custom_offline as co
    dataset = cte.MinariDataset(11, (40, 55, 33, 60, 47, 52))
    env = dataset.recover_environment()
    layers = cte.reward_layers(5, env.S, env.A)
    if qmlp:
        rm = co.QMLP(env.S, env.A, (32,), "relu", "none").load_flax_params(layers).to(DEV)
    else:
        host = cte.numpy_reward(layers)
        rm = lambda obs, act: torch.from_numpy(host(obs, act))
    config = co.TrainConfig(update_steps=update_steps, eval_every=eval_every, batch_size=64, eval_episodes=2, eval_seed=4,
                            train_seed=train_seed, checkpoints_path=str(tmp))
    records, saves = [], []
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.relpath(path, config.checkpoints_path)))
        real_save(obj, path)

    logger = lambda d, step: records.extend((int(step), k, v, int(d.get("seed", -1))) for k, v in d.items()
                                            if k != "seed")
    torch.save = save
    try:
        out = co.train(config, dataset, rm, logger=logger, normalized_score=_normalizer(affine),
                       seeds_per_gpu=seeds_per_gpu, sampler=sampler, device=DEV, **kw)
    finally:
        torch.save = real_save
    return config, records, saves, out


@pytest.mark.parametrize("name", ["raw", "norm"])
def test_replays_reference_train(name, golden, tmp_path):
    g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    affine = None if np.isnan(g["affine"]).any() else tuple(g["affine"])
    # the reference's rewards to the bit: 287 rows at batch 64 overfit fast, and the QMLP's last-ulp
    # differences (test_gpu_custom_offline.py checks it) would grow with the steps
    config, records, saves, _ = _run(tmp_path, int(g["train_seed"]), affine, qmlp=False)
    steps = np.asarray([r[0] for r in records])
    keys = np.asarray([r[1] for r in records])
    vals = np.asarray([r[2] for r in records], np.float64)
    np.testing.assert_array_equal(keys, g["rec_key"])
    np.testing.assert_array_equal(steps, g["rec_step"])
    loss = np.isin(keys, LOSSES)
    assert loss.sum() == 3 * 60
    # the per-step losses: fp32 arithmetic of a different summation order, as the train_runs replay; the
    # atol covers value losses of ~1e-4, whose last-bit rounding alone is ~1e-8
    np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=2e-5, atol=2e-8)
    # best_step_so_far exactly; returns and scores to 1e-5: the fake environment integrates the actions
    # of the fp32 actor over 5..13 steps, and the actor weights of the two runs differ by a few ulp
    # (test_gpu_reference_runs.py holds the offline flavour's evaluation to the same 1e-5)
    exact = keys == "best_step_so_far"
    np.testing.assert_array_equal(vals[exact], g["rec_value"][exact])
    rest = ~loss & ~exact
    np.testing.assert_allclose(vals[rest], g["rec_value"][rest], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
    np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])
    # numpy's global generator: exactly where the reference's 60 host draws left it
    st = np.random.get_state()
    np.testing.assert_array_equal(st[1], g["np_key"])
    assert st[2] == g["np_pos"] and st[3] == g["np_has_gauss"] and st[4] == g["np_cached"]
    last = [s[1] for s in saves if s[1].startswith("checkpoint_")][-1]
    for tag, fname in (("best", "best_model.pt"), ("last", last)):
        sd = torch.load(os.path.join(config.checkpoints_path, fname), weights_only=True)
        assert set(sd) == {"qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer", "actor_lr_scheduler"}
        for net, full in (("actor", "net.net.4.weight"), ("vf", "v.net.4.weight"), ("qf", "q1.net.4.weight")):
            # after 20-60 fp32 Adam steps the weights agree to ~1e-6 (test_gpu_reference_runs.py: 2e-6)
            np.testing.assert_allclose(sd[net][full].cpu().numpy(), g[f"{tag}/{net}/{full}"], atol=5e-6, rtol=0,
                                       err_msg=f"{tag}/{net}/{full}")
            for k, v in sd[net].items():
                want = g[f"{tag}/{net}/{k}/sum"]
                np.testing.assert_allclose(v.double().sum().item(), want, rtol=1e-5, atol=2e-6 * v.numel(),
                                           err_msg=f"{tag}/{net}/{k}")
        for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
            for i, s in sd[opt]["state"].items():
                assert float(s["step"]) == g[f"{tag}/{opt}/{i}/step"]
                for k in ("exp_avg", "exp_avg_sq"):
                    np.testing.assert_allclose(s[k].double().sum().item(), g[f"{tag}/{opt}/{i}/{k}/sum"],
                                               rtol=1e-3, atol=1e-6 * s[k].numel(), err_msg=f"{tag}/{opt}/{i}/{k}")
        assert sd["actor_lr_scheduler"]["last_epoch"] == g[f"{tag}/actor_lr_scheduler/last_epoch"]


def test_train_on_buffer_device_sampler_equals_host():
    """The same chunks with indices drawn on the host and on the device: identical losses, parameters
    and final state of numpy's global generator."""
    import iqlpref_amd as ia
    from iqlpref_amd import custom_offline as co
    S, A, n_rows, B = 45, 24, 3001, 64
    rng = np.random.default_rng(0)
    data = {"observations": rng.standard_normal((n_rows, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (n_rows, A)).astype(np.float32),
            "rewards": rng.standard_normal(n_rows).astype(np.float32),
            "next_observations": rng.standard_normal((n_rows, S)).astype(np.float32),
            "terminals": (rng.uniform(size=n_rows) < 0.05).astype(np.float32)}
    runs = {}
    for sampler in ("host", "device"):
        torch.manual_seed(1)
        q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), ia.GaussianPolicy(S, A, 1.0).to(DEV)
        ao = torch.optim.Adam(actor.parameters(), lr=3e-4)
        tr = co.ImplicitQLearning(1.0, actor, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, 1000), q,
                                  torch.optim.Adam(q.parameters(), lr=3e-4), v,
                                  torch.optim.Adam(v.parameters(), lr=3e-4), device=DEV, seed=1)
        buf = co.ReplayBuffer(S, A, n_rows, DEV)
        buf.load_dataset(data)
        np.random.seed(9)
        np.random.standard_normal()  # a cached gaussian that no draw may touch
        losses = torch.cat([tr.train_on_buffer(buf, n, B, sampler=sampler) for n in (100, 7, 150, 43)])
        torch.cuda.synchronize()
        runs[sampler] = (losses.cpu(), tr.state_dict(), np.random.get_state())
    (lh, sdh, sth), (ld, sdd, std) = runs["host"], runs["device"]
    assert torch.equal(lh, ld)
    for net in ("qf", "vf", "actor"):
        for k in sdh[net]:
            assert torch.equal(sdh[net][k], sdd[net][k]), f"{net}/{k}"
    np.testing.assert_array_equal(sth[1], std[1])
    assert sth[2:] == std[2:]


def test_seeds_per_gpu_equals_solo_runs(tmp_path):
    """seeds_per_gpu=3: seed k trains bit-identically to train() of seed 3 + k alone -- losses of
    every step, evaluation records, final parameters and every checkpoint file."""
    cfg_g, rec_g, saves_g, trainers = _run(tmp_path / "group", 3, seeds_per_gpu=3, update_steps=250, eval_every=100)
    assert len(trainers) == 3
    for k in range(3):
        cfg_s, rec_s, saves_s, solo = _run(tmp_path / f"solo{k}", 3 + k, update_steps=250, eval_every=100)
        mine = [(s, key, v) for s, key, v, seed in rec_g if seed == 3 + k]
        assert mine == [(s, key, v) for s, key, v, _ in rec_s], f"seed {3 + k}: records differ"
        mine_saves = [(s, f) for s, f in saves_g if f.startswith(f"seed_{3 + k}{os.sep}")]
        assert [(s, f.split(os.sep, 1)[1]) for s, f in mine_saves] == saves_s
        for _, f in saves_s:
            a = torch.load(os.path.join(cfg_g.checkpoints_path, f"seed_{3 + k}", f), weights_only=True)
            b = torch.load(os.path.join(cfg_s.checkpoints_path, f), weights_only=True)
            for net in ("qf", "vf", "actor"):
                for key in b[net]:
                    assert torch.equal(a[net][key], b[net][key]), f"seed {3 + k} {f} {net}/{key}"
            for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
                for i, s in b[opt]["state"].items():
                    for key in ("exp_avg", "exp_avg_sq"):
                        assert torch.equal(a[opt]["state"][i][key], s[key])
        for p, q in zip(trainers[k].actor.parameters(), solo.actor.parameters()):
            assert torch.equal(p, q)
        for p, q in zip(trainers[k].qf.parameters(), solo.qf.parameters()):
            assert torch.equal(p, q)

