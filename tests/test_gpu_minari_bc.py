"""minari_bc.train() (algorithms/minari/any_percent_bc.py, "bcref") on the HIP step.  -m gpu.

1. replays tests/golden/minari_bc_run.npz -- two runs of the reference's own train() on the CPU
   (make_minari_fixture.py) -- record for record, with sampler="host" and sampler="device" bit-identical;
2. seeds_per_gpu=3 equals three runs of one seed, bit for bit;
3. a state dict the reference wrote loads and continues the reference's run; one written here has its keys.
The bounds are those of tests/test_gpu_custom_train.py's replay (the fixture's length was chosen under them).
"""
import os

import numpy as np
import pytest
import torch

from tests import minari_cases as mc, minari_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load(golden_dir, "minari_bc_run.npz")


def _normalizer(affine):
    def f(ds, returns):
        if affine is None:
            raise ValueError("no reference scores for this dataset")
        return affine[0] + affine[1] * np.asarray(returns)
    return f


def _run(tmp, train_seed, affine=None, seeds_per_gpu=1, sampler="device", update_steps=45, eval_every=15, **kw):
    """Our train() on the fixture's inputs; returns (config, records, saves, trainer(s))."""
    from iqlpref_amd import minari_bc
    dataset = minari_env.MinariDataset(11)
    config = minari_bc.TrainConfig(update_steps=update_steps, eval_every=eval_every, batch_size=64, eval_episodes=2,
                                   eval_seed=4, train_seed=train_seed, top_fraction=minari_env.TOP_FRACTION,
                                   checkpoints_path=str(tmp))
    records, saves = [], []
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.relpath(path, config.checkpoints_path)))
        real_save(obj, path)

    logger = lambda d, step: records.extend((int(step), k, v, int(d.get("seed", -1))) for k, v in d.items()
                                            if k != "seed")
    torch.save = save
    try:
        out = minari_bc.train(config, dataset, logger=logger, normalized_score=_normalizer(affine),
                              seeds_per_gpu=seeds_per_gpu, sampler=sampler, device=DEV, **kw)
    finally:
        torch.save = real_save
    return config, records, saves, out


def _check_checkpoint(sd, g, fname):
    assert sorted(sd) == list(g[f"{fname}/keys"]) == ["actor", "actor_optimizer"]
    assert list(sd["actor"]) == list(mc.NAMES)
    for k, v in sd["actor"].items():
        # after 15-45 fp32 Adam steps the weights agree to ~1e-6 (test_gpu_custom_train.py: the same bounds)
        np.testing.assert_allclose(v.double().sum().item(), g[f"{fname}/actor/{k}/sum"], rtol=1e-5, atol=2e-6 * v.numel(),
                                   err_msg=f"{fname}/{k}")
        if f"{fname}/actor/{k}" in g:
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{fname}/actor/{k}"], atol=5e-6, rtol=0, err_msg=f"{fname}/{k}")
    state = sd["actor_optimizer"]["state"]
    assert sorted(state) == list(range(6))
    for i, s in state.items():
        assert float(s["step"]) == g[f"{fname}/actor_optimizer/{i}/step"]
        for k in ("exp_avg", "exp_avg_sq"):
            np.testing.assert_allclose(s[k].double().sum().item(), g[f"{fname}/actor_optimizer/{i}/{k}/sum"], rtol=1e-3,
                                       atol=1e-6 * s[k].numel(), err_msg=f"{fname}/{i}/{k}")
    group = sd["actor_optimizer"]["param_groups"][0]
    assert group["lr"] == 3e-4 and group["params"] == list(range(6))


@pytest.mark.parametrize("name", ["raw", "norm"])
def test_replays_reference_train(name, golden, tmp_path):
    g = mc.run_of(golden, name)
    affine = None if np.isnan(g["affine"]).any() else tuple(g["affine"])
    runs = {}
    for sampler in ("device", "host"):
        config, records, saves, tr = _run(tmp_path / sampler, int(g["train_seed"]), affine, sampler=sampler)
        runs[sampler] = (config, records, saves, np.random.get_state())
        steps = np.asarray([r[0] for r in records])
        keys = np.asarray([r[1] for r in records])
        vals = np.asarray([r[2] for r in records], np.float64)
        np.testing.assert_array_equal(keys, g["rec_key"])  # (no best_* records: the reference's loop has none)
        np.testing.assert_array_equal(steps, g["rec_step"])
        loss = keys == "actor_loss"
        assert loss.sum() == 45 and set(keys) == {"actor_loss", "evaluation_return"} | ({"normalized_score"} if affine else set())
        np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=2e-5, atol=2e-8)
        np.testing.assert_allclose(vals[~loss], g["rec_value"][~loss], rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
        np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])
        assert sorted(f for f in os.listdir(config.checkpoints_path) if f.endswith(".pt")) == sorted(g["save_name"])
        # numpy's global generator: exactly where the reference's 45 host draws left it
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], g["np_key"])
        assert st[2] == g["np_pos"] and st[3] == g["np_has_gauss"] and st[4] == g["np_cached"]
        for _, fname in saves:
            _check_checkpoint(torch.load(os.path.join(config.checkpoints_path, fname), weights_only=True), g, fname)
        assert tr.total_it == 45
    (cd, rd, sd, std), (ch, rh, sh, sth) = runs["device"], runs["host"]
    assert rd == rh and sd == sh  # every record, bit for bit
    np.testing.assert_array_equal(std[1], sth[1])
    assert std[2:] == sth[2:]
    for _, fname in sd:
        a = torch.load(os.path.join(cd.checkpoints_path, fname), weights_only=True)
        b = torch.load(os.path.join(ch.checkpoints_path, fname), weights_only=True)
        for k in a["actor"]:
            assert torch.equal(a["actor"][k], b["actor"][k]), f"{fname} {k}"
        for i, s in a["actor_optimizer"]["state"].items():
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(s[k], b["actor_optimizer"]["state"][i][k]), f"{fname} {i}/{k}"


def test_seeds_per_gpu_equals_solo_runs(tmp_path):
    """seeds_per_gpu=3: seed k trains bit-identically to train() of seed 3 + k alone -- the loss of every step, the
    evaluation records, every checkpoint file, the final parameters and the seed's index stream."""
    cfg_g, rec_g, saves_g, trainers = _run(tmp_path / "group", 3, seeds_per_gpu=3, update_steps=120, eval_every=50)
    assert len(trainers) == 3
    for k in range(3):
        cfg_s, rec_s, saves_s, solo = _run(tmp_path / f"solo{k}", 3 + k, update_steps=120, eval_every=50)
        # the solo run drew from numpy's global generator seeded with 3 + k; the group's member from a
        # RandomState(3 + k) of its own: identical losses mean identical index streams
        mine = [(s, key, v) for s, key, v, seed in rec_g if seed == 3 + k]
        assert mine == [(s, key, v) for s, key, v, _ in rec_s], f"seed {3 + k}: records differ"
        mine_saves = [(s, f) for s, f in saves_g if f.startswith(f"seed_{3 + k}{os.sep}")]
        assert [(s, f.split(os.sep, 1)[1]) for s, f in mine_saves] == saves_s and len(saves_s) == 2
        for _, f in saves_s:
            a = torch.load(os.path.join(cfg_g.checkpoints_path, f"seed_{3 + k}", f), weights_only=True)
            b = torch.load(os.path.join(cfg_s.checkpoints_path, f), weights_only=True)
            for key in b["actor"]:
                assert torch.equal(a["actor"][key], b["actor"][key]), f"seed {3 + k} {f} {key}"
            for i, s in b["actor_optimizer"]["state"].items():
                for key in ("exp_avg", "exp_avg_sq", "step"):
                    assert torch.equal(a["actor_optimizer"]["state"][i][key], s[key])
        for p, q in zip(trainers[k].actor.parameters(), solo.actor.parameters()):
            assert torch.equal(p, q)
        assert trainers[k].total_it == solo.total_it == 120


def test_reference_state_dict_loads_and_continues(golden, tmp_path):
    """The reference's checkpoint_14.pt (kept whole in the fixture) goes into a fresh BC; steps 15 .. 44 on the
    reference's indices then give the reference's losses and its last checkpoint."""
    from iqlpref_amd import custom_offline as co, minari_bc
    from iqlpref_amd.iql import compute_mean_std, normalize_states
    g = mc.run_of(golden, "raw")
    fname, ref_sd = mc.bc_state_dict(g)
    ds = minari_env.MinariDataset(11)
    q = minari_bc.qlearning_dataset(ds, minari_bc.best_trajectories_ids(ds, minari_env.TOP_FRACTION, 0.99))
    mean, std = compute_mean_std(q["observations"], eps=1e-3)
    q["observations"] = normalize_states(q["observations"], mean, std)
    q["next_observations"] = normalize_states(q["next_observations"], mean, std)
    buf = co.ReplayBuffer(45, 24, 1000, DEV)
    buf.load_dataset(q)
    torch.manual_seed(99)  # (another initialisation: everything must come from the file)
    actor = minari_bc.Actor(45, 24, 1.0).to(DEV)
    tr = minari_bc.BC(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), DEV)
    tr.train_steps(buf, 2, 64, indices=torch.zeros((2, 64), dtype=torch.int64, device=DEV))  # (a used trainer)
    tr.load_state_dict(ref_sd)
    assert tr.total_it == 15
    back = tr.state_dict()
    for k, v in ref_sd["actor"].items():
        assert torch.equal(back["actor"][k].cpu(), v), k
    for i, s in ref_sd["actor_optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["actor_optimizer"]["state"][i][k].cpu(), s[k]), (i, k)
        assert float(back["actor_optimizer"]["state"][i]["step"]) == 15.0
    np.random.seed(int(g["train_seed"]))
    idx = buf.draw_indices(64, 45)[15:]  # the reference's draws of steps 15 .. 44
    losses = tr.train_steps(buf, 30, 64, indices=torch.from_numpy(idx).to(DEV)).cpu().numpy()[:, 0]
    want = g["rec_value"][g["rec_key"] == "actor_loss"][15:]
    np.testing.assert_allclose(losses, want, rtol=2e-5, atol=2e-8)
    _check_checkpoint(tr.state_dict(), g, "checkpoint_44.pt")


class _WideEnv:
    """129 observations: one beyond the step's envelope."""

    def __init__(self):
        from tests import fake_envs
        self.observation_space, self.action_space = fake_envs._Box(129, np.inf), fake_envs._Box(24, 1.0)


def test_train_refuses_a_shape_outside_the_envelope(tmp_path):
    """state_dim 129: NotImplementedError from the trainer's construction -- no handle, no launch, no record."""
    from iqlpref_amd import minari_bc
    rng = np.random.default_rng(0)
    episodes = [minari_env.Episode(i, rng.standard_normal((9, 129)), rng.uniform(-1, 1, (8, 24)), rng.standard_normal(8),
                                   np.zeros(8, bool)) for i in range(4)]
    records = []
    with pytest.raises(NotImplementedError, match="state_dim 129"):
        minari_bc.train(minari_bc.TrainConfig(update_steps=4, eval_every=2, batch_size=8, top_fraction=0.5), episodes,
                        _WideEnv(), logger=lambda d, step: records.append(d), device=DEV)
    assert not records
