"""offline_bc.train() (algorithms/offline/any_percent_bc.py, "dbc") on the HIP step and the device selection.  -m gpu.

1. replays tests/golden/offline_bc_run.npz -- the reference's own train() on the CPU (make_offline_bc_fixture.py)
   -- record for record, with sampler="host" and sampler="device" bit-identical;
2. seeds_per_gpu=3 equals three runs of one seed, bit for bit;
3. load_model continues the reference's own checkpoint as the reference's train() continued it;
4. eval_actor on the stand-in environment gives the reference's returns for the reference's weights.
The bounds are those of tests/test_gpu_minari_bc.py (the fixture's length was chosen under them): losses rtol 2e-5,
returns and scores 1e-5, weights 5e-6.
"""
import os

import numpy as np
import pytest
import torch

from tests import minari_cases as mc, offline_bc_env as obe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load(golden_dir, "offline_bc_run.npz")


def _run(tmp, seed, seeds_per_gpu=1, sampler="device", max_timesteps=45, eval_freq=15, load_model="", **kw):
    """Our train() on the fixture's inputs; returns (config, records, saves, evaluation returns, trainer(s))."""
    from iqlpref_amd import offline_bc
    config = offline_bc.TrainConfig(env=obe.ENV, max_timesteps=max_timesteps, eval_freq=eval_freq, batch_size=64, n_episodes=2,
                                    frac=obe.FRAC, max_traj_len=7, seed=seed, checkpoints_path=str(tmp), load_model=load_model)
    records, saves, evals = [], [], []
    real_save, real_eval = torch.save, offline_bc.eval_actor

    def save(obj, path):
        saves.append((records[-1][0], os.path.relpath(path, config.checkpoints_path)))
        real_save(obj, path)

    def eval_actor(*a, **k):
        evals.append(real_eval(*a, **k))
        return evals[-1]

    logger = lambda d, step: records.extend((int(step), k, v, int(d.get("seed", -1))) for k, v in d.items() if k != "seed")
    torch.save, offline_bc.eval_actor = save, eval_actor
    try:
        out = offline_bc.train(config, obe.make_dataset(11), obe.OfflineBCEnv(), logger=logger, seeds_per_gpu=seeds_per_gpu,
                               sampler=sampler, device=DEV, **kw)
    finally:
        torch.save, offline_bc.eval_actor = real_save, real_eval
    return config, records, saves, np.asarray(evals), out


def _check_checkpoint(sd, g, fname):
    assert sorted(sd) == list(g[f"{fname}/keys"]) == ["actor", "actor_optimizer", "total_it"]
    assert sd["total_it"] == g[f"{fname}/total_it"]
    assert list(sd["actor"]) == list(mc.NAMES)
    for k, v in sd["actor"].items():
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


def _check_records(records, saves, evals, g, n_losses):
    steps = np.asarray([r[0] for r in records])
    keys = np.asarray([r[1] for r in records])
    vals = np.asarray([r[2] for r in records], np.float64)
    np.testing.assert_array_equal(keys, g["rec_key"])
    np.testing.assert_array_equal(steps, g["rec_step"])
    loss = keys == "actor_loss"
    assert loss.sum() == n_losses and set(keys) == {"actor_loss", "d4rl_normalized_score"}
    np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=2e-5, atol=2e-8)
    np.testing.assert_allclose(vals[~loss], g["rec_value"][~loss], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(evals, g["eval_returns"], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
    np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])
    # numpy's global generator: exactly where the reference's host draws left it
    st = np.random.get_state()
    np.testing.assert_array_equal(st[1], g["np_key"])
    assert st[2] == g["np_pos"] and st[3] == g["np_has_gauss"] and st[4] == g["np_cached"]


def test_replays_reference_train(golden, tmp_path):
    g = mc.run_of(golden, "run")
    runs = {}
    for sampler in ("device", "host"):
        config, records, saves, evals, tr = _run(tmp_path / sampler, int(g["train_seed"]), sampler=sampler)
        runs[sampler] = (config, records, saves, np.random.get_state())
        _check_records(records, saves, evals, g, 45)
        assert sorted(os.listdir(config.checkpoints_path)) == sorted(g["save_name"]) + ["config.yaml"]
        for _, fname in saves:
            _check_checkpoint(torch.load(os.path.join(config.checkpoints_path, fname), weights_only=True), g, fname)
        assert tr.total_it == 45 and tr.discount == 0.99
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


def test_float64_rewards_take_the_host_selection_and_train_the_same(golden, tmp_path):
    """float64 rewards go through keep_best_trajectories on the host; with this dataset's distinct returns the kept
    rows are the same, so the run is the float32 run's -- bit for bit on everything but the rewards, which the
    step never reads."""
    from iqlpref_amd import offline_bc
    recs = []
    for dtype in (np.float32, np.float64):
        config = offline_bc.TrainConfig(env=obe.ENV, max_timesteps=20, eval_freq=10, batch_size=64, n_episodes=2, frac=obe.FRAC,
                                        seed=3)
        rec = []
        offline_bc.train(config, obe.make_dataset(11, dtype), obe.OfflineBCEnv(), logger=lambda d, s: rec.append((s, dict(d))),
                         device=DEV)
        recs.append(rec)
    assert recs[0] == recs[1] and len(recs[0]) == 22


def test_seeds_per_gpu_equals_solo_runs(tmp_path):
    """seeds_per_gpu=3: seed k trains bit-identically to train() of seed 3 + k alone -- the loss of every step, the
    evaluation records, every checkpoint file, the final parameters and the seed's index stream."""
    cfg_g, rec_g, saves_g, _, trainers = _run(tmp_path / "group", 3, seeds_per_gpu=3, max_timesteps=120, eval_freq=50)
    assert len(trainers) == 3
    for k in range(3):
        cfg_s, rec_s, saves_s, _, solo = _run(tmp_path / f"solo{k}", 3 + k, max_timesteps=120, eval_freq=50)
        mine = [(s, key, v) for s, key, v, seed in rec_g if seed == 3 + k]
        assert mine == [(s, key, v) for s, key, v, _ in rec_s], f"seed {3 + k}: records differ"
        mine_saves = [(s, f) for s, f in saves_g if f.startswith(f"seed_{3 + k}{os.sep}")]
        assert [(s, f.split(os.sep, 1)[1]) for s, f in mine_saves] == saves_s
        assert [f for _, f in saves_s] == ["checkpoint_49.pt", "checkpoint_99.pt"]
        for _, f in saves_s:
            a = torch.load(os.path.join(cfg_g.checkpoints_path, f"seed_{3 + k}", f), weights_only=True)
            b = torch.load(os.path.join(cfg_s.checkpoints_path, f), weights_only=True)
            assert a["total_it"] == b["total_it"]
            for key in b["actor"]:
                assert torch.equal(a["actor"][key], b["actor"][key]), f"seed {3 + k} {f} {key}"
            for i, s in b["actor_optimizer"]["state"].items():
                for key in ("exp_avg", "exp_avg_sq", "step"):
                    assert torch.equal(a["actor_optimizer"]["state"][i][key], s[key])
        for p, q in zip(trainers[k].actor.parameters(), solo.actor.parameters()):
            assert torch.equal(p, q)
        assert trainers[k].total_it == solo.total_it == 120


def _reference_checkpoint(g):
    fname, sd = mc.bc_state_dict(g)
    sd["total_it"] = int(g[f"{fname}/total_it"])
    group = sd["actor_optimizer"]["param_groups"][0]
    group["betas"] = tuple(float(b) for b in group["betas"])  # (plain floats: the file is read with weights_only)
    return fname, sd


def test_load_model_continues_the_references_checkpoint(golden, tmp_path):
    """The reference's checkpoint that the fixture keeps whole, through ``config.load_model``: the records go on from
    the file's total_it and are those of the reference's own train() continued from that file."""
    g, cont = mc.run_of(golden, "run"), mc.run_of(golden, "cont")
    fname, ref_sd = _reference_checkpoint(g)
    it0 = ref_sd["total_it"]
    assert fname == str(cont["candidates"][-1]) and it0 == int(fname[len("checkpoint_"):-len(".pt")]) + 1
    path = tmp_path / "reference_checkpoint.pt"
    torch.save(ref_sd, path)
    steps = int(cont["steps"])
    config, records, saves, evals, tr = _run(tmp_path / "cont", int(g["train_seed"]), max_timesteps=steps,
                                             load_model=str(path))
    _check_records(records, saves, evals, cont, steps)
    assert records[0][0] == it0 + 1 and tr.total_it == it0 + steps
    last = saves[-1][1]
    sd = torch.load(os.path.join(config.checkpoints_path, last), weights_only=True)
    _check_checkpoint(sd, cont, last)
    # and the file goes through BC.load_state_dict unchanged
    from iqlpref_amd import offline_bc
    torch.manual_seed(99)
    actor = offline_bc.Actor(17, 6, 1.0).to(DEV)
    bc = offline_bc.BC(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), 0.99, DEV)
    bc.load_state_dict(ref_sd)
    back = bc.state_dict()
    assert back["total_it"] == it0
    for k, v in ref_sd["actor"].items():
        assert torch.equal(back["actor"][k].cpu(), v), k
    for i, s in ref_sd["actor_optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["actor_optimizer"]["state"][i][k].cpu(), s[k]), (i, k)
    with pytest.raises(ValueError, match="total_it"):
        bc.load_state_dict(dict(ref_sd, total_it=it0 - 1))


def test_eval_actor_on_the_references_weights(golden):
    """The reference evaluated the weights of the checkpoint kept whole right before it wrote it: eval_actor with those
    weights on a fresh environment, normalised with the statistics of the selected rows, gives its two returns."""
    from iqlpref_amd import offline_bc
    g = mc.run_of(golden, "run")
    _, ref_sd = _reference_checkpoint(g)
    d = obe.make_dataset(11)
    offline_bc.keep_best_trajectories(d, obe.FRAC, 0.99)
    mean, std = offline_bc.compute_mean_std(d["observations"], eps=1e-3)
    env = offline_bc.wrap_env(obe.OfflineBCEnv(), state_mean=mean, state_std=std)
    actor = offline_bc.Actor(17, 6, 1.0).to(DEV)
    actor.load_state_dict(ref_sd["actor"])
    got = offline_bc.eval_actor(env, actor, DEV, 2, int(g["train_seed"]))
    assert actor.training and got.dtype == np.float64
    want = g["eval_returns"][ref_sd["total_it"] // 15 - 1]  # (evaluations every 15 steps)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    again = offline_bc.eval_actor(env, actor, DEV, 2, int(g["train_seed"]))
    np.testing.assert_array_equal(got, again)  # env.seed(seed) at the start of every call
