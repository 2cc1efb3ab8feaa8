"""The train() programs of the flavours at batch sizes that are no multiple of 16: losses and final state
bit-identical to a hand-written loop of train_steps over indices drawn on the host.  -m gpu.

  custom_offline.train       40 steps at batch_size 100
  custom_offline_bb.train    250 rows at batch_size 100: two whole blocks and a tail slot with n_valid = 50
  finetune.train             two offline steps and five online ticks at batch_size 24
"""
import copy

import numpy as np
import pytest
import torch

from tests import bb_env
from tests import custom_train_env as cte
from tests import finetune_env as fe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ("value_loss", "q_loss", "actor_loss")


def _losses_of(records, n):
    """[n, 3] float32 out of (step, key, value) logger records."""
    vals = [v for _, k, v in records if k in LOSSES]
    assert len(vals) == 3 * n
    return np.asarray(vals, np.float64).reshape(n, 3).astype(np.float32)


def _same(tr, twin, got, want):
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, want.cpu().numpy())
    assert tr.total_it == twin.total_it
    for what in ("_params", "_exp_avg", "_exp_avg_sq", "_target"):
        assert torch.equal(getattr(tr, what), getattr(twin, what)), what


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def test_custom_offline_train_at_batch_100(tmp_path, monkeypatch):
    from iqlpref_amd import custom_offline as co
    N, B, seed = 40, 100, 3
    dataset = cte.MinariDataset(11, (40, 55, 33, 60, 47, 52))
    env = dataset.recover_environment()
    host = cte.numpy_reward(cte.reward_layers(5, env.S, env.A))
    config = co.TrainConfig(update_steps=N, eval_every=N, batch_size=B, eval_episodes=1, eval_seed=4, train_seed=seed,
                            checkpoints_path=str(tmp_path))
    loaded, records = {}, []
    real_load = co.ReplayBuffer.load_dataset

    def load(self, data):
        loaded.update({k: np.array(v) for k, v in data.items()})
        return real_load(self, data)

    def no_score(ds, returns):
        raise ValueError("no reference scores for this dataset")

    monkeypatch.setattr(co.ReplayBuffer, "load_dataset", load)
    tr = co.train(config, dataset, lambda obs, act: torch.from_numpy(host(obs, act)), device=DEV,
                  logger=lambda d, step: records.extend((int(step), k, v) for k, v in d.items()),
                  normalized_score=no_score, sampler="device")
    monkeypatch.setattr(co.ReplayBuffer, "load_dataset", real_load)
    assert tr.step_kind(B) == "tuned"

    co.set_seed(seed)
    twin = co._build_trainer(config, seed, env.S, env.A, (float(env.action_space.high[0]),), DEV)
    buf = co.ReplayBuffer(env.S, env.A, config.buffer_size, DEV)
    buf.load_dataset(loaded)
    idx = np.stack([np.random.randint(0, buf.index_bound(), size=B) for _ in range(N)])
    want = twin.train_steps(buf, N, B, indices=_dev(idx))
    _same(tr, twin, _losses_of(records, N), want)


def test_bb_train_on_250_rows_at_batch_100(tmp_path, monkeypatch):
    from iqlpref_amd import custom_offline as co
    from iqlpref_amd import custom_offline_bb as bb
    N, B, rows, seed = 7, 100, 250, 5  # two epochs of three slots and the first slot of a third
    perm = np.asarray([1, 0])
    config = bb.TrainConfig(update_steps=N, eval_every=N, batch_size=B, normalize_state=True, normalize_reward=True,
                            eval_episodes=1, train_seed=seed, eval_seed=4, checkpoints_path=str(tmp_path))
    records = []
    real_eval = bb.bb_run_eval_IQL
    monkeypatch.setattr(bb, "bb_run_eval_IQL", lambda **kw: real_eval(**dict(kw, max_horizon=20)))
    tr = bb.train(config, bb_env.synth_dataset(21, rows), bb_env.numpy_reward, bb_env.MOVE_STATS, perm=perm, device=DEV,
                  logger=lambda d, step: records.extend((int(step), k, float(v)) for k, v in d.items()), chunk=4)
    assert tr.step_kind(B) == "tuned"

    ds = bb.BBDataset(bb_env.synth_dataset(21, rows), normalized_states=True, normalized_rewards=True, device=DEV)
    (_, S), (_, A) = ds.shapes()
    limits = (ds.max_actions().to(DEV), ds.min_actions().to(DEV))
    bb.set_seed(seed)
    twin = co._build_trainer(config, seed, S, A, limits, DEV, (bb.GaussianPolicy, bb.DeterministicPolicy),
                             bb.ImplicitQLearning)
    buf = bb.ReplayBuffer(S, A, len(ds), DEV)
    buf.load_dataset(ds.transitions())
    idx, valid = bb.BlockEpochSampler(rows, B, perm=perm).host_indices(0, N)
    assert valid.tolist() == [B, B, 50, B, B, 50, B]
    want = twin.train_steps(buf, N, B, indices=_dev(idx), n_valid=_dev(valid, torch.int32))
    _same(tr, twin, _losses_of(records, N), want)


def test_finetune_ticks_at_batch_24():
    from iqlpref_amd import finetune as ft
    name, B, n_off, n_on, cap, seed = "halfcheetah-medium-v2", 24, 2, 5, 200, 7
    dataset = fe.make_dataset(name, 61, seed=1)
    config = ft.TrainConfig(device=DEV, env=name, seed=seed, eval_seed=3, eval_freq=1000, n_episodes=1,
                            offline_iterations=n_off, online_iterations=n_on, checkpoints_path=None, buffer_size=cap,
                            batch_size=B, normalize_reward=False)
    eps = np.random.default_rng(2).standard_normal((n_on, fe.A)).astype(np.float32)
    records, box, added = [], {}, []

    def on_start(trainer, buf):
        box["np"] = np.random.get_state()
        box["sd"] = copy.deepcopy(trainer.state_dict())
        box["rows"] = buf.index_bound()
        real_add = buf.add_transition

        def add(*a):
            added.append(tuple(np.array(x) if isinstance(x, np.ndarray) else x for x in a))
            return real_add(*a)
        buf.add_transition = add

    tr = ft.train(config, fe.FinetuneEnv(name), fe.FinetuneEnv(name), dataset, device=DEV,
                  logger=lambda d, step: records.extend((int(step), k, float(v)) for k, v in d.items()),
                  exploration_noise=lambda tick: eps[tick], on_start=on_start)
    assert tr.step_kind(B) == "tuned" and len(added) == n_on

    q, v = ft.TwinQ(fe.S, fe.A).to(DEV), ft.ValueFunction(fe.S).to(DEV)
    actor = (ft.DeterministicPolicy if config.iql_deterministic else ft.GaussianPolicy)(fe.S, fe.A, 1.0).to(DEV)
    twin = ft.ImplicitQLearning(max_action=1.0, actor=actor,
                                actor_optimizer=torch.optim.Adam(actor.parameters(), lr=config.actor_lr), q_network=q, q_optimizer=torch.optim.Adam(q.parameters(), lr=config.qf_lr), v_network=v,
                                v_optimizer=torch.optim.Adam(v.parameters(), lr=config.vf_lr), discount=config.discount,
                                tau=config.tau, device=DEV, beta=config.beta, iql_tau=config.iql_tau, max_steps=n_off,
                                seed=seed)
    twin.load_state_dict(box["sd"])
    buf = ft.ReplayBuffer(fe.S, fe.A, cap, DEV)
    buf.load_d4rl_dataset(dataset)  # (train() left the normalised arrays in the dict it was given)
    n0 = buf.index_bound()
    assert n0 == box["rows"] == 61
    np.random.set_state(box["np"])
    idx = np.stack([np.random.randint(0, n0, size=B) for _ in range(n_off)])
    want = [twin.train_steps(buf, n_off, B, indices=_dev(idx))]
    online = [np.random.randint(0, min(n0 + 1 + t, cap), size=B) for t in range(n_on)]  # (drawn a chunk ahead)
    for t in range(n_on):
        buf.add_transition(*added[t])
        want.append(twin.train_steps(buf, 1, B, indices=_dev(online[t][None])))
    _same(tr, twin, _losses_of(records, n_off + n_on), torch.cat(want))
