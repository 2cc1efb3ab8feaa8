#!/usr/bin/env python3
"""Generate tests/golden/bb_train_run.npz by RUNNING the reference's BB flavour
(algorithms/custom_offline/iql_bb.py, "bref") on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_bb_fixture.py [--ref /root/reference]

bref is imported at run time with inert stubs for the packages that are absent (orbax, flax, wandb,
pyrallis, tqdm when missing, ``load_PT``, and h5py backed by an in-memory stand-in that serves the
synthetic dataset of tests/bb_env.py).  Its own classes then run as written:

* training: ``IQL_H5Dataset`` + ``fast_loader`` + ``ImplicitQLearning`` driven by the loop of
  bref:892-970 for 12 steps = two epochs of 5 whole blocks and a tail of 7 rows;
* evaluation: one ``bb_run_eval_IQL`` call (2 episodes, max_horizon 40) with a small fixed actor, the
  numpy reward of tests/bb_env.py, every state / action / reward recorded.

Only arrays are stored: inputs, the permutation, batches, losses, records, and of every parameter / moment
tensor its float64 sum plus the tensor itself when small, else its first row (the file stays under 1 MiB)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import bb_env  # noqa: E402

STEPS, TRAIN_SEED, PERM_SEED, EVAL_SEED = 12, 3, 123, 9
EVAL = dict(num_episodes=2, max_horizon=40, hidden=16, actor_seed=19, gain_in=3.0, gain=6.0)
H5_PATH = "<in-memory bb dataset>"


class _MemoryH5:
    """h5py.File over a dict of arrays: context manager + item access, nothing else is used."""

    def __init__(self, arrays):
        self._a = arrays

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, key):
        return self._a[key]


def import_bb_reference(ref_root, arrays):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("orbax")
    stub("orbax.checkpoint")
    sys.modules["orbax"].checkpoint = sys.modules["orbax.checkpoint"]
    stub("pyrallis", wrap=lambda *a, **k: (lambda f: f))
    stub("wandb")
    stub("flax", nnx=types.SimpleNamespace())
    stub("iqlpref")
    stub("iqlpref.reward_models")
    stub("iqlpref.reward_models.pref_transformer", load_PT=None)
    try:
        import tqdm.auto  # noqa: F401
    except ImportError:
        stub("tqdm")
        stub("tqdm.auto", trange=range)
    stub("h5py", File=lambda path, mode="r": _MemoryH5(arrays))
    path = os.path.join(ref_root, "algorithms", "custom_offline", "iql_bb.py")
    spec = importlib.util.spec_from_file_location("ref_bb_iql", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    keep_path = list(sys.path)
    spec.loader.exec_module(mod)
    sys.path[:] = keep_path
    return mod


SMALL = 512  # tensors up to this many elements are stored whole, of the larger ones the float64 sum and the first row


def summarise(prefix, t, out):
    a = t.detach().numpy()
    out[f"{prefix}/sum"] = np.float64(t.detach().double().sum().item())
    if a.size <= SMALL:
        out[f"{prefix}/full"] = a.copy()
    else:
        out[f"{prefix}/row0"] = a[0].copy()


def flat_params(trainer):
    out = {}
    for net, module in (("qf", trainer.qf), ("vf", trainer.vf), ("actor", trainer.actor), ("q_target", trainer.q_target)):
        for k, v in module.state_dict().items():
            summarise(f"{net}/{k}", v, out)
    return out


def training_record(bref, out):
    """bref:892-970 with the services stripped: the dataset, the loader (its permutation is drawn
    BEFORE the training seed is set, as in bref), the nets, 12 steps."""
    B = bb_env.BATCH
    data = bref.IQL_H5Dataset(H5_PATH, normalized_states=True, normalized_rewards=True, device="cpu")
    torch.manual_seed(PERM_SEED)
    loader = bref.fast_loader(data, batch_size=B)
    out["perm"] = loader.sampler.sampler.batch_ids.numpy().astype(np.int64)
    interval = -(-len(data) // B)
    state_dim, action_dim = data.shapes()[0][1], data.shapes()[1][1]
    max_actions, min_actions = data.max_actions(), data.min_actions()
    out["stats/max_actions"] = max_actions.numpy()
    out["stats/min_actions"] = min_actions.numpy()
    out["stats/state_mean"], out["stats/state_std"] = data.state_mean(), data.state_std()

    batches = []
    real_get = bref.IQL_H5Dataset.__getitem__
    bref.IQL_H5Dataset.__getitem__ = lambda self, index: (batches.append(list(index)), real_get(self, index))[1]
    try:
        bref.set_seed(TRAIN_SEED)
        q_network = bref.TwinQ(state_dim, action_dim)
        v_network = bref.ValueFunction(state_dim)
        actor = bref.GaussianPolicy(state_dim, action_dim, max_actions, min_actions, dropout=None)
        v_optimizer = torch.optim.Adam(v_network.parameters(), lr=3e-4)
        q_optimizer = torch.optim.Adam(q_network.parameters(), lr=3e-4)
        actor_optimizer = torch.optim.Adam(actor.parameters(), lr=3e-4)
        sched = bref.CosineAnnealingLR(actor_optimizer, STEPS)
        trainer = bref.ImplicitQLearning(
            max_actions=max_actions, min_actions=min_actions, actor=actor, actor_optimizer=actor_optimizer,
            actor_lr_scheduler=sched, q_network=q_network, q_optimizer=q_optimizer, v_network=v_network,
            v_optimizer=v_optimizer, device="cpu")
        for k, v in flat_params(trainer).items():
            out[f"init/{k}"] = v
        losses = []
        for step in range(STEPS):
            if step % interval == 0:
                tdl = iter(loader)
            log = trainer.train([b for b in next(tdl)])
            losses.append([log["value_loss"], log["q_loss"], log["actor_loss"]])
            for k, v in flat_params(trainer).items():
                out[f"step{step}/{k}"] = v
    finally:
        bref.IQL_H5Dataset.__getitem__ = real_get
    assert len(batches) == STEPS and sorted(len(b) for b in batches[:interval]) == [7] + [B] * 5
    out["losses"] = np.asarray(losses, np.float64)
    out["batch_len"] = np.asarray([len(b) for b in batches], np.int64)
    out["batch_rows"] = np.asarray([b + [-1] * (B - len(b)) for b in batches], np.int64)
    sd = trainer.state_dict()
    for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
        for i, st in sd[opt]["state"].items():
            summarise(f"final/{opt}/{i}/exp_avg", st["exp_avg"], out)
            summarise(f"final/{opt}/{i}/exp_avg_sq", st["exp_avg_sq"], out)
            out[f"final/{opt}/{i}/step"] = np.float64(float(st["step"]))
    out["final/last_lr"] = np.float64(sd["actor_lr_scheduler"]["_last_lr"][0])
    return data


def evaluation_record(bref, data, out):
    e = EVAL
    torch.manual_seed(e["actor_seed"])
    actor = bref.GaussianPolicy(bb_env.STATE_DIM, bb_env.ACTION_DIM, data.max_actions(), data.min_actions(),
                                hidden_dim=e["hidden"])
    with torch.no_grad():
        # a steep first layer (the normalised state moves by ~0.01 per step: the action then changes along an
        # episode) and a large last one (tanh saturates both ways): the speed clamp is hit on both sides
        actor.net.net[0].weight.mul_(e["gain_in"])
        actor.net.net[0].weight[:, -4:] = 0.0  # (level .. day are not normalised and constant in an episode)
        actor.net.net[4].weight.mul_(e["gain"])
    states, actions, rewards = [], [], []

    class Recorder:
        eval, train = actor.eval, actor.train

        @staticmethod
        def act(state, device="cpu"):
            states.append(np.array(state))
            actions.append(actor.act(state, device))
            return actions[-1]

    def r_model(s, a, t, m, training=False):
        res = bb_env.numpy_reward(s, a, t, m, training=training)
        rewards.append(np.array(res[0]["value"][:, 0, -1]))
        return res

    returns = bref.bb_run_eval_IQL(Recorder, e["num_episodes"], r_model, bb_env.MOVE_STATS,
                                   state_mean=data.state_mean(), state_std=data.state_std(),
                                   max_horizon=e["max_horizon"], seed=EVAL_SEED, device="cpu")
    acts = np.asarray(actions)
    assert acts.dtype == np.float32
    lo, hi = data.min_actions().numpy(), data.max_actions().numpy()
    assert (acts[:, 0] == lo[0]).any() and (acts[:, 0] == hi[0]).any(), "the speed clamp must be hit on both sides"
    assert ((acts[:, 0] > lo[0]) & (acts[:, 0] < hi[0])).any(), "and some actions must lie inside it"
    for k, v in actor.state_dict().items():
        out[f"eval/actor/{k}"] = v.numpy()
    out["eval/states"] = np.asarray(states, np.float64)
    out["eval/actions"] = acts
    out["eval/rewards"] = np.asarray(rewards, np.float64)
    out["eval/returns"] = np.asarray(returns, np.float64)
    out["eval/seed"], out["eval/num_episodes"] = np.int64(EVAL_SEED), np.int64(e["num_episodes"])
    out["eval/max_horizon"] = np.int64(e["max_horizon"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    arrays = bb_env.synth_dataset()
    bref = import_bb_reference(args.ref, arrays)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    out = {f"data/{k}": v for k, v in arrays.items()}
    out["move_stats"] = np.asarray(bb_env.MOVE_STATS, np.float64)
    out["train_seed"], out["perm_seed"] = np.int64(TRAIN_SEED), np.int64(PERM_SEED)
    data = training_record(bref, out)
    evaluation_record(bref, data, out)
    path = os.path.join(HERE, "bb_train_run.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), f"{size} bytes: over the limit for a committed fixture"
    print(f"wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
