#!/usr/bin/env python3
"""Generate tests/golden/minari_iql_run.npz and minari_bc_run.npz by RUNNING the reference's two Minari programs,
``algorithms/minari/iql.py`` ("mref") and ``algorithms/minari/any_percent_bc.py`` ("bcref"), on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_minari_fixture.py [--ref /root/reference] [--measure 150]

Each file is imported under inert stubs for the packages that are absent (gymnasium, minari, pyrallis, wandb,
tqdm); its ``train()`` then runs as written against stand-ins: the dataset of tests/minari_env.py (episodes with
``id`` and ``rewards``, a tie in return on the selection boundary, ``top_fraction * n`` = 3.15), the environment of
tests/custom_train_env.py, ``wandb.log`` recording every call, ``minari.get_normalized_score`` raising
``ValueError`` in run "raw" and affine in run "norm".  Only inputs and outputs are stored: the log records, the
checkpoint files written at each step, the selected ids, per-tensor sums and a few whole tensors of the
checkpoints, the final ``np.random.get_state()`` -- and, for the behaviour-cloning run "raw", the whole state dict
of its first checkpoint (the tensors as byte planes, which compress), from which ``BC.load_state_dict`` continues.

Length of the runs, and their seeds.  CPU and GPU fp32 trajectories part as rounding is amplified by Adam (a
gradient entry of any size, once it is not zero, moves its weight by about lr), so a record-for-record replay
holds for a limited number of steps only, and for some seeds hardly at all.  The generator measures that on the
reference itself: every run is repeated with the modules and the sampled data cast to float64 (same initial
weights, same indices, observations rounded to float32 first as the file says) and |fp32 - float64| of every
logged loss and of every evaluation return is held against the bounds tests/test_gpu_custom_train.py applies to
its replay: rtol 2e-5 with atol 2e-8 for the losses, rtol = atol = 1e-5 for the returns.  Measured over 150
steps (``--measure``), evaluations every 15, as fractions of those bounds:

    iql/raw   seed 3   losses: first 45 steps 0.02, none beyond in 150 (largest 0.09); returns: 0.00 .. 0.00
    bc/raw    seed 3   losses: first 45 steps 0.01, none beyond in 150 (largest 0.02); returns: 0.00 .. 0.01
    iql/norm  seed 7   losses: first 45 steps 0.06 (0.25 at step 49, 0.44 at step 57), beyond the bound at step 61
    iql/norm  seed 8   losses: 0.05, beyond at step 90; returns: 0.68, 0.56, 11.3, 15.6, 43.9, 8.5
    iql/norm  seed 9   losses: 0.02, none beyond (largest 0.16); returns: 0.00, 0.03, 0.19, 2.88, 4.73, 7.38
    iql/norm  seed 10  losses: 0.02, beyond at step 140; returns: 0.00, 0.00, 0.01, 0.01, 0.01, 0.01
    bc/norm   seeds 7 .. 10  losses: 0.01; returns: at most 0.10 (seed 7, step 90)

``update_steps`` = 45 with ``eval_every`` = 15 for both programs: the custom flavour's 60 steps are where the
IQL run of seed 7 reaches 0.44 of the bound, one step before it leaves it; 45 steps are three evaluation
boundaries (the resume test cuts at the second) at no more than 0.06.  A run is recorded only from a seed at
which both programs stay under the bounds for TWICE that length, losses and returns (``report``): the GPU is one
more restatement with a rounding pattern of its own, and a run that leaves the bound right behind its last
recorded step has no room for it.  The seed of a run is the first from its entry of ``RUNS`` on that does:
3 for "raw", 10 for "norm" (7, 8 and 9 do not, above).  The behaviour-cloning step is far calmer than the IQL
actor's: no exp(beta * advantage) weights, no second network in its loss.
"""
import argparse
import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import fake_envs, minari_env  # noqa: E402

# one entry per run: (first candidate train_seed, normalized score: None = raises ValueError, else (a, b): a + b * returns)
RUNS = {"raw": (3, None), "norm": (7, (2.0, 0.5))}  # (first candidate seed, score): see main()
COMMON = dict(update_steps=45, eval_every=15, batch_size=64, eval_episodes=2, eval_seed=4, data_seed=11,
              top_fraction=minari_env.TOP_FRACTION)
RTOL, ATOL = 2e-5, 2e-8  # tests/test_gpu_custom_train.py: the bound of its record-for-record replay, losses
EVAL_TOL = 1e-5          # the same test: rtol = atol of its evaluation returns and scores
IQL_FULL = {"actor": "net.net.4.weight", "vf": "v.net.4.weight", "qf": "q1.net.4.weight"}  # stored whole
BC_FULL = ("net.4.weight", "net.0.bias")


def import_reference(ref_root, rel_path, modname):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)  # (torch looks some of these names up with find_spec)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("gymnasium", Env=object,
         wrappers=types.SimpleNamespace(TransformObservation=fake_envs.TransformObservation,
                                        TransformReward=fake_envs.TransformReward))
    stub("minari", MinariDataset=object)
    stub("pyrallis", wrap=lambda *a, **k: (lambda f: f))
    stub("wandb")
    stub("tqdm")
    stub("tqdm.auto", trange=range)
    spec = importlib.util.spec_from_file_location(modname, os.path.join(ref_root, rel_path))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    keep_path = list(sys.path)
    spec.loader.exec_module(mod)
    sys.path[:] = keep_path
    return mod


def as_double(ref, trainer):
    """Swap the trainer class ``trainer`` of a reference file for a factory that casts every module it is handed to
    float64 first (in place: the fp32 initial weights, the same Parameter objects the optimisers hold), and its
    ReplayBuffer for one that samples float64 (the stored data are fp32 numbers).  Returns the function that
    puts the originals back."""
    saved = {n: getattr(ref, n) for n in (trainer, "ReplayBuffer")}

    def make(*a, **k):
        for v in list(a) + list(k.values()):
            if isinstance(v, torch.nn.Module):
                v.double()
        return saved[trainer](*a, **k)
    setattr(ref, trainer, make)

    class Torch64:  # the file's ``torch``: float32 tensors it builds from data (the observation in act()) in float64
        def __getattr__(self, name):
            return getattr(torch, name)

        def tensor(self, *a, **k):
            t = torch.tensor(*a, **k)  # (rounded to float32 first where the file says so: the same inputs)
            return t.double() if t.dtype is torch.float32 else t
    saved["torch"] = ref.torch
    ref.torch = Torch64()

    class Buffer(saved["ReplayBuffer"]):
        def sample(self, batch_size):
            return [t.double() for t in super().sample(batch_size)]
    ref.ReplayBuffer = Buffer

    def restore():
        for n, v in saved.items():
            setattr(ref, n, v)
    return restore


def install(ref, dataset, affine, records):
    def log(d, step):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    def normalized(ds, returns):
        if affine is None:
            raise ValueError("no reference scores for this dataset")
        return affine[0] + affine[1] * np.asarray(returns)

    ref.wandb = types.SimpleNamespace(init=lambda **kw: None, log=log)
    ref.minari = types.SimpleNamespace(download_dataset=lambda i: None, load_dataset=lambda i: dataset,
                                       get_normalized_score=normalized, MinariDataset=object)
    ref.pyrallis = types.SimpleNamespace(dump=lambda cfg, f: f.write(repr(cfg)))


def run_reference(ref, config_kw, train_seed, affine, tmp, update_steps, eval_every):
    """One run of ``ref.train``; returns (records, saves, {file name: state dict}, numpy state, dataset)."""
    c = COMMON
    dataset = minari_env.MinariDataset(c["data_seed"])
    records, saves = [], []
    install(ref, dataset, affine, records)
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    config = ref.TrainConfig(update_steps=update_steps, eval_every=eval_every, batch_size=c["batch_size"],
                             eval_episodes=c["eval_episodes"], eval_seed=c["eval_seed"], train_seed=train_seed,
                             checkpoints_path=tmp, **config_kw)
    torch.save = save
    try:
        ref.train(config)
    finally:
        torch.save = real_save
    files = {}
    if tmp is not None:
        files = {name: torch.load(os.path.join(config.checkpoints_path, name), weights_only=True)
                 for name in sorted({s[1] for s in saves})}
    return records, saves, files, np.random.get_state(), dataset


def loss_series(records, key):
    return np.asarray([r[2] for r in records if r[1] == key], np.float64)


def measure_gap(ref, trainer, config_kw, train_seed, keys, n_steps):
    """|fp32 - float64| of the logged losses ``keys`` per step and of the evaluation returns per evaluation, over
    ``n_steps`` steps, and the same as fractions of the replay's bounds; returns (loss gap [n_steps, len(keys)],
    float64 losses, loss fractions, evaluation gap [n_evals], float64 returns, evaluation fractions)."""
    runs, evals = [], []
    for double in (False, True):
        restore = as_double(ref, trainer) if double else (lambda: None)
        try:
            rec = run_reference(ref, config_kw, train_seed, None, None, n_steps, COMMON["eval_every"])[0]
        finally:
            restore()
        runs.append(np.stack([loss_series(rec, k) for k in keys], 1))
        evals.append(loss_series(rec, "evaluation_return"))
    gap, egap = np.abs(runs[0] - runs[1]), np.abs(evals[0] - evals[1])
    return (gap, runs[1], gap / (ATOL + RTOL * np.abs(runs[1])), egap, evals[1],
            egap / (EVAL_TOL + EVAL_TOL * np.abs(evals[1])))


def report(tag, seed, frac, efrac, steps, every):
    """Prints the figures of one candidate seed; True when the run may be recorded: the gap stays under the bound
    for TWICE the recorded length (losses and evaluations) -- the GPU is one more restatement with a rounding
    pattern of its own, and a run that leaves the bound right behind its last recorded step has no room for it."""
    beyond = np.nonzero((frac >= 1).any(1))[0]
    first = f"first step beyond it: {beyond[0]}" if beyond.size else f"none in {len(frac)} (largest {frac.max():.2f})"
    evals = ", ".join(f"{f:.2f}" for f in efrac[:2 * steps // every])
    print(f"    {tag:9s} seed {seed}: losses, first {steps} steps {frac[:steps].max():.2f} of the bound, {first}; "
          f"evaluations every {every} steps: {evals}")
    return frac[:2 * steps].max() < 1 and efrac[:2 * steps // every].max() < 1


def common_arrays(name, train_seed, affine, records, saves, state):
    return {f"{name}/train_seed": np.int64(train_seed),
            f"{name}/affine": np.asarray(affine if affine is not None else (np.nan, np.nan), np.float64),
            f"{name}/rec_step": np.asarray([r[0] for r in records], np.int64),
            f"{name}/rec_key": np.asarray([r[1] for r in records]),
            f"{name}/rec_value": np.asarray([r[2] for r in records], np.float64),
            f"{name}/save_step": np.asarray([s[0] for s in saves], np.int64),
            f"{name}/save_name": np.asarray([s[1] for s in saves]),
            f"{name}/np_key": np.asarray(state[1], np.uint32), f"{name}/np_pos": np.int64(state[2]),
            f"{name}/np_has_gauss": np.int64(state[3]), f"{name}/np_cached": np.float64(state[4])}


def iql_checkpoint_arrays(prefix, sd):
    out = {}
    for net in ("qf", "vf", "actor"):
        for k, v in sd[net].items():
            out[f"{prefix}/{net}/{k}/sum"] = np.float64(v.double().sum().item())
        out[f"{prefix}/{net}/{IQL_FULL[net]}"] = sd[net][IQL_FULL[net]].numpy()
    for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
        for i, st in sd[opt]["state"].items():
            for k in ("exp_avg", "exp_avg_sq"):
                out[f"{prefix}/{opt}/{i}/{k}/sum"] = np.float64(st[k].double().sum().item())
            out[f"{prefix}/{opt}/{i}/step"] = np.float64(float(st["step"]))
    out[f"{prefix}/actor_lr_scheduler/last_epoch"] = np.int64(sd["actor_lr_scheduler"]["last_epoch"])
    out[f"{prefix}/actor_lr_scheduler/last_lr"] = np.float64(sd["actor_lr_scheduler"]["_last_lr"][0])
    return out


def bc_checkpoint_arrays(prefix, sd, full):
    out = {f"{prefix}/keys": np.asarray(sorted(sd))}
    for k, v in sd["actor"].items():
        out[f"{prefix}/actor/{k}/sum"] = np.float64(v.double().sum().item())
    for k in BC_FULL if full else ():
        out[f"{prefix}/actor/{k}"] = sd["actor"][k].numpy()
    for i, st in sd["actor_optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"{prefix}/actor_optimizer/{i}/{k}/sum"] = np.float64(st[k].double().sum().item())
        out[f"{prefix}/actor_optimizer/{i}/step"] = np.float64(float(st["step"]))
    return out


def byte_planes(t):
    """An fp32 tensor as uint8 [4, n]: plane b holds byte b of every element (the exponent plane compresses)."""
    return np.ascontiguousarray(t.numpy().reshape(-1).view(np.uint8).reshape(-1, 4).T)


def bc_whole_state(prefix, sd):
    """Everything of a bcref state dict, to be rebuilt by the test (tests/minari_cases.py: bc_state_dict)."""
    out = {}
    for k, v in sd["actor"].items():
        out[f"{prefix}/actor/{k}/planes"] = byte_planes(v)
        out[f"{prefix}/actor/{k}/shape"] = np.asarray(v.shape, np.int64)
    for i, st in sd["actor_optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"{prefix}/actor_optimizer/{i}/{k}/planes"] = byte_planes(st[k])
        out[f"{prefix}/actor_optimizer/{i}/step"] = np.float64(float(st["step"]))
    g = sd["actor_optimizer"]["param_groups"][0]
    out[f"{prefix}/actor_optimizer/lr"] = np.float64(g["lr"])
    out[f"{prefix}/actor_optimizer/betas"] = np.asarray(g["betas"], np.float64)
    out[f"{prefix}/actor_optimizer/eps"] = np.float64(g["eps"])
    out[f"{prefix}/actor_optimizer/params"] = np.asarray(g["params"], np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--measure", type=int, default=150, help="steps of the fp32 / float64 gap measurement")
    args = ap.parse_args()
    mref = import_reference(args.ref, os.path.join("algorithms", "minari", "iql.py"), "ref_minari_iql")
    bcref = import_reference(args.ref, os.path.join("algorithms", "minari", "any_percent_bc.py"), "ref_minari_bc")
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    c = COMMON
    steps = c["update_steps"]
    bc_kw = dict(top_fraction=c["top_fraction"])
    iql, bc = ({f"common/{k}": np.asarray(v) for k, v in c.items()} for _ in range(2))
    print("measured fp32 / float64 loss gaps:")
    keys = ("value_loss", "q_loss", "actor_loss")
    n_measure = max(args.measure, 2 * steps)
    for name, (first_seed, affine) in RUNS.items():
        # the run's seed: the first from ``first_seed`` on at which both programs keep the margin (``report``)
        for seed in range(first_seed, first_seed + 16):
            gap, l64, frac, egap, e64, efrac = measure_gap(mref, "ImplicitQLearning", {}, seed, keys, n_measure)
            ok = report(f"iql/{name}", seed, frac, efrac, steps, c["eval_every"])
            bgap, bl64, bfrac, begap, be64, befrac = measure_gap(bcref, "BC", bc_kw, seed, ("actor_loss",), n_measure)
            if report(f"bc/{name}", seed, bfrac, befrac, steps, c["eval_every"]) and ok:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps the margin")
        # ---- task-reward IQL ----
        with tempfile.TemporaryDirectory() as tmp:
            records, saves, files, state, _ = run_reference(mref, {}, seed, affine, tmp, steps, c["eval_every"])
        iql.update(common_arrays(name, seed, affine, records, saves, state))
        iql[f"{name}/f64_gap_of_bound"] = frac[:steps]  # (of a run of n_measure steps: another cosine schedule)
        last = max((s for s in saves if s[1].startswith("checkpoint_")), key=lambda s: s[0])[1]
        iql.update(iql_checkpoint_arrays(f"{name}/best", files["best_model.pt"]))
        iql.update(iql_checkpoint_arrays(f"{name}/last", files[last]))
        # ---- any-percent BC ----
        with tempfile.TemporaryDirectory() as tmp:
            records, saves, files, state, dataset = run_reference(bcref, bc_kw, seed, affine, tmp, steps,
                                                                  c["eval_every"])
        bc.update(common_arrays(name, seed, affine, records, saves, state))
        bc[f"{name}/f64_gap"], bc[f"{name}/f64_loss"] = bgap[:steps, 0], bl64[:steps, 0]  # (BC has no schedule)
        last = max(saves, key=lambda s: s[0])[1]
        for fname, sd in files.items():  # (the whole tensors of the last checkpoint only)
            bc.update(bc_checkpoint_arrays(f"{name}/{fname}", sd, fname == last))
        if name == "raw":
            first = min((s for s in saves), key=lambda s: s[0])[1]
            bc[f"{name}/whole"] = np.asarray(first)
            bc.update(bc_whole_state(f"{name}/whole/{first}", files[first]))
    # ---- the selection by itself: ids and rows for both reward dtypes and several fractions ----
    for dtype in (np.float64, np.float32):
        ds = minari_env.MinariDataset(c["data_seed"], reward_dtype=dtype)
        tag = f"select/{np.dtype(dtype).name}"
        bc[f"{tag}/returns"] = np.asarray([bcref.discounted_return(ep.rewards, 0.99) for ep in ds], dtype)
        for frac in (0.45, 0.05, 0.3, 0.6, 1.0):
            ids = bcref.best_trajectories_ids(ds, frac, 0.99)
            q = bcref.qlearning_dataset(ds, ids)
            bc[f"{tag}/{frac}/ids"] = np.asarray(ids, np.int64)
            bc[f"{tag}/{frac}/obs_sum"] = np.float64(q["observations"].astype(np.float64).sum())
            bc[f"{tag}/{frac}/first_action"] = q["actions"][0]
            bc[f"{tag}/{frac}/rewards"] = q["rewards"]
            bc[f"{tag}/{frac}/terminals"] = q["terminals"]
    q = mref.qlearning_dataset(minari_env.MinariDataset(c["data_seed"]))
    iql["select/rewards"], iql["select/terminals"] = q["rewards"], q["terminals"]
    iql["select/obs_sum"] = np.float64(q["observations"].astype(np.float64).sum())
    for fname, out in (("minari_iql_run.npz", iql), ("minari_bc_run.npz", bc)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
