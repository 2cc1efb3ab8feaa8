#!/usr/bin/env python3
"""Generate tests/golden/offline_bc_select.npz and offline_bc_run.npz by RUNNING the reference's D4RL any-percent
behaviour cloning, ``algorithms/offline/any_percent_bc.py`` ("dbc"), on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_offline_bc_fixture.py [--ref /root/reference] [--measure 150]

The file is imported under inert stubs for the packages that are absent (gym, d4rl, wandb, pyrallis), as
make_minari_fixture.py imports its files, whose helpers this generator reuses.  Only arrays and short key strings
are stored.

offline_bc_select.npz: dbc's ``keep_best_trajectories`` (dbc:206-239) on the datasets of
``tests/offline_bc_env.py: CASES``, for float32 and float64 rewards and every fraction of the case: the inputs, the
five output arrays, and -- read from the function's own lists when it returns -- the first row, length and return
of every trajectory and the kept trajectory numbers.  Observations hold the row number, so the selected
observations are dbc's ``order``.  The order among equal returns is the sorting host's: every case marked
``ordered`` must have pairwise distinct returns (asserted here), and tests compare ORDER on those cases only.

offline_bc_run.npz: one run of dbc's ``train()`` as written, against stand-ins: the environment and the dataset
of tests/offline_bc_env.py (``gym.make`` / ``d4rl.qlearning_dataset``), ``wandb.log`` recording every call,
``eval_actor`` wrapped to keep the returns it hands back.  Stored: the log records, the checkpoint files written
at each step, per-tensor sums and a few whole tensors of the checkpoints, one checkpoint whole (from which
``load_model`` continues), the evaluation returns, the final ``np.random.get_state()`` -- and the same of "cont", dbc's
``train()`` run again for 15 steps with ``load_model`` = one of its own checkpoints.

Length of the run and its seed are chosen exactly as make_minari_fixture.py chooses them (its docstring has the
reasoning): 45 steps, evaluations every 15, batch 64, and the first seed from ``FIRST_SEED`` on at which the
reference ALONE -- the same run repeated with modules and sampled data cast to float64 -- stays inside the replay
bounds of tests/test_gpu_minari_bc.py (losses rtol 2e-5 / atol 2e-8, returns and scores rtol = atol = 1e-5) for
TWICE the recorded length.  Measured over 150 steps (``--measure``), as fractions of those bounds:

    seed 3   losses: first 45 steps 0.01, none beyond in 150 (largest 0.01); evaluations, all 10 of them: 0.00

so seed 3 is recorded; the gap would leave the bound at no step of the 150 measured.  The fractions of the first
90 steps and of their 6 evaluations are stored in the fixture (``run/f64_gap_of_bound``,
``run/f64_eval_gap_of_bound``), with every candidate seed tried and whether it kept the margin.

One more margin, also from the reference alone (``kink_margin``): no hidden pre-activation of a recorded step may
lie closer to zero than 4 x the rms difference between the reference's fp32 and float64 pre-activations (4.6e-8
and 5.4e-8 for the two layers).  The float64 twin cannot see a pre-activation on a relu kink when it happens to
fall on the fp32 run's side, but another fp32 summation order -- the GPU's -- can take it the other way, and Adam
turns the changed gradient into a weight change of a sizeable fraction of lr.  That is what the continuation from
``checkpoint_14.pt`` does: its float64 twin stays at 0.00 of the bounds for 30 steps, yet at its step 11 a
second-layer pre-activation lies 1.9e-8 from zero (0.09 of the margin), and on the MI355X that continuation parted
from the record right there (losses from 0.005 to 0.08 of the bound at steps 12 .. 14, ``net.0.bias`` 8.9e-6 off,
one evaluation return 1.16e-5 off against a bound of 1.03e-5) while the 45-step run itself, margin 3.17, was met
at 0.009 of the loss bound.  The continuation is therefore taken from the first checkpoint that keeps both
margins, ``checkpoint_29.pt`` (3.68), and is 15 steps long: measured over 60 steps from ``checkpoint_14.pt`` the
float64 twin reaches 0.57 (losses) and 1.86 (fourth evaluation), so 30 steps would not keep twice their length.
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_minari_fixture as mmf  # noqa: E402  (as_double, report, byte_planes, the checkpoint readers)
from tests import fake_envs, offline_bc_env as obe  # noqa: E402

FIRST_SEED = 3
KINK_SIGMAS = 4.0  # kink_margin: a pre-activation within this many rms fp32 errors of zero may change sides
CONT_STEPS = 15  # the continuation from the first checkpoint: one evaluation period (see the docstring)
COMMON = dict(max_timesteps=45, eval_freq=15, batch_size=64, n_episodes=2, data_seed=11, frac=obe.FRAC,
              max_traj_len=7)  # (max_traj_len: dbc's train() never reads it -- a cut at 7 would change every record)
RTOL, ATOL, EVAL_TOL = mmf.RTOL, mmf.ATOL, mmf.EVAL_TOL
DISCOUNT = 0.99
DTYPES = (np.float32, np.float64)


def import_reference(ref_root):
    import importlib.machinery
    import importlib.util

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    stub("gym", Env=object, wrappers=types.SimpleNamespace(TransformObservation=fake_envs.TransformObservation,
                                                           TransformReward=fake_envs.TransformReward))
    stub("d4rl")
    stub("pyrallis", wrap=lambda *a, **k: (lambda f: f))
    stub("wandb")
    spec = importlib.util.spec_from_file_location(
        "ref_offline_bc", os.path.join(ref_root, "algorithms", "offline", "any_percent_bc.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


# --------------------------------------------------------------------------- #
# the selection
# --------------------------------------------------------------------------- #
def traced_keep_best(ref, dataset, frac, discount, max_len):
    """``ref.keep_best_trajectories`` as written; returns its lists ``ids_by_trajectories`` / ``returns`` and its
    ``top_trajs`` as they stand when the function returns (or raises)."""
    code, seen = ref.keep_best_trajectories.__code__, {}

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(frame, event, arg):
            if event in ("return", "exception"):
                seen.update(frame.f_locals)
            return local
        return local

    sys.settrace(tracer)
    try:
        ref.keep_best_trajectories(dataset, frac, discount, max_len)
    finally:
        sys.settrace(None)
    return seen


def selection_arrays(ref):
    out = {"discount": np.float64(DISCOUNT), "cases": np.asarray(sorted(obe.CASES))}
    for name, (n, max_len, term_rows, fracs, ordered) in obe.CASES.items():
        for dtype in DTYPES:
            tag = f"{name}/{np.dtype(dtype).name}"
            data = obe.selection_case(name, dtype)
            out[f"{tag}/in/rewards"], out[f"{tag}/in/terminals"] = data["rewards"], data["terminals"]
            out[f"{tag}/in/actions"] = data["actions"]
            for frac in fracs:
                d = {k: v.copy() for k, v in data.items()}
                try:
                    seen = traced_keep_best(ref, d, frac, DISCOUNT, max_len)
                except IndexError:  # dbc's empty ``order``: no complete trajectory
                    assert name == "n1_open"
                    out[f"{tag}/raises"] = np.asarray("IndexError")
                    continue
                ids, returns = seen["ids_by_trajectories"], np.asarray(seen["returns"])
                assert returns.dtype == dtype, (tag, returns.dtype)
                if ordered:
                    assert len(set(returns.tolist())) == len(returns), f"{tag}: equal returns in an ordered case"
                out[f"{tag}/starts"] = np.asarray([t[0] for t in ids], np.int64)
                out[f"{tag}/lengths"] = np.asarray([len(t) for t in ids], np.int64)
                out[f"{tag}/returns"] = returns
                out[f"{tag}/{frac}/top"] = np.asarray(seen["top_trajs"], np.int64)
                for k in ("observations", "actions", "next_observations", "rewards", "terminals"):
                    out[f"{tag}/{frac}/{k}"] = d[k]
    return out


# --------------------------------------------------------------------------- #
# the run
# --------------------------------------------------------------------------- #
def run_reference(ref, seed, tmp, max_timesteps, reward_dtype=np.float32, load_model=""):
    """One run of ``ref.train``; returns (records, saves, {file name: state dict}, numpy state, evaluation returns,
    the checkpoint directory)."""
    c = COMMON
    records, saves, evals = [], [], []

    def log(d, step):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    ref.wandb = types.SimpleNamespace(init=lambda **kw: None, log=log, run=types.SimpleNamespace(save=lambda: None))
    ref.gym = types.SimpleNamespace(make=lambda name: obe.OfflineBCEnv(), Env=object, wrappers=sys.modules["gym"].wrappers)
    ref.d4rl = types.SimpleNamespace(qlearning_dataset=lambda env: obe.make_dataset(c["data_seed"], reward_dtype))
    ref.pyrallis = types.SimpleNamespace(dump=lambda cfg, f: f.write(repr(cfg)))
    real_eval, real_save = ref.eval_actor, torch.save

    def eval_actor(*a, **k):
        scores = real_eval(*a, **k)
        evals.append(np.asarray(scores, np.float64))
        return scores

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    config = ref.TrainConfig(env=obe.ENV, max_timesteps=max_timesteps, eval_freq=c["eval_freq"], batch_size=c["batch_size"],
                             n_episodes=c["n_episodes"], frac=c["frac"], max_traj_len=c["max_traj_len"], seed=seed,
                             checkpoints_path=tmp, load_model=load_model, device="cpu")
    ref.eval_actor, torch.save = eval_actor, save
    try:
        ref.train(config)
    finally:
        ref.eval_actor, torch.save = real_eval, real_save
    files = {}
    if tmp is not None:
        files = {name: torch.load(os.path.join(config.checkpoints_path, name), weights_only=True)
                 for name in sorted({s[1] for s in saves})}
    return records, saves, files, np.random.get_state(), np.asarray(evals), config.checkpoints_path


def measure_gap(ref, seed, n_steps, load_model=""):
    """|fp32 - float64| of the reference's own losses per step and of its evaluation returns and scores per
    evaluation over ``n_steps`` steps, as fractions of the replay's bounds."""
    runs = []
    for double in (False, True):
        restore = mmf.as_double(ref, "BC") if double else (lambda: None)
        try:
            rec, _, _, _, evals, _ = run_reference(ref, seed, None, n_steps, load_model=load_model)
        finally:
            restore()
        runs.append((mmf.loss_series(rec, "actor_loss"), evals.mean(1), mmf.loss_series(rec, "d4rl_normalized_score")))
    (l32, e32, s32), (l64, e64, s64) = runs
    frac = np.abs(l32 - l64) / (ATOL + RTOL * np.abs(l64))
    efrac = np.maximum(np.abs(e32 - e64) / (EVAL_TOL + EVAL_TOL * np.abs(e64)),
                       np.abs(s32 - s64) / (EVAL_TOL + EVAL_TOL * np.abs(s64)))
    return frac[:, None], efrac


def kink_margin(ref, seed, n_steps, load_model=""):
    """How far the recorded steps stay from a relu kink, from the reference alone.  At every step, with the
    reference's own fp32 weights and batch, the two hidden layers' pre-activations are computed in float64 and
    in fp32; ``rms`` = the root mean square of their difference over all entries and steps of a layer is the size of
    the error ANOTHER correct fp32 implementation makes there with its own summation order.  A pre-activation
    closer to zero than KINK_SIGMAS x rms may fall on the other side of relu' in such an implementation, which
    changes that row's gradient outright and, through Adam, weights by a sizeable fraction of lr -- the float64 twin
    does not see this when it happens to fall on the reference's side.  Returns (smallest |z| / (KINK_SIGMAS x rms)
    over both layers and all steps, the step where it lies, rms of layer 1, rms of layer 2)."""
    small, sq, count = [], [0.0, 0.0], [0, 0]
    real_train = ref.BC.train

    def train(self, batch):
        p = self.actor.state_dict()
        s = batch[0]
        z1f = torch.nn.functional.linear(s, p["net.0.weight"], p["net.0.bias"])
        z2f = torch.nn.functional.linear(torch.relu(z1f), p["net.2.weight"], p["net.2.bias"])
        d = {k: v.double() for k, v in p.items()}
        z1 = torch.nn.functional.linear(s.double(), d["net.0.weight"], d["net.0.bias"])
        z2 = torch.nn.functional.linear(torch.relu(z1), d["net.2.weight"], d["net.2.bias"])
        for i, (zf, z) in enumerate(((z1f, z1), (z2f, z2))):
            sq[i] += float(((zf.double() - z) ** 2).sum())
            count[i] += z.numel()
        small.append((float(z1.abs().min()), float(z2.abs().min())))
        return real_train(self, batch)

    ref.BC.train = train
    try:
        run_reference(ref, seed, None, n_steps, load_model=load_model)
    finally:
        ref.BC.train = real_train
    rms = [float(np.sqrt(q / c)) for q, c in zip(sq, count)]
    ratio = np.asarray(small) / (KINK_SIGMAS * np.asarray(rms))
    return float(ratio.min()), int(ratio.min(1).argmin()), rms[0], rms[1]


def choose_seed(ref, n_measure):
    """The first seed from FIRST_SEED on that keeps the margin; (seed, loss fractions, evaluation fractions, the
    candidates tried, which of them kept it)."""
    steps, every = COMMON["max_timesteps"], COMMON["eval_freq"]
    tried, ok = [], []
    for seed in range(FIRST_SEED, FIRST_SEED + 16):
        frac, efrac = measure_gap(ref, seed, n_measure)
        kink = kink_margin(ref, seed, steps)
        print(f"    dbc       seed {seed}: nearest relu kink of the {steps} steps at {kink[0]:.2f} x {KINK_SIGMAS} rms "
              f"(step {kink[1]}; rms {kink[2]:.1e}, {kink[3]:.1e})")
        tried.append(seed)
        ok.append(bool(mmf.report("dbc", seed, frac, efrac, steps, every)) and kink[0] > 1)
        if ok[-1]:
            return seed, frac[:, 0], efrac, tried, ok, kink
    raise SystemExit("no seed keeps the margin: shorten the run")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--measure", type=int, default=150, help="steps of the fp32 / float64 gap measurement")
    args = ap.parse_args()
    ref = import_reference(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    select = selection_arrays(ref)
    c = COMMON
    steps = c["max_timesteps"]
    print("measured fp32 / float64 gaps of the reference alone:")
    seed, frac, efrac, tried, ok, kink = choose_seed(ref, max(args.measure, 2 * steps))
    beyond = np.nonzero(frac >= 1)[0]
    run = {f"common/{k}": np.asarray(v) for k, v in c.items()}
    run["common/first_seed"] = np.int64(FIRST_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        records, saves, files, state, evals, ckdir = run_reference(ref, seed, tmp, steps)
        # the continuation: dbc's train() again with load_model = one of its own checkpoints, for CONT_STEPS steps (it
        # seeds numpy afresh, so its indices are those of steps 0 .. and its records go on from the file's total_it).
        # The file: the first of the run's checkpoints from which the continuation keeps both margins.
        names = [s_[1] for s_ in sorted(saves)]
        cont_tried, cont_ok = [], []
        for first in names:
            model = os.path.join(ckdir, first)
            cfrac, cefrac = measure_gap(ref, seed, 2 * CONT_STEPS, load_model=model)
            ckink = kink_margin(ref, seed, CONT_STEPS, load_model=model)
            print(f"    dbc/cont  from {first}: nearest relu kink at {ckink[0]:.2f} x {KINK_SIGMAS} rms (step {ckink[1]})")
            cont_tried.append(first)
            cont_ok.append(bool(mmf.report("dbc/cont", seed, cfrac, cefrac, CONT_STEPS, c["eval_freq"])) and ckink[0] > 1)
            if cont_ok[-1]:
                break
        else:
            raise SystemExit("no continuation keeps the margins")
        with tempfile.TemporaryDirectory() as tmp2:
            crec, csaves, cfiles, cstate, cevals, _ = run_reference(ref, seed, tmp2, CONT_STEPS, load_model=model)
    run["cont/candidates"], run["cont/candidate_ok"] = np.asarray(cont_tried), np.asarray(cont_ok)
    run["run/kink_margin"], run["cont/kink_margin"] = np.float64(kink[0]), np.float64(ckink[0])
    run["common/kink_sigmas"] = np.float64(KINK_SIGMAS)
    run.update(mmf.common_arrays("cont", seed, None, crec, csaves, cstate))
    run["cont/eval_returns"], run["cont/steps"] = cevals, np.int64(CONT_STEPS)
    run["cont/f64_gap_of_bound"], run["cont/f64_eval_gap_of_bound"] = cfrac[:, 0], cefrac
    clast = max(csaves, key=lambda s: s[0])[1]
    run.update(mmf.bc_checkpoint_arrays(f"cont/{clast}", {k: v for k, v in cfiles[clast].items() if k != "total_it"}, True))
    run[f"cont/{clast}/total_it"] = np.int64(cfiles[clast]["total_it"])
    run[f"cont/{clast}/keys"] = np.asarray(sorted(cfiles[clast]))
    run.update(mmf.common_arrays("run", seed, None, records, saves, state))
    run["run/eval_returns"] = evals
    run["run/candidates"], run["run/candidate_ok"] = np.asarray(tried, np.int64), np.asarray(ok)
    run["run/f64_gap_of_bound"], run["run/f64_eval_gap_of_bound"] = frac[:2 * steps], efrac[:2 * steps // c["eval_freq"]]
    run["run/f64_measured_steps"] = np.int64(len(frac))
    run["run/f64_first_step_beyond"] = np.int64(beyond[0] if beyond.size else -1)
    last = max(saves, key=lambda s: s[0])[1]
    for fname, sd in files.items():  # (the whole tensors of the last checkpoint only)
        run.update(mmf.bc_checkpoint_arrays(f"run/{fname}", {k: v for k, v in sd.items() if k != "total_it"}, fname == last))
        run[f"run/{fname}/keys"] = np.asarray(sorted(sd))
        run[f"run/{fname}/total_it"] = np.int64(sd["total_it"])
    run["run/whole"] = np.asarray(first)
    run.update(mmf.bc_whole_state(f"run/whole/{first}", files[first]))
    # the rows the run trained on: dbc's selection of the training dataset
    d = obe.make_dataset(c["data_seed"])
    seen = traced_keep_best(ref, d, c["frac"], DISCOUNT, 1000)
    run["select/top"] = np.asarray(seen["top_trajs"], np.int64)
    run["select/returns"] = np.asarray(seen["returns"])
    assert len(set(run["select/returns"].tolist())) == len(run["select/returns"])
    run["select/rewards"], run["select/obs_sum"] = d["rewards"], np.float64(d["observations"].astype(np.float64).sum())
    for fname, out in (("offline_bc_select.npz", select), ("offline_bc_run.npz", run)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
