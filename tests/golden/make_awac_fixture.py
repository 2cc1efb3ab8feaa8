#!/usr/bin/env python3
"""Generate tests/golden/awac_step.npz and awac_run.npz by RUNNING the reference's offline AWAC,
``algorithms/offline/awac.py`` ("awac"), on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_awac_fixture.py [--ref /root/reference] [--measure 120]

The file is imported under inert stubs for the packages that are absent (gym, d4rl, wandb, pyrallis, tqdm), as
make_offline_bc_fixture.py imports its file.  Only arrays and short key strings are stored.

The normal draw.  ``Normal.rsample`` takes its standard normals from ``torch.distributions.normal._standard_normal``;
the generator wraps that function: in a recording run it hands on what torch drew and keeps a copy, in a replaying
run (the float64 twin, the step cases) it hands back given numbers in the dtype asked for.  An update draws twice,
eps_1 for ``a'`` (awac:269) and eps_2 for ``pi`` (awac:250), each [B, A]; evaluations draw nothing (``actor.eval()``
acts on the mean).

awac_step.npz: the reference's own ``update`` for STEPS steps on two cases of tests/awac_cases.py (the one-row case
and the lambda 0.1 case) from the case's parameters, targets, rows and eps: per step both losses, every gradient,
the new parameters, both Adam moments and the new targets (the lambda case: whole tensors at its last step, whose
values the earlier steps decide, and float64 sums per tensor before it).  And ``modify_reward`` / ``return_reward_range`` on the
stand-in dataset under a locomotion, an antmaze and another name.

awac_run.npz: one run of awac's ``train()`` as written, against stand-ins: the environment and the dataset of
tests/offline_bc_env.py (``gym.make`` / ``d4rl.qlearning_dataset``), ``wandb.log`` recording every call.  hidden_dim
32, batch 64, 45 steps, evaluations every 15.  Stored: the log records, eps per step, the evaluation returns, the
checkpoint files written at each step with per-tensor sums, one checkpoint whole.

Length and seed are chosen as make_offline_bc_fixture.py chooses them: the first seed from ``FIRST_SEED`` on at which
the reference ALONE -- the same run repeated with modules and sampled data cast to float64, on the fp32 run's eps
-- stays inside the replay bounds of tests/test_gpu_minari_bc.py (losses rtol 2e-5 / atol 2e-8, returns and scores
rtol = atol = 1e-5) for TWICE the recorded length, and keeps the kink margin: no hidden pre-activation of a
differentiated network (both critics at (s, a), the actor at s) of a recorded step closer to zero than
``KINK_SIGMAS`` x the rms difference between the reference's fp32 and float64 pre-activations.  The measured
fractions are stored in the fixture (``run/f64_gap_of_bound``, ``run/f64_eval_gap_of_bound``, ``run/kink_margin``);
the generator prints them, and the figures of the recorded seed are quoted in tests/test_gpu_awac.py.
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
import make_minari_fixture as mmf  # noqa: E402  (as_double, report, byte_planes, loss_series)
from tests import awac_cases as ac, fake_envs, offline_bc_env as obe  # noqa: E402

FIRST_SEED = 3
KINK_SIGMAS = 4.0
COMMON = dict(num_train_ops=45, eval_frequency=15, batch_size=64, hidden_dim=32, n_test_episodes=2, test_seed=5,
              data_seed=11)
RTOL, ATOL, EVAL_TOL = mmf.RTOL, mmf.ATOL, mmf.EVAL_TOL
STEP_CASES = ("s3_a1_b1_h16", ac.LAMBDA_CASE)
LOSSES = ("critic_loss", "actor_loss")


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
    stub("tqdm", trange=lambda n, **k: range(n))
    spec = importlib.util.spec_from_file_location("ref_awac", os.path.join(ref_root, "algorithms", "offline", "awac.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    mod.trainer_class = mod.AdvantageWeightedActorCritic  # (mmf.as_double swaps the module's name for a factory)
    return mod


class Noise:
    """The wrapped ``_standard_normal``: records what torch draws, or replays ``given`` (a list of arrays)."""

    def __init__(self):
        import torch.distributions.normal as tdn
        self._mod, self._real = tdn, tdn._standard_normal
        self.drawn, self.given = [], None
        tdn._standard_normal = self

    def __call__(self, shape, dtype, device):
        if self.given is not None:
            e = torch.as_tensor(np.asarray(self.given.pop(0))).reshape(tuple(shape)).to(dtype=dtype, device=device)
        else:
            e = self._real(shape, dtype, device)
        self.drawn.append(e.detach().to(torch.float32).numpy().copy())
        return e

    def start(self, given=None):
        self.drawn, self.given = [], None if given is None else list(given)

    def close(self):
        self._mod._standard_normal = self._real


# --------------------------------------------------------------------------- #
# the step cases
# --------------------------------------------------------------------------- #
def step_arrays(ref, noise):
    out = {"cases": np.asarray(STEP_CASES)}
    for case in STEP_CASES:
        S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
        mods = {"actor": ref.Actor(S, A, H), "critic_1": ref.Critic(S, A, H), "critic_2": ref.Critic(S, A, H)}
        for n, m in mods.items():
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        opts = {n: torch.optim.Adam(m.parameters(), lr=ac.LR) for n, m in mods.items()}
        tr = ref.AdvantageWeightedActorCritic(
            actor=mods["actor"], actor_optimizer=opts["actor"], critic_1=mods["critic_1"],
            critic_1_optimizer=opts["critic_1"], critic_2=mods["critic_2"], critic_2_optimizer=opts["critic_2"],
            gamma=ac.GAMMA, tau=ac.TAU, awac_lambda=lam)
        mods["target_critic_1"], mods["target_critic_2"] = tr._target_critic_1, tr._target_critic_2
        for n in ac.TARGETS:
            mods[n].load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        for t in range(ac.STEPS):
            s, a, r, s2, d = ac.batch_of(data, idx[t, :B])
            batch = [torch.from_numpy(np.ascontiguousarray(x)) for x in (s, a, r[:, None], s2, d[:, None])]
            noise.start([eps[t, 0], eps[t, 1]])
            res = tr.update(batch)
            assert not noise.given and len(noise.drawn) == 2
            pre = f"{case}/{t}"
            for k in LOSSES:
                out[f"{pre}/{k}"] = np.float64(res[k])
            whole = t == ac.STEPS - 1 or case == STEP_CASES[0]  # (the steps are chained: the last one holds them all)

            def put(key, x, big=False):
                if whole and not (big and case != STEP_CASES[0]):
                    out[key] = x.detach().numpy().copy()
                out[key + "/sum"] = np.float64(x.detach().double().sum().item())

            for n, m in mods.items():
                for k, p in m.named_parameters():
                    put(f"{pre}/param/{n}.{k}", p)
                    if n in opts:
                        st = opts[n].state[p]
                        put(f"{pre}/grad/{n}.{k}", p.grad)
                        put(f"{pre}/exp_avg/{n}.{k}", st["exp_avg"])
                        put(f"{pre}/exp_avg_sq/{n}.{k}", st["exp_avg_sq"], big=True)  # (sums only: the file stays under 1 MiB)
    # modify_reward / return_reward_range (awac:380-401) on the stand-in dataset
    for name in ("halfcheetah-medium-v2", "antmaze-medium-diverse-v2", "pen-human-v1"):
        d = obe.make_dataset(COMMON["data_seed"])
        if "antmaze" not in name and "pen" not in name:
            lo, hi = ref.return_reward_range(d, 1000)
            out[f"reward/{name}/range"] = np.asarray([lo, hi], np.float64)
            lo, hi = ref.return_reward_range(d, 40)
            out[f"reward/{name}/range40"] = np.asarray([lo, hi], np.float64)
        ref.modify_reward(d, name)
        out[f"reward/{name}/rewards"] = d["rewards"]
    return out


# --------------------------------------------------------------------------- #
# the run
# --------------------------------------------------------------------------- #
def run_reference(ref, noise, seed, tmp, n_steps, given=None, probe=None):
    """One run of ``ref.train``; returns (records, saves, {file name: state dict}, eps [n_steps, 2, B, A], evaluation
    returns).  ``probe(trainer, batch)``: called before every update."""
    c = COMMON
    records, saves, evals = [], [], []

    def log(d, step):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    ref.wandb = types.SimpleNamespace(init=lambda **kw: None, log=log, finish=lambda: None,
                                      run=types.SimpleNamespace(save=lambda: None))
    ref.gym = types.SimpleNamespace(make=lambda name: obe.OfflineBCEnv(), Env=object, wrappers=sys.modules["gym"].wrappers)
    ref.d4rl = types.SimpleNamespace(qlearning_dataset=lambda env: obe.make_dataset(c["data_seed"]))
    ref.pyrallis = types.SimpleNamespace(dump=lambda cfg, f: f.write(repr(cfg)))
    real_eval, real_save, real_update = ref.eval_actor, torch.save, ref.trainer_class.update

    def eval_actor(*a, **k):
        scores = real_eval(*a, **k)
        evals.append(np.asarray(scores, np.float64))
        return scores

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    def update(self, batch):
        if probe is not None:
            probe(self, batch)
        return real_update(self, batch)

    config = ref.TrainConfig(env_name=obe.ENV, num_train_ops=n_steps, eval_frequency=c["eval_frequency"],
                             batch_size=c["batch_size"], hidden_dim=c["hidden_dim"], n_test_episodes=c["n_test_episodes"],
                             test_seed=c["test_seed"], seed=seed, checkpoints_path=tmp, device="cpu")
    ref.eval_actor, torch.save, ref.trainer_class.update = eval_actor, save, update
    noise.start(given)
    try:
        ref.train(config)
    finally:
        ref.eval_actor, torch.save, ref.trainer_class.update = real_eval, real_save, real_update
    eps = np.stack(noise.drawn).reshape(n_steps, 2, c["batch_size"], -1)
    files = {}
    if tmp is not None:
        files = {name: torch.load(os.path.join(config.checkpoints_path, name), weights_only=True)
                 for name in sorted({s[1] for s in saves})}
    return records, saves, files, eps, np.asarray(evals)


def measure_gap(ref, noise, seed, n_steps):
    """|fp32 - float64| of the reference's own losses per step and of its evaluation returns and scores per
    evaluation over ``n_steps`` steps, as fractions of the replay's bounds; the twin replays the fp32 run's eps."""
    rec32, _, _, eps, ev32 = run_reference(ref, noise, seed, None, n_steps)
    restore = mmf.as_double(ref, "AdvantageWeightedActorCritic")
    try:
        rec64, _, _, _, ev64 = run_reference(ref, noise, seed, None, n_steps, given=list(eps.reshape(-1, *eps.shape[2:])))
    finally:
        restore()
    l32, l64 = (np.stack([mmf.loss_series(r, k) for k in LOSSES], 1) for r in (rec32, rec64))
    s32, s64 = (mmf.loss_series(r, "d4rl_normalized_score") for r in (rec32, rec64))
    e32, e64 = ev32.mean(1), ev64.mean(1)
    frac = np.abs(l32 - l64) / (ATOL + RTOL * np.abs(l64))
    efrac = np.maximum(np.abs(e32 - e64) / (EVAL_TOL + EVAL_TOL * np.abs(e64)),
                       np.abs(s32 - s64) / (EVAL_TOL + EVAL_TOL * np.abs(s64)))
    return frac, efrac


def kink_margin(ref, noise, seed, n_steps):
    """How far the recorded steps stay from a relu kink of a differentiated network, from the reference alone
    (make_offline_bc_fixture.kink_margin has the reasoning).  Returns (smallest |z| / (KINK_SIGMAS x rms), its step)."""
    small, sq, count = [], 0.0, 0

    def hidden(mlp, x, dtype):
        sd = {k: v.to(dtype) for k, v in mlp.state_dict().items()}
        zs, h = [], x.to(dtype)
        for i in (0, 2, 4):
            z = torch.nn.functional.linear(h, sd[f"{i}.weight"], sd[f"{i}.bias"])
            zs.append(z)
            h = torch.relu(z)
        return zs

    def probe(self, batch):
        nonlocal sq, count
        s, a = batch[0], batch[1]
        lo = np.inf
        for mlp, x in ((self._critic_1._mlp, torch.cat([s, a], -1)), (self._critic_2._mlp, torch.cat([s, a], -1)),
                       (self._actor._mlp, s)):
            with torch.no_grad():
                for zf, z in zip(hidden(mlp, x, torch.float32), hidden(mlp, x, torch.float64)):
                    sq += float(((zf.double() - z) ** 2).sum())
                    count += z.numel()
                    lo = min(lo, float(z.abs().min()))
        small.append(lo)

    run_reference(ref, noise, seed, None, n_steps, probe=probe)
    ratio = np.asarray(small) / (KINK_SIGMAS * np.sqrt(sq / count))
    return float(ratio.min()), int(ratio.argmin()), float(np.sqrt(sq / count))


def choose_seed(ref, noise, n_measure):
    steps, every = COMMON["num_train_ops"], COMMON["eval_frequency"]
    tried, ok = [], []
    for seed in range(FIRST_SEED, FIRST_SEED + 16):
        frac, efrac = measure_gap(ref, noise, seed, n_measure)
        kink = kink_margin(ref, noise, seed, steps)
        print(f"    awac      seed {seed}: nearest relu kink of the {steps} steps at {kink[0]:.2f} x {KINK_SIGMAS} rms "
              f"(step {kink[1]}; rms {kink[2]:.1e})")
        tried.append(seed)
        ok.append(bool(mmf.report("awac", seed, frac, efrac, steps, every)) and kink[0] > 1)
        if ok[-1]:
            return seed, frac, efrac, tried, ok, kink
    raise SystemExit("no seed keeps the margin: shorten the run")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--measure", type=int, default=120, help="steps of the fp32 / float64 gap measurement")
    args = ap.parse_args()
    ref = import_reference(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    noise = Noise()
    try:
        step = step_arrays(ref, noise)
        c = COMMON
        steps = c["num_train_ops"]
        print("measured fp32 / float64 gaps of the reference alone:")
        seed, frac, efrac, tried, ok, kink = choose_seed(ref, noise, max(args.measure, 2 * steps))
        with tempfile.TemporaryDirectory() as tmp:
            records, saves, files, eps, evals = run_reference(ref, noise, seed, tmp, steps)
    finally:
        noise.close()
    run = {f"common/{k}": np.asarray(v) for k, v in c.items()}
    run["common/first_seed"], run["common/kink_sigmas"] = np.int64(FIRST_SEED), np.float64(KINK_SIGMAS)
    run["run/seed"] = np.int64(seed)
    run["run/rec_step"] = np.asarray([r[0] for r in records], np.int64)
    run["run/rec_key"] = np.asarray([r[1] for r in records])
    run["run/rec_value"] = np.asarray([r[2] for r in records], np.float64)
    run["run/save_step"] = np.asarray([s[0] for s in saves], np.int64)
    run["run/save_name"] = np.asarray([s[1] for s in saves])
    run["run/eps"], run["run/eval_returns"] = eps, evals
    run["run/candidates"], run["run/candidate_ok"] = np.asarray(tried, np.int64), np.asarray(ok)
    run["run/f64_gap_of_bound"], run["run/f64_eval_gap_of_bound"] = frac[:2 * steps], efrac[:2 * steps // c["eval_frequency"]]
    run["run/f64_measured_steps"] = np.int64(len(frac))
    run["run/kink_margin"], run["run/kink_step"] = np.float64(kink[0]), np.int64(kink[1])
    last = max(saves, key=lambda s: s[0])[1]
    for fname, sd in files.items():
        run[f"run/{fname}/keys"] = np.asarray(sorted(sd))
        for net, tensors in sd.items():
            run[f"run/{fname}/{net}/names"] = np.asarray(list(tensors))
            for k, v in tensors.items():
                run[f"run/{fname}/{net}/{k}/sum"] = np.float64(v.double().sum().item())
                if fname == last:  # the last checkpoint whole
                    run[f"run/{fname}/{net}/{k}"] = v.numpy()
    run["run/whole"] = np.asarray(last)
    for fname, out in (("awac_step.npz", step), ("awac_run.npz", run)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
