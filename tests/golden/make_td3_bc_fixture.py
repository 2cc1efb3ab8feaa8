#!/usr/bin/env python3
"""Generate tests/golden/td3_bc_step.npz and td3_bc_run.npz by RUNNING the reference's offline TD3+BC,
``algorithms/offline/td3_bc.py`` ("tdbc"), on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_td3_bc_fixture.py [--ref /root/reference] [--measure 60]

The file is imported under inert stubs for the packages that are absent (gym, d4rl, wandb, pyrallis), as
make_awac_fixture.py imports its file.  Only arrays and short key strings are stored.

The normal draw.  tdbc:333 calls ``torch.randn_like(action)``; inside the imported module ``torch`` is replaced by a
proxy whose ``randn_like`` records what torch drew, or (the float64 twin, the step cases) hands back given numbers in
the dtype of its argument.  A ``train`` call draws once, [B, A]; evaluations draw nothing.

td3_bc_step.npz: the reference's own ``train`` on two cases of tests/td3_bc_cases.py (the one-row case and the
policy_freq 3 case) from the case's parameters, targets, rows and eps: per step the losses, every gradient, the new
parameters, both Adam moments and the new targets (the larger case: whole tensors at its last step, whose values the
earlier steps decide, and float64 sums per tensor before it; the gradients of a network are those of the last
backward that reached it).  tdbc's networks are 256 wide as written: the cases' widths are set by replacing ``net``
of the reference's own ``Actor`` / ``Critic`` objects, whose ``forward`` stays the reference's.

td3_bc_run.npz: one run of tdbc's ``train()`` as written, against stand-ins: the environment and the dataset of
tests/offline_bc_env.py (``gym.make`` / ``d4rl.qlearning_dataset``), ``wandb.log`` recording every call.  256-wide
networks (hard-coded there), batch 64, 30 steps, evaluations every 10.  Stored: the log records, eps per step, the
evaluation returns, the checkpoint files written with per-tensor float64 sums (optimiser state included), the actor
of the last checkpoint whole.

Length and seed are chosen as make_awac_fixture.py chooses them: the first seed from ``FIRST_SEED`` on at which the
reference ALONE -- the same run repeated with modules and sampled data cast to float64, on the fp32 run's eps -- stays
inside the replay bounds (losses rtol 2e-5 / atol 2e-8, returns and scores rtol = atol = 1e-5) for TWICE the recorded
length, and keeps the kink margin: no hidden pre-activation of a differentiated network (both critics at (s, a), the
actor at s, critic 1 at (s, pi)) of a recorded step closer to zero than ``KINK_SIGMAS`` x the rms difference between
the reference's fp32 and float64 pre-activations.  The measured fractions are stored in the fixture and quoted in
tests/test_gpu_td3_bc.py.
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
import make_minari_fixture as mmf  # noqa: E402  (as_double, loss_series)
from tests import fake_envs, offline_bc_env as obe, td3_bc_cases as tc  # noqa: E402

FIRST_SEED = 0
KINK_SIGMAS = 4.0
COMMON = dict(max_timesteps=30, eval_freq=10, batch_size=64, n_episodes=2, data_seed=11)
RTOL, ATOL, EVAL_TOL = mmf.RTOL, mmf.ATOL, mmf.EVAL_TOL
STEP_CASES = ("s3_a1_b1_h16", "s45_a24_b64_h64_pf3")
NETS = ("critic_1", "critic_2", "actor")


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
    spec = importlib.util.spec_from_file_location("ref_td3_bc", os.path.join(ref_root, "algorithms", "offline", "td3_bc.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


class Noise:
    """The module's ``torch`` with ``randn_like`` wrapped: records what torch draws, or replays ``given``."""

    def __init__(self):
        self.drawn, self.given, self._ref, self._base = [], None, None, None

    def __getattr__(self, name):
        return getattr(self._base, name)

    def randn_like(self, x, **kw):
        if self.given is not None:
            e = torch.as_tensor(np.asarray(self.given.pop(0))).reshape(x.shape).to(dtype=x.dtype, device=x.device)
        else:
            e = torch.randn_like(x, **kw)
        self.drawn.append(e.detach().to(torch.float32).numpy().copy())
        return e

    def install(self, ref, given=None):
        """Over whatever ``ref.torch`` is now (torch, or mmf.as_double's float64 proxy)."""
        self.drawn, self.given = [], None if given is None else list(given)
        self._ref, self._base = ref, ref.torch
        ref.torch = self

    def remove(self):
        self._ref.torch = self._base


def resized(module, in_dim, hidden, out_dim, tanh):
    """The reference's own Actor / Critic object with ``net`` at another width (its forward stays tdbc's)."""
    layers = [torch.nn.Linear(in_dim, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden), torch.nn.ReLU(),
              torch.nn.Linear(hidden, out_dim)] + ([torch.nn.Tanh()] if tanh else [])
    module.net = torch.nn.Sequential(*layers)
    return module


# --------------------------------------------------------------------------- #
# the step cases
# --------------------------------------------------------------------------- #
def step_arrays(ref, noise):
    out = {"cases": np.asarray(STEP_CASES)}
    for case in STEP_CASES:
        S, A, B, H, params, data, idx, eps, _ = tc.case_inputs(case)
        hp = tc.hyper(case)
        mods = {"actor": resized(ref.Actor(S, A, hp["max_action"]), S, H, A, True),
                "critic_1": resized(ref.Critic(S, A), S + A, H, 1, False), "critic_2": resized(ref.Critic(S, A), S + A, H, 1, False)}
        for n, m in mods.items():
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        opts = {n: torch.optim.Adam(m.parameters(), lr=tc.LR) for n, m in mods.items()}
        tr = ref.TD3_BC(max_action=hp["max_action"], actor=mods["actor"], actor_optimizer=opts["actor"],
                        critic_1=mods["critic_1"], critic_1_optimizer=opts["critic_1"], critic_2=mods["critic_2"],
                        critic_2_optimizer=opts["critic_2"], discount=hp["discount"], tau=hp["tau"],
                        policy_noise=hp["policy_noise"], noise_clip=hp["noise_clip"], policy_freq=hp["policy_freq"],
                        alpha=hp["alpha"])
        mods["actor_target"], mods["critic_1_target"], mods["critic_2_target"] = tr.actor_target, tr.critic_1_target, tr.critic_2_target
        for n in tc.TARGETS:
            mods[n].load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        steps = tc.n_steps(case)
        for t in range(steps):
            s, a, r, s2, d = tc.batch_of(data, idx[t, :B])
            batch = [torch.from_numpy(np.ascontiguousarray(x)) for x in (s, a, r[:, None], s2, d[:, None])]
            noise.install(ref, [eps[t]])
            try:
                res = tr.train(batch)
            finally:
                noise.remove()
            assert not noise.given and len(noise.drawn) == 1
            pre = f"{case}/{t}"
            out[f"{pre}/keys"] = np.asarray(list(res))
            for k, v in res.items():
                out[f"{pre}/{k}"] = np.float64(v)
            whole = t == steps - 1 or case == STEP_CASES[0]  # (the steps are chained: the last one holds them all)

            def put(key, x, big=False):
                if whole and not (big and case != STEP_CASES[0]):
                    out[key] = x.detach().numpy().copy()
                out[key + "/sum"] = np.float64(x.detach().double().sum().item())

            for n, m in mods.items():
                for k, p in m.named_parameters():
                    put(f"{pre}/param/{n}.{k}", p)
                    if n in opts and p in opts[n].state:
                        st = opts[n].state[p]
                        # (a critic's .grad after an actor step is the actor loss's: tdbc never applies it)
                        if not (n == "critic_1" and "actor_loss" in res):
                            put(f"{pre}/grad/{n}.{k}", p.grad)
                        put(f"{pre}/exp_avg/{n}.{k}", st["exp_avg"])
                        put(f"{pre}/exp_avg_sq/{n}.{k}", st["exp_avg_sq"], big=True)  # (sums only: the file stays small)
                        out[f"{pre}/step/{n}.{k}"] = np.float64(float(st["step"]))
    return out


# --------------------------------------------------------------------------- #
# the run
# --------------------------------------------------------------------------- #
def run_reference(ref, noise, seed, tmp, n_steps, given=None, probe=None):
    """One run of ``ref.train``; returns (records, saves, {file name: state dict}, eps [n_steps, B, A], evaluation
    returns).  ``probe(trainer, batch)``: called before every ``train`` call of the trainer."""
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
    trainer_class = ref.TD3_BC if isinstance(ref.TD3_BC, type) else ref.TD3_BC.cls
    real_eval, real_save, real_train = ref.eval_actor, torch.save, trainer_class.train

    def eval_actor(*a, **k):
        scores = real_eval(*a, **k)
        evals.append(np.asarray(scores, np.float64))
        return scores

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    def train(self, batch):
        if probe is not None:
            probe(self, batch)
        return real_train(self, batch)

    config = ref.TrainConfig(env=obe.ENV, max_timesteps=n_steps, eval_freq=c["eval_freq"], batch_size=c["batch_size"],
                             n_episodes=c["n_episodes"], seed=seed, checkpoints_path=tmp, device="cpu")
    ref.eval_actor, torch.save, trainer_class.train = eval_actor, save, train
    noise.install(ref, given)
    try:
        ref.train(config)
    finally:
        noise.remove()
        ref.eval_actor, torch.save, trainer_class.train = real_eval, real_save, real_train
    eps = np.stack(noise.drawn).reshape(n_steps, c["batch_size"], -1)
    files = {}
    if tmp is not None:
        files = {name: torch.load(os.path.join(config.checkpoints_path, name), weights_only=True)
                 for name in sorted({s[1] for s in saves})}
    return records, saves, files, eps, np.asarray(evals)


def as_double(ref):
    """mmf.as_double for tdbc's trainer; the factory remembers the class for run_reference's wrapping of ``train``."""
    cls = ref.TD3_BC
    restore = mmf.as_double(ref, "TD3_BC")
    ref.TD3_BC.cls = cls
    return restore


def measure_gap(ref, noise, seed, n_steps):
    """|fp32 - float64| of the reference's own losses per record and of its evaluation returns and scores per
    evaluation over ``n_steps`` steps, as fractions of the replay's bounds; the twin replays the fp32 run's eps.
    Returns (critic_loss fractions [n_steps], actor_loss fractions [actor steps], evaluation fractions)."""
    rec32, _, _, eps, ev32 = run_reference(ref, noise, seed, None, n_steps)
    restore = as_double(ref)
    try:
        rec64, _, _, _, ev64 = run_reference(ref, noise, seed, None, n_steps, given=list(eps))
    finally:
        restore()
    fr = []
    for k in ("critic_loss", "actor_loss"):
        l32, l64 = mmf.loss_series(rec32, k), mmf.loss_series(rec64, k)
        fr.append(np.abs(l32 - l64) / (ATOL + RTOL * np.abs(l64)))
    s32, s64 = (mmf.loss_series(r, "d4rl_normalized_score") for r in (rec32, rec64))
    e32, e64 = ev32.mean(1), ev64.mean(1)
    efrac = np.maximum(np.abs(e32 - e64) / (EVAL_TOL + EVAL_TOL * np.abs(e64)),
                       np.abs(s32 - s64) / (EVAL_TOL + EVAL_TOL * np.abs(s64)))
    return fr[0], fr[1], efrac


def kink_margin(ref, noise, seed, n_steps):
    """How far the recorded steps stay from a relu kink of a differentiated network, from the reference alone, at the
    parameters before each step.  Returns (smallest |z| / (KINK_SIGMAS x rms), its step, the rms)."""
    small, sq, count = [], 0.0, 0

    def hidden(net, x, dtype):
        sd = {k: v.to(dtype) for k, v in net.state_dict().items()}
        zs, h = [], x.to(dtype)
        for i in (0, 2):
            z = torch.nn.functional.linear(h, sd[f"{i}.weight"], sd[f"{i}.bias"])
            zs.append(z)
            h = torch.relu(z)
        return zs

    def probe(self, batch):
        nonlocal sq, count
        s, a = batch[0], batch[1]
        lo = np.inf
        with torch.no_grad():
            pi = self.actor(s)
            for net, x in ((self.critic_1.net, torch.cat([s, a], 1)), (self.critic_2.net, torch.cat([s, a], 1)),
                           (self.actor.net, s), (self.critic_1.net, torch.cat([s, pi], 1))):
                for zf, z in zip(hidden(net, x, torch.float32), hidden(net, x, torch.float64)):
                    sq += float(((zf.double() - z) ** 2).sum())
                    count += z.numel()
                    lo = min(lo, float(z.abs().min()))
        small.append(lo)

    run_reference(ref, noise, seed, None, n_steps, probe=probe)
    ratio = np.asarray(small) / (KINK_SIGMAS * np.sqrt(sq / count))
    return float(ratio.min()), int(ratio.argmin()), float(np.sqrt(sq / count))


def choose_seed(ref, noise, n_measure):
    steps, every = COMMON["max_timesteps"], COMMON["eval_freq"]
    tried, ok = [], []
    for seed in range(FIRST_SEED, FIRST_SEED + 16):
        cfrac, afrac, efrac = measure_gap(ref, noise, seed, n_measure)
        kink = kink_margin(ref, noise, seed, steps)
        n2 = 2 * steps
        good = cfrac[:n2].max() < 1 and afrac[:n2 // 2].max() < 1 and efrac[:n2 // every].max() < 1 and kink[0] > 1
        print(f"    td3_bc    seed {seed}: critic_loss {cfrac[:n2].max():.2f}, actor_loss {afrac[:n2 // 2].max():.2f} of the bound "
              f"over {n2} steps; evaluations " + ", ".join(f"{f:.2f}" for f in efrac[:n2 // every])
              + f"; nearest relu kink of the {steps} steps at {kink[0]:.2f} x {KINK_SIGMAS} rms (step {kink[1]}; rms {kink[2]:.1e})")
        tried.append(seed)
        ok.append(bool(good))
        if good:
            return seed, cfrac, afrac, efrac, tried, ok, kink
    raise SystemExit("no seed keeps the margin: shorten the run")


def sums_of(prefix, sd, out, whole_net=None):
    out[f"{prefix}/keys"] = np.asarray(list(sd))
    out[f"{prefix}/total_it"] = np.int64(sd["total_it"])
    for net in NETS:
        out[f"{prefix}/{net}/names"] = np.asarray(list(sd[net]))
        for k, v in sd[net].items():
            out[f"{prefix}/{net}/{k}/sum"] = np.float64(v.double().sum().item())
            if net == whole_net:
                out[f"{prefix}/{net}/{k}"] = v.numpy()
        opt = sd[net + "_optimizer"]
        for i, st in opt["state"].items():
            out[f"{prefix}/{net}_optimizer/{i}/step"] = np.float64(float(st["step"]))
            for k in ("exp_avg", "exp_avg_sq"):
                out[f"{prefix}/{net}_optimizer/{i}/{k}/sum"] = np.float64(st[k].double().sum().item())
        out[f"{prefix}/{net}_optimizer/lr"] = np.float64(opt["param_groups"][0]["lr"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--measure", type=int, default=60, help="steps of the fp32 / float64 gap measurement")
    args = ap.parse_args()
    ref = import_reference(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    noise = Noise()
    step = step_arrays(ref, noise)
    c = COMMON
    steps = c["max_timesteps"]
    print("measured fp32 / float64 gaps of the reference alone:")
    seed, cfrac, afrac, efrac, tried, ok, kink = choose_seed(ref, noise, max(args.measure, 2 * steps))
    with tempfile.TemporaryDirectory() as tmp:
        records, saves, files, eps, evals = run_reference(ref, noise, seed, tmp, steps)
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
    run["run/f64_critic_gap_of_bound"], run["run/f64_actor_gap_of_bound"] = cfrac[:2 * steps], afrac[:steps]
    run["run/f64_eval_gap_of_bound"] = efrac[:2 * steps // c["eval_freq"]]
    run["run/kink_margin"], run["run/kink_step"] = np.float64(kink[0]), np.int64(kink[1])
    last = max(saves, key=lambda s: s[0])[1]
    for fname, sd in files.items():
        sums_of(f"run/{fname}", sd, run, whole_net="actor" if fname == last else None)
    run["run/whole"] = np.asarray(last)
    for fname, out in (("td3_bc_step.npz", step), ("td3_bc_run.npz", run)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
