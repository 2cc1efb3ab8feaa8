"""What the envelope tests of the two training steps share (tests/test_gpu_general_step_envelope.py: the general
layer-wise step of csrc/iql_deep.hip; tests/test_gpu_tuned_step_envelope.py: the tuned three-kernel step of
csrc/iql_step.hip): two judged steps of one case at the GPU's own parameters.  A step is one train_steps(buf, 1, B,
indices=...) on a trainer with keep_grads; the reference of step t is evaluated at what the GPU held BEFORE step t
(helpers.gs_reference_step), so every check is a single-step comparison: losses, gradients, then Adam / Polyak from
the device's own numbers, then, after the last step, forwards on the copies the update refreshed.  The bounds are
helpers.GS_*; the calling file's docstring says what each of them is."""
import os

import numpy as np
import torch

from oracle import iql_oracle as orc
from tests import helpers

N_FWD = 20
GROUPS = ("q", "v", "actor")


def new_tally():
    """Step-2 (case, mode, net) checks of the counted cases, and those that took the loose bound."""
    return {"checks": 0, "uses": []}


def say(tag, line):
    print(f"IQLTEST {tag} " + line)
    path = os.environ.get("IQL_TEST_DIAG")
    if path:
        with open(path, "a") as f:
            f.write(f"{tag} " + line + "\n")


def _mods(tr):
    return (("q", tr.qf, tr.q_optimizer), ("v", tr.vf, tr.v_optimizer), ("actor", tr.actor, tr.actor_optimizer))


def state(gh, tr):
    torch.cuda.synchronize()
    return tuple(gh.module_params(m) for m in (tr.qf, tr.vf, tr.actor, tr.q_target))


def moments(tr):
    """group -> name -> (exp_avg, exp_avg_sq) through optimizer.state; zeros before the first step (no state yet)."""
    out = {}
    for g, mod, opt in _mods(tr):
        out[g] = {}
        for name, p in mod.named_parameters():
            st = opt.state.get(p) or {}
            out[g][name] = tuple(st[k].detach().cpu().numpy().copy() if k in st else np.zeros(tuple(p.shape), np.float32)
                                 for k in ("exp_avg", "exp_avg_sq"))
    return out


def grads(tr):
    return {g: {name: p.grad.detach().cpu().numpy().copy() for name, p in mod.named_parameters()} for g, mod, _ in _mods(tr)}


def run(gh, cases, case, mode, *, tag, step_kind, plan, tally, counted=lambda row: row[4] < 1024, inject_masks=False):
    """Two judged steps of ``cases[case]``; returns what each step left (losses, gradients, state) for bitwise
    comparisons.  ``plan(row, mode)`` asserts that the case reaches what its table entry records and returns that as
    text; ``step_kind`` is what the trainer must report; ``counted(row)``: the case never takes the loose bound at
    step 1 and its step-2 uses are counted in ``tally`` (the calling file's cap test)."""
    row = cases[case]
    S, A, NH, H, B, E = row[:6]
    reached = plan(row, mode)
    hyper, nets, data, idx = helpers.gs_inputs(case)
    tr = gh.make_trainer(hyper, nets, mode, lr=helpers.GS_LR, seed=helpers.GS_SEED, keep_grads=True)
    assert tr.step_kind(B) == step_kind
    label = f"{case} {mode}" + (" injected masks" if inject_masks else "")
    say(tag, f"{label}: {reached}, S{S} A{A} {NH}x{H} B{B} E{E}")
    buf = gh.make_buffer(hyper, data)
    idx_t = torch.from_numpy(idx).to(gh.DEV)
    tau = float(np.float32(hyper["tau"]))
    left, failures = [], []
    for t in range(helpers.GS_STEPS):
        before, mom0 = state(gh, tr), moments(tr)
        keeps, kw = helpers.gs_keep_masks(hyper, t), {}
        if inject_masks:
            kw["dropout_keep"] = torch.from_numpy(np.stack(keeps)[None].astype(np.uint8)).to(gh.DEV)
        losses = tr.train_steps(buf, 1, B, indices=idx_t[t:t + 1], graph_unroll=0, **kw).cpu().numpy()[0]
        after, mom1, got = state(gh, tr), moments(tr), grads(tr)
        assert tr.total_it == t + 1
        left.append((losses, got, after))
        ref = helpers.gs_reference_step(hyper, before, mode, orc.gather_batch(data, idx[t]), t, keeps)
        # 1. losses
        want = np.array([ref["losses"][k] for k in ("value_loss", "q_loss", "actor_loss")])
        rel = np.abs(losses - want) / np.where(want == 0, 1.0, np.abs(want))  # (a zero reference: the absolute error)
        say(tag, f"{label} step {t + 1}: losses {losses.tolist()} against {want.tolist()}: "
                 f"max rel {rel.max():.2e} (rtol {helpers.GS_LOSS_RTOL[mode]:.0e})")
        if not np.allclose(losses, want, rtol=helpers.GS_LOSS_RTOL[mode], atol=0):
            failures.append(f"step {t + 1}: losses {losses.tolist()} against {want.tolist()}")
        # 2. gradients
        bad, lines, loose, worst, same = helpers.gs_judge_grads(mode, got, ref, B)
        for line in lines:
            say(tag, f"{label} step {t + 1} {line}")
        margins = ", ".join("%s %.1e" % (g, ref["margin"][g]) for g in GROUPS)
        say(tag, f"{label} step {t + 1}: largest gradient error {worst:.2e} of the largest entry, bit-identical entries {same:.4f}, "
                 f"loose bound for {loose or 'no net'} (margins {margins})")
        failures += [f"step {t + 1}: {b}" for b in bad]
        if counted(row):
            if t == 0:
                assert not loose, f"{label}: step 1 within {helpers.GS_MARGIN} of a kink ({ref['margin']}): pick another seed"
            else:
                tally["checks"] += len(GROUPS)
                tally["uses"] += [(case, mode, g) for g in loose]
        # 3. the update, from the GPU's own numbers
        coef = helpers.gs_adam_coef(t + 1, helpers.GS_LR, helpers.GS_LR, hyper["max_steps"])
        top = {}
        for gi, g in enumerate(GROUPS):
            for name in got[g]:
                tgt = dict(t0=before[3][name], t1=after[3][name], tau=tau) if g == "q" else {}
                ub, fig = helpers.gs_judge_update(coef, g, before[gi][name], *mom0[g][name], got[g][name], after[gi][name],
                                                  *mom1[g][name], lr=helpers.GS_LR, **tgt)
                failures += [f"step {t + 1} update {g}/{name}: {b}" for b in ub]
                for k, v in fig.items():
                    top[k] = max(top.get(k, 0.0), v)
        say(tag, f"{label} step {t + 1} update: exp_avg {top['m']:.3f}e-6, exp_avg_sq {top['v']:.3f}e-6 (bound 1e-6 relative), parameter "
                 f"{top['p_ulp']:.2f} ulp32, beyond one ulp32 {top['p_lr']:.2e} lr (bound 1 ulp32 + 1e-5 lr), target {top['t_ulp']:.2f} ulp32 (bound 2)")
    # 4. the compute and target copies the second update wrote
    s, a = data["observations"][:N_FWD], data["actions"][:N_FWD]
    ts, ta = (torch.from_numpy(np.ascontiguousarray(x)).to(gh.DEV) for x in (s, a))
    fref = helpers.forward_reference(after, mode, s, a)
    for which in ("q", "v", "actor", "q_target"):
        out = tr.forward(which, ts, ta if which in ("q", "q_target") else None).cpu().numpy()
        ok, text = helpers.forward_judge(mode, out, *fref[which], NH + 1, max(H, S + A))
        say(tag, f"{label} forward {which} after step {helpers.GS_STEPS}: {text}")
        if not ok:
            failures.append(f"forward {which}: {text}")
    assert not failures, f"{label}:\n  " + "\n  ".join(failures)
    return left


def assert_runs_bit_identical(own, injected):
    """Two runs of one case (run's return values): losses, gradients and states equal bit for bit."""
    for t, ((l0, g0, s0), (l1, g1, s1)) in enumerate(zip(own, injected)):
        np.testing.assert_array_equal(l0.view(np.uint32), l1.view(np.uint32), err_msg=f"step {t + 1} losses")
        for g in GROUPS:
            for k in g0[g]:
                np.testing.assert_array_equal(g0[g][k].view(np.uint32), g1[g][k].view(np.uint32), err_msg=f"step {t + 1} grad {g}/{k}")
        for a, b in zip(s0, s1):
            for k in a:
                np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"step {t + 1} {k}")
