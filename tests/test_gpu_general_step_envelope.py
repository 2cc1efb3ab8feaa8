"""The general layer-wise training step (csrc/iql_deep.hip: kd_forward / kd_backward / kd_update) over its stated
envelope -- n_hidden 1..6, hidden_dim 1..1024 -- at the widths no other test trains: hidden widths that are
not a multiple of 4 (kd_update's dW = dZ^T X orientation on hidden and output layers: its scalar stores of the
transposed copy wt, its bias sums, its 64 x 16 tq tile table, its edge guards) and the 64 x 64 update tiles
(tq = 4), reached by width and by batch size.  -m gpu.

Every step is judged at the GPU's own parameters.  A step is one train_steps(buf, 1, B, indices=...) on a
trainer with keep_grads; before and after it the test reads the parameters, q_target, the Adam moments
(optimizer.state) and p.grad.  The reference of step t is evaluated at what the GPU held BEFORE step t, so the
two sides never drift apart and every check is a single-step comparison.  Step 1 runs on the copies kd_sync
made, step 2 on the copies kd_update wrote (wc, wt, tc, the target arena).  lr = 1e-2: one sign-like Adam step
moves every weight by several bf16 ulps, so a copy that was not refreshed shows in bf16 too.

Checked after each step, in fp32 and bf16 (helpers.gs_*; none of the bounds is fitted to what the kernels give):
  losses     against the oracle in the same mode, the project's rtol 3e-5 / 6e-3 (_shape_case).
  gradients  of every tensor, log_std included, relative to the largest reference entry; a reference that is
             identically zero must be met exactly.
             fp32: float64 autograd of the three losses (helpers.gs_f64_step); the project's 5e-5.
             bf16: the oracle's autocast restatement; the yardstick is what the same restatement with every sum
             in fp64 differs from it by (gap): max |err| <= max(4 max gap, 2e-2 of the largest entry),
             median |err| <= max(4 median gap, a quarter bf16 ulp at the median |reference|).
             A net whose reference reports a pre-activation (for V also an advantage) within 1e-5 of a kink in
             this step gets the project's loose bound for it, max(4 / B, 2e-2 in bf16).  At B >= 1024 (3.9e-3)
             freely -- those cases cannot avoid a kink; at B < 1024 never at step 1, and at step 2 in at most one
             in ten of the (case, mode, net) checks: counted, and test_loose_bound_stays_within_its_cap fails beyond.
  update     float64 Adam (make_adam_coef's coefficients, the actor's lr on the cosine schedule) and Polyak in the
             lerp form from the GPU's own p0, m0, v0, g, t0: moments 1e-6 relative (floor 1e-37), parameters
             1 ulp32 + 1e-5 lr, target 2 ulp32 -- biases and log_std too (helpers.gs_judge_update has the derivation).
  copies     after step 2, forward("q" | "v" | "actor" | "q_target") on 20 rows against the CPU references on the
             current state_dicts, under tests/test_gpu_forward_envelope.py's bounds.
The offset cases (hidden biases +- 3) test tile geometry only: most units are on or off for the whole batch (of
V's hidden units, 3 to 15 % see both signs at step 1, against 94 % at 3 x 129), which keeps a wide layer's thousands
of pre-activations away from the kink; the per-sample relu' masks are what the small cases test.  After one step at
lr = 1e-2 the outputs of these wide nets have moved by tens (~ lr x 3 x width): at step 2 their actor's tanh is
saturated and exp(beta adv) is clamped or underflows, so the actor's gradients there are exact zeros on both sides
(helpers.gs_f64_step holds those two tensors as the fp32 numbers the step stores); Q and V keep ordinary gradients.
The seed of a case is the first at which the reference, by itself, keeps its margins and, in bf16, agrees with a
third restatement of itself within these bounds (helpers.gs_pick_seed): at 6 x 1024 most seeds do not, because one
rounding tie that falls the other way flips relu' of units tens of ulps from zero (4 % of the largest entry).  tests/test_general_step_envelope_host.py shows
on the CPU that the reference alone keeps its margins and that these bounds reject a zeroed or transposed tile,
a bias block from the wrong wave and a backward through stale weights.

Every test prints its figures (IQLTEST lines with -s, IQL_TEST_DIAG=<file>).  An MI355X gave, over the 44 runs:
  every case reached the tile width and orientation of its table entry (asserted from the restated rule);
  losses     fp32 within 1.1e-5, bf16 within 1.3e-3 of the oracle's;
  gradients  fp32: largest error 1.5e-5 of the largest entry (1 x 1023 at step 2; 4.9e-6 elsewhere), 1.8e-6 at batch 1024;
             bf16: 39 of the 44 (run, step) pairs bit-identical to the oracle in every entry, the others in >= 0.9994 of
             their entries except step 1 of 6 x 1024 (0.895; largest error 7.4e-3 of the largest entry, a third of its
             bound); at batch 1024 at most 1.7e-4;
  loose bound  at B < 1024: 0 uses at step 1, 0 of 114 checks at step 2.  At batch 1024 it judged 643 tensors, whose
             errors stayed at 2.1e-6 (fp32) / 2.3e-3 (bf16): no relu' actually fell the other way;
  update     exp_avg within 0.06e-6, exp_avg_sq within 0.17e-6 relative; parameters within 1 ulp32 + 2.5e-7 lr;
             target within 0.50 ulp32 -- the last rounding alone;
  copies     fp32 max |err| 4.6e-5 (6 x 1024, outputs ~1e5); bf16: 87 of 88 output arrays bit-identical, the other in 0.975.
  The two dropout runs (Philox / injected masks) were bit-identical in losses, gradients and parameters."""
import os

import numpy as np
import pytest
import torch

from oracle import iql_oracle as orc
from tests import helpers

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16")
N_FWD = 20
GROUPS = ("q", "v", "actor")
LOOSE = {"checks": 0, "uses": []}  # step-2 (case, mode, net) checks at B < 1024, and those that took the loose bound


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _say(line):
    print("IQLTEST general-step " + line)
    path = os.environ.get("IQL_TEST_DIAG")
    if path:
        with open(path, "a") as f:
            f.write("general-step " + line + "\n")


def _mods(tr):
    return (("q", tr.qf, tr.q_optimizer), ("v", tr.vf, tr.v_optimizer), ("actor", tr.actor, tr.actor_optimizer))


def _state(gh, tr):
    torch.cuda.synchronize()
    return tuple(gh.module_params(m) for m in (tr.qf, tr.vf, tr.actor, tr.q_target))


def _moments(tr):
    """group -> name -> (exp_avg, exp_avg_sq) through optimizer.state; zeros before the first step (no state yet)."""
    out = {}
    for g, mod, opt in _mods(tr):
        out[g] = {}
        for name, p in mod.named_parameters():
            st = opt.state.get(p) or {}
            out[g][name] = tuple(st[k].detach().cpu().numpy().copy() if k in st else np.zeros(tuple(p.shape), np.float32)
                                 for k in ("exp_avg", "exp_avg_sq"))
    return out


def _grads(tr):
    return {g: {name: p.grad.detach().cpu().numpy().copy() for name, p in mod.named_parameters()} for g, mod, _ in _mods(tr)}


def _run(gh, case, mode, inject_masks=False):
    """Two judged steps of a case; returns what each step left (losses, gradients, state) for bitwise comparisons."""
    S, A, NH, H, B, E, det, drop, offset, seed, tq, orient = helpers.GS_CASES[case]
    assert helpers.gs_update_plan(S, A, NH, H, B, E)[:2] == (tq, orient)
    hyper, nets, data, idx = helpers.gs_inputs(case)
    tr = gh.make_trainer(hyper, nets, mode, lr=helpers.GS_LR, seed=helpers.GS_SEED, keep_grads=True)
    assert tr.step_kind(B) == "general"
    label = f"{case} {mode}" + (" injected masks" if inject_masks else "")
    _say(f"{label}: tq {tq}, hidden/output layers {orient}, S{S} A{A} {NH}x{H} B{B} E{E}")
    buf = gh.make_buffer(hyper, data)
    idx_t = torch.from_numpy(idx).to(gh.DEV)
    tau = float(np.float32(hyper["tau"]))
    left, failures = [], []
    for t in range(helpers.GS_STEPS):
        before, mom0 = _state(gh, tr), _moments(tr)
        keeps, kw = helpers.gs_keep_masks(hyper, t), {}
        if inject_masks:
            kw["dropout_keep"] = torch.from_numpy(np.stack(keeps)[None].astype(np.uint8)).to(gh.DEV)
        losses = tr.train_steps(buf, 1, B, indices=idx_t[t:t + 1], graph_unroll=0, **kw).cpu().numpy()[0]
        after, mom1, grads = _state(gh, tr), _moments(tr), _grads(tr)
        assert tr.total_it == t + 1
        left.append((losses, grads, after))
        ref = helpers.gs_reference_step(hyper, before, mode, orc.gather_batch(data, idx[t]), t, keeps)
        # 1. losses
        want = np.array([ref["losses"][k] for k in ("value_loss", "q_loss", "actor_loss")])
        rel = np.abs(losses - want) / np.where(want == 0, 1.0, np.abs(want))  # (a zero reference: the absolute error)
        _say(f"{label} step {t + 1}: losses {losses.tolist()} against {want.tolist()}: "
             f"max rel {rel.max():.2e} (rtol {helpers.GS_LOSS_RTOL[mode]:.0e})")
        if not np.allclose(losses, want, rtol=helpers.GS_LOSS_RTOL[mode], atol=0):
            failures.append(f"step {t + 1}: losses {losses.tolist()} against {want.tolist()}")
        # 2. gradients
        bad, lines, loose, worst, same = helpers.gs_judge_grads(mode, grads, ref, B)
        for line in lines:
            _say(f"{label} step {t + 1} {line}")
        margins = ", ".join("%s %.1e" % (g, ref["margin"][g]) for g in GROUPS)
        _say(f"{label} step {t + 1}: largest gradient error {worst:.2e} of the largest entry, bit-identical entries {same:.4f}, "
             f"loose bound for {loose or 'no net'} (margins {margins})")
        failures += [f"step {t + 1}: {b}" for b in bad]
        if B < 1024:
            if t == 0:
                assert not loose, f"{label}: step 1 within {helpers.GS_MARGIN} of a kink ({ref['margin']}): pick another seed"
            else:
                LOOSE["checks"] += len(GROUPS)
                LOOSE["uses"] += [(case, mode, g) for g in loose]
        # 3. the update, from the GPU's own numbers
        coef = helpers.gs_adam_coef(t + 1, helpers.GS_LR, helpers.GS_LR, hyper["max_steps"])
        top = {}
        for gi, g in enumerate(GROUPS):
            for name in grads[g]:
                tgt = dict(t0=before[3][name], t1=after[3][name], tau=tau) if g == "q" else {}
                ub, fig = helpers.gs_judge_update(coef, g, before[gi][name], *mom0[g][name], grads[g][name], after[gi][name],
                                                  *mom1[g][name], lr=helpers.GS_LR, **tgt)
                failures += [f"step {t + 1} update {g}/{name}: {b}" for b in ub]
                for k, v in fig.items():
                    top[k] = max(top.get(k, 0.0), v)
        _say(f"{label} step {t + 1} update: exp_avg {top['m']:.3f}e-6, exp_avg_sq {top['v']:.3f}e-6 (bound 1e-6 relative), parameter "
             f"{top['p_ulp']:.2f} ulp32, beyond one ulp32 {top['p_lr']:.2e} lr (bound 1 ulp32 + 1e-5 lr), target {top['t_ulp']:.2f} ulp32 (bound 2)")
    # 4. the compute and target copies the second update wrote
    s, a = data["observations"][:N_FWD], data["actions"][:N_FWD]
    ts, ta = (torch.from_numpy(np.ascontiguousarray(x)).to(gh.DEV) for x in (s, a))
    fref = helpers.forward_reference(after, mode, s, a)
    for which in ("q", "v", "actor", "q_target"):
        got = tr.forward(which, ts, ta if which in ("q", "q_target") else None).cpu().numpy()
        ok, text = helpers.forward_judge(mode, got, *fref[which], NH + 1, max(H, S + A))
        _say(f"{label} forward {which} after step {helpers.GS_STEPS}: {text}")
        if not ok:
            failures.append(f"forward {which}: {text}")
    assert not failures, f"{label}:\n  " + "\n  ".join(failures)
    return left


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in helpers.GS_CASES if helpers.GS_CASES[c][7] is None])
def test_general_step_at_the_gpus_own_parameters(gh, case, mode):
    _run(gh, case, mode)


@pytest.mark.parametrize("mode", MODES)
def test_dropout_at_an_odd_width(gh, mode):
    """3 x 33 at batch 17 with dropout 0.25: once with the device's Philox masks (the reference's masks from
    oracle/philox.py), once with the same masks injected through dropout_keep=.  Both runs are judged as every
    case is, and their losses, gradients and parameters are bit-identical to each other."""
    case = "3x33_b17_dropout"
    own, injected = _run(gh, case, mode), _run(gh, case, mode, inject_masks=True)
    for t, ((l0, g0, s0), (l1, g1, s1)) in enumerate(zip(own, injected)):
        np.testing.assert_array_equal(l0.view(np.uint32), l1.view(np.uint32), err_msg=f"step {t + 1} losses")
        for g in GROUPS:
            for k in g0[g]:
                np.testing.assert_array_equal(g0[g][k].view(np.uint32), g1[g][k].view(np.uint32), err_msg=f"step {t + 1} grad {g}/{k}")
        for a, b in zip(s0, s1):
            for k in a:
                np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"step {t + 1} {k}")


def test_loose_bound_stays_within_its_cap():
    """Runs last: of the step-2 (case, mode, net) checks at B < 1024 that this session made, at most one in ten
    took the loose bound (none at step 1: asserted where it is judged)."""
    _say(f"loose-bound uses at step 2, B < 1024: {len(LOOSE['uses'])} of {LOOSE['checks']} checks {LOOSE['uses']}")
    assert len(LOOSE["uses"]) * 10 <= LOOSE["checks"], LOOSE
