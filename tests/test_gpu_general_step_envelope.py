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
import pytest
import torch

from tests import helpers, step_envelope

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16")
LOOSE = step_envelope.new_tally()  # step-2 (case, mode, net) checks at B < 1024, and those that took the loose bound


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _say(line):
    step_envelope.say("general-step", line)


def _plan(row, mode):
    """The tile width and orientation the case records are what deep_create's rule, restated, gives."""
    S, A, NH, H, B, E = row[:6]
    tq, orient = row[10:12]
    assert helpers.gs_update_plan(S, A, NH, H, B, E)[:2] == (tq, orient)
    return f"tq {tq}, hidden/output layers {orient}"


def _run(gh, case, mode, inject_masks=False):
    """Two judged steps of a case (step_envelope.run): what each step left, for bitwise comparisons."""
    return step_envelope.run(gh, helpers.GS_CASES, case, mode, tag="general-step", step_kind="general", plan=_plan,
                             tally=LOOSE, inject_masks=inject_masks)


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
    step_envelope.assert_runs_bit_identical(_run(gh, case, mode), _run(gh, case, mode, inject_masks=True))


def test_loose_bound_stays_within_its_cap():
    """Runs last: of the step-2 (case, mode, net) checks at B < 1024 that this session made, at most one in ten
    took the loose bound (none at step 1: asserted where it is judged)."""
    _say(f"loose-bound uses at step 2, B < 1024: {len(LOOSE['uses'])} of {LOOSE['checks']} checks {LOOSE['uses']}")
    assert len(LOOSE["uses"]) * 10 <= LOOSE["checks"], LOOSE
