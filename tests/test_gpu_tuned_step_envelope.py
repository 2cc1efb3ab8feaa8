"""The tuned three-kernel training step (csrc/iql_step.hip: k_forward / k_backward / k_update and the throughput pair
k_forward_tp / k_backward_tp; n_hidden 2, hidden_dim 64 / 128 / 256) judged step by step at the edges of the
envelope its header admits, and in every instantiation one trainer can launch.  -m gpu.

The judging is the general step's (tests/step_envelope.py; the docstring of tests/test_gpu_general_step_envelope.py
says what every bound is and where it comes from): each of two steps at the GPU's own parameters -- losses against
the oracle, every gradient against float64 autograd (fp32) or the oracle's autocast restatement (bf16), Adam and
Polyak from the device's own p0, m0, v0, g, then forwards on the copies the second update wrote (wc, w2ct, w3t, tc,
the target arena).  The bounds are helpers.GS_* as they stand.  helpers.TS_CASES is the table; before a case is
stepped the launch plan it records is compared with helpers.ts_plan, the launchers' selection rules restated (the
CU count read from the device).

  edges     S + A = 128 (all four bf16 / eight fp32 layer-1 k-steps) at an odd S and at A = 32; A = 17 (one real
            column in the second output tile), A = 16 and S = 16 (exact tiles), S = A = 1; E = 8 with A = 32
            (OUTW = 50 of the 64 columns the backward's finish covers); padded batches 17, 33, 40, 1020, 1030.
  kernels   k_forward<MT, PW, DROP> in all eight combinations, k_forward_tp with and without dropout;
            k_backward<PRE, PW, NV> in all six (PW 2 has no PRE), k_backward_tp on one and on two XCDs per net;
            k_update<LAT, CNT> in all four.  Precision and hidden width multiply these: every (kernel, parameters)
            above runs in fp32 and bf16 (the throughput pair and CNT are bf16 only), at the widths the table names,
            not at all three.  tests/test_tuned_step_envelope_host.py asserts this coverage from ts_plan.
            Reached by a K-seed group only, and covered by the bitwise group check below alone: two forward parts
            per work-group under 1024 rows a seed, two backward parts under 512, and k_update's 256-thread variant
            on a table that a lone seed runs with 512 (every group launch).
  cases at B >= 1024 have offset biases and a picked seed (helpers.gs_pick_seed searches them too), so they are
            judged under the tight bounds like every other case: never the loose bound at step 1, its uses at step 2
            counted under the one-in-ten cap (test_loose_bound_stays_within_its_cap).
  dropout   rows run twice, on the device's Philox masks and on the same masks injected through dropout_keep=; both
            are judged and must agree bit for bit.
  groups    three trainers with their own nets and seeds at S + A = 128 (H = 64, E = 3, and H = 128 with A = 32), five
            steps on the device's own indices as SeedGroup(mode="group") and "split", against the same trainers
            stepped alone: losses, _params, _target and both moments bit for bit.
  LDS bound the largest batch check_cfg admits for (S 20, A 32, H 64, E 8, Gaussian) by the rule restated in
            helpers.ts_max_batch, 1,744, creates a trainer and 1,760 raises; one fp32 step at 1,744: the three losses
            and the log_std gradient, the sums that live in k_update's LDS.

Every test prints its figures (IQLTEST lines with -s, IQL_TEST_DIAG=<file>).  An MI355X gave, over the 62 runs
(25 cases x 2 precisions, the six dropout rows twice) -- these are reports, not bounds:
  every case took the instantiations of its table entry (asserted from the restated rules; 256 CUs);
  losses     fp32 within 7.1e-6 (1020 rows at H = 64 with dropout, step 1), bf16 within 3.7e-7 of the oracle's;
  gradients  fp32: largest error 1.5e-5 of the largest entry (H = 128 at batch 1024, step 2);
             bf16: 52 of the 62 (run, step 1 | 2) pairs bit-identical to the oracle in every entry, the others in
             >= 0.9993 of their entries; largest error 5.3e-3 of the largest entry (E = 8 at batch 256, step 1), a
             quarter of its bound;
  loose bound  0 uses at step 1, 0 of 186 checks at step 2, the batches from 1020 to 1152 rows included;
  update     exp_avg within 0.06e-6, exp_avg_sq within 0.17e-6 relative; parameters within 1 ulp32 + 2.6e-7 lr;
             target within 0.50 ulp32 -- the last rounding alone;
  copies     fp32 max |err| 1.2e-5 (E = 6 at batch 320 with dropout); bf16: all 124 output arrays bit-identical;
  dropout    the Philox and the injected-mask run of each of the six rows were bit-identical in losses, gradients
             and parameters;
  groups     all eight (case, group | split, precision) sets of three members equal to the members alone bit for bit;
  LDS bound  the library and helpers.ts_max_batch agree on 1,744 (1,760 is refused: "too large for action_dim 32");
             losses within 2.5e-7, the log_std gradient within 3.5e-7 of its largest entry under the tight bound (the
             actor kept a margin of 2.6e-5).
No case failed and nothing in csrc/iql_step.hip had to change."""
import numpy as np
import pytest
import torch

from oracle import iql_oracle as orc
from tests import helpers, step_envelope

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16")
TAG = "tuned-step"
LOOSE = step_envelope.new_tally()  # step-2 (case, mode, net) checks, and those that took the loose bound
GROUP_CASES = ("s111a17_h64_e3", "s96a32_h128_det")
GROUP_STEPS = 5
LDS_SHAPE = (20, 32, 64, 8)  # S, A, H, E: Gaussian, 42 floats of k_update's LDS per 16 rows


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _say(line):
    step_envelope.say(TAG, line)


def _plan(row, mode):
    """The instantiations the case records are what the launchers' rules, restated, select on this device."""
    S, A, NH, H, B, E, det, drop = row[:8]
    got = helpers.ts_plan(S, A, H, B, E, mode, drop, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert got == row[10][mode], (got, row[10][mode])
    return got


def _run(gh, case, mode, inject_masks=False):
    # counted: every case below 1024 rows, and the offset cases beyond (their seeds are picked like the others')
    return step_envelope.run(gh, helpers.TS_CASES, case, mode, tag=TAG, step_kind="tuned", plan=_plan, tally=LOOSE,
                             counted=lambda row: row[4] < 1024 or row[8], inject_masks=inject_masks)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in helpers.TS_CASES if helpers.TS_CASES[c][7] is None])
def test_tuned_step_at_the_gpus_own_parameters(gh, case, mode):
    _run(gh, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in helpers.TS_CASES if helpers.TS_CASES[c][7] is not None])
def test_dropout_philox_and_injected_masks(gh, case, mode):
    """A dropout row on the device's Philox masks (the reference's from oracle/philox.py) and on the same masks
    injected through dropout_keep=: both judged as every case is, and bit-identical to each other."""
    step_envelope.assert_runs_bit_identical(_run(gh, case, mode), _run(gh, case, mode, inject_masks=True))


def _members(gh, case, mode):
    """Three trainers of a case's shape, each with nets of its own (numpy seeds 100..102) and its own Philox key."""
    return [gh.make_trainer(*helpers.gs_inputs(case, seed=100 + k)[:2], mode, lr=helpers.GS_LR, seed=11 + k) for k in range(3)]


def _arenas(tr):
    return {k: getattr(tr, k).clone() for k in ("_params", "_target", "_exp_avg", "_exp_avg_sq")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group_mode", ("group", "split"))
@pytest.mark.parametrize("case", GROUP_CASES)
def test_group_launches_at_the_edges_equal_the_members_alone(gh, case, group_mode, mode):
    import iqlpref_amd as ia
    hyper, _, data, _ = helpers.gs_inputs(case)
    B, buf = hyper["batch"], gh.make_buffer(hyper, data)
    alone = _members(gh, case, mode)
    want = [tr.train_steps(buf, GROUP_STEPS, B, graph_unroll=0).clone() for tr in alone]
    members = _members(gh, case, mode)
    assert all(tr.step_kind(B) == "tuned" for tr in members)
    group = ia.SeedGroup(members, mode=group_mode)
    try:
        got = group.train_steps(buf, GROUP_STEPS, B, return_losses=True, graph_unroll=0)
        torch.cuda.synchronize()
        for k, (a, m) in enumerate(zip(alone, members)):
            assert m.total_it == a.total_it == GROUP_STEPS
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), f"member {k}: losses"
            for name, t in _arenas(a).items():
                assert torch.equal(getattr(m, name).view(torch.int32), t.view(torch.int32)), f"member {k}: {name}"
    finally:
        group.close()
    _say(f"group {case} {mode} {group_mode}: 3 members x {GROUP_STEPS} steps bit-identical to the members alone")


def test_largest_batch_of_the_lds_rule(gh):
    """check_cfg's rule, (round_up(B, 16) / 16)(E + 2 + A) + E + 2 <= update_lds_floats(): its largest batch steps,
    the next slab is refused.  One fp32 step at the largest: losses at GS_LOSS_RTOL, the log_std gradient by
    gs_judge_grad (under the loose kink bound where the actor is within GS_MARGIN of a kink: 1,744 rows of an
    unshifted net cannot avoid one)."""
    S, A, H, E = LDS_SHAPE
    B = helpers.ts_max_batch(A, E, False)
    assert B == 1744
    row = (S, A, 2, H, B, E, False, None, False, 0)
    hyper, nets, data, idx = helpers.gs_inputs(row)
    with pytest.raises(NotImplementedError, match="too large"):
        gh.make_trainer(dict(hyper, batch=B + 16), nets, "fp32", lr=helpers.GS_LR, seed=helpers.GS_SEED).step_kind(B + 16)
    tr = gh.make_trainer(hyper, nets, "fp32", lr=helpers.GS_LR, seed=helpers.GS_SEED, keep_grads=True)
    assert tr.step_kind(B) == "tuned"
    before = step_envelope.state(gh, tr)
    buf = gh.make_buffer(hyper, data)
    losses = tr.train_steps(buf, 1, B, indices=torch.from_numpy(idx[:1]).to(gh.DEV), graph_unroll=0).cpu().numpy()[0]
    got = step_envelope.grads(tr)["actor"]["log_std"]
    ref = helpers.gs_reference_step(hyper, before, "fp32", orc.gather_batch(data, idx[0]), 0)
    want = np.array([ref["losses"][k] for k in ("value_loss", "q_loss", "actor_loss")])
    _say(f"lds bound B{B}: losses {losses.tolist()} against {want.tolist()}: max rel {np.abs(losses / want - 1).max():.2e}")
    np.testing.assert_allclose(losses, want, rtol=helpers.GS_LOSS_RTOL["fp32"], atol=0)
    loose = helpers.gs_loose_bound("fp32", B) if ref["margin"]["actor"] < helpers.GS_MARGIN else None
    ok, text, _, _ = helpers.gs_judge_grad("fp32", got, ref["grads"]["actor"]["log_std"], None, loose)
    _say(f"lds bound B{B}: grad actor/log_std (margin {ref['margin']['actor']:.1e}): {text}")
    assert ok, text


def test_loose_bound_stays_within_its_cap():
    """Runs last: of the step-2 (case, mode, net) checks that this session made, at most one in ten took the loose
    bound (none at step 1: asserted where it is judged)."""
    _say(f"loose-bound uses at step 2: {len(LOOSE['uses'])} of {LOOSE['checks']} checks {LOOSE['uses']}")
    assert len(LOOSE["uses"]) * 10 <= LOOSE["checks"], LOOSE
