"""The references, bounds and launch-plan restatement of tests/test_gpu_tuned_step_envelope.py, checked on the CPU
(the companion tests/test_general_step_envelope_host.py is for the general step):

a. the fp32 oracle against float64 autograd (helpers.gs_f64_step) over helpers.TS_CASES: pins the oracle's backward
   at S + A = 128, A = 32, S = A = 1, E = 8 and on padded batches, where no golden vector exists;
b. the reference by itself stays 2e-5 away from every kink at both steps in both modes on the committed seeds -- the
   offset cases at B >= 1024 included -- and in bf16 agrees with a third restatement of itself within the bounds the
   GPU is held to; the committed seed is the first the picker accepts;
c. helpers.ts_plan at the thresholds of the launchers' rules, the item-table size behind k_update's LAT, the LDS
   batch rule, and that the table reaches every (kernel, parameters) one trainer can launch;
d. the judges reject what a wrong tuned kernel would produce -- shown on damaged COPIES of the reference."""
import numpy as np
import pytest

from oracle import iql_oracle as orc
from tests import helpers
from tests.test_general_step_envelope_host import _copy, _step2_reference

CASES = list(helpers.TS_CASES)
MODES = ("fp32", "bf16")


_row = helpers.TS_CASES.__getitem__


# ---- (c) the table and the plan
@pytest.mark.parametrize("case", CASES)
def test_case_is_a_tuned_shape_and_reaches_its_plan(case):
    S, A, NH, H, B, E, det, drop, offset, seed, plan = _row(case)
    assert NH == 2 and H in (64, 128, 256) and 2 <= E <= 8 and 1 <= A <= 32 and S + A <= 128
    assert B <= helpers.ts_max_batch(A, E, det) and case not in helpers.GS_CASES
    assert offset or B < 1024  # (only the offset biases keep 1024 rows away from the kinks)
    for mode in MODES:
        assert helpers.ts_plan(S, A, H, B, E, mode, drop) == plan[mode], (case, mode)


def _tokens(mode):
    return {tok for c in CASES for tok in helpers.TS_CASES[c][10][mode].split()[:3]}


def test_table_reaches_every_instantiation_of_one_trainer():
    """Per precision: k_forward<MT, PW, DROP> in all eight combinations, k_backward<PRE, PW, NV> in all six (two parts
    per work-group have no PRE variant), k_update<LAT, CNT> (CNT: bf16 only); in bf16 also k_forward_tp<DROP> and
    k_backward_tp on one and on two XCDs per net.  And the edges of the header's envelope."""
    fwd = {f"F<{mt},{pw},{d}>" for mt in (1, 2) for pw in (1, 2) for d in (0, 1)}
    bwd = {f"B<{pre},{pw},{nv}>" for pre, pw in ((1, 1), (0, 1), (0, 2)) for nv in (0, 1)}
    assert _tokens("fp32") == fwd | bwd | {"U<1,0>", "U<0,0>"}
    assert _tokens("bf16") == fwd | bwd | {"U<1,0>", "U<0,0>", "U<1,1>", "U<0,1>", "Ftp<0>", "Ftp<1>", "Btp<1>", "Btp<2>"}
    rows = [_row(c) for c in CASES]
    k1 = {(m, r[10][m].split("k1 ")[1].split()[0]) for r in rows for m in MODES}
    assert {("fp32", "8/7"), ("bf16", "4/4"), ("fp32", "8/6"), ("bf16", "4/3"), ("fp32", "1/1"), ("bf16", "3/2")} <= k1
    assert {(r[0], r[1]) for r in rows} >= {(1, 1), (16, 16), (111, 17), (96, 32)}
    assert any(r[5] == 8 and r[1] == 32 for r in rows) and {r[3] for r in rows} == {64, 128, 256}
    assert any(r[4] % 16 for r in rows if r[7]) and any(r[4] % 16 for r in rows if not r[7])  # padded, with / without masks


def test_plan_at_its_thresholds():
    P = lambda *a, **k: helpers.ts_plan(17, 6, *a, **k).split()[:3]
    # 512 rows a launch: 32-row forward work-groups (batch a multiple of 32), two backward parts from H = 128 on
    assert P(128, 496, 2, "fp32", None) == ["F<1,1,0>", "B<1,1,0>", "U<1,0>"]
    assert P(128, 512, 2, "fp32", None) == ["F<2,1,0>", "B<0,2,0>", "U<1,0>"]
    assert P(128, 511, 2, "bf16", None) == ["F<2,1,0>", "B<0,2,1>", "U<1,1>"]  # (511 rows are 512 with one that does not count)
    assert P(128, 528, 2, "fp32", None)[0] == "F<1,1,0>" and P(128, 256, 2, "fp32", None, n_seeds=2)[:2] == ["F<2,1,0>", "B<0,2,0>"]
    # 1024 rows: two forward parts; one backward part loses PRE
    assert P(128, 1008, 2, "fp32", None)[:2] == ["F<1,1,0>", "B<0,2,0>"] and P(128, 1024, 2, "fp32", None)[:2] == ["F<2,2,0>", "B<0,2,0>"]
    assert P(64, 1008, 2, "fp32", None)[:2] == ["F<1,1,0>", "B<1,1,0>"] and P(64, 1024, 2, "fp32", None)[:2] == ["F<2,1,0>", "B<0,1,0>"]
    assert P(128, 1023, 2, "fp32", None)[:2] == ["F<2,2,0>", "B<0,2,1>"] and P(128, 128, 2, "fp32", None, n_seeds=8)[0] == "F<2,2,0>"
    # H = 64 never takes two parts, alone or in a group
    for B in range(16, 4097, 16):
        for K in (1, 2, 8):
            f, b = helpers.ts_plan(11, 3, 64, B, 2, "bf16", None, n_seeds=K).split()[:2]
            assert f[4] == "1" and b[4] == "1", (B, K, f, b)
    # the throughput window, by work-group counts ...
    assert helpers.ts_tp_window(71, 200) == (False, False) and helpers.ts_tp_window(72, 143) == (True, False)
    assert helpers.ts_tp_window(256, 144) == (True, True) and helpers.ts_tp_window(257, 144) == (False, False)
    assert helpers.ts_tp_window(200, 256) == (True, True) and helpers.ts_tp_window(200, 257) == (True, False)
    # ... and by the shapes next to them (evaluations 2E + 3 are odd and >= 7: 71, 256 and 257 forward work-groups, and
    # 143 backward ones, have no shape): 70 / 72 / 252 / 259 forward, 136 / 144 backward
    assert P(256, 640, 2, "bf16", None)[0] == "F<2,1,0>" and P(256, 512, 3, "bf16", None)[:2] == ["Ftp<0>", "B<0,2,0>"]
    assert P(256, 2304, 2, "bf16", None)[0] == "Ftp<0>" and P(256, 2368, 2, "bf16", None)[0] == "F<2,2,0>"
    assert P(256, 1088, 2, "bf16", None)[:2] == ["Ftp<0>", "B<0,2,0>"] and P(256, 1152, 2, "bf16", None)[:2] == ["Ftp<0>", "Btp<2>"]
    assert P(256, 448, 4, "bf16", None)[:2] == ["Ftp<0>", "B<1,1,0>"] and P(256, 1024, 3, "bf16", None)[:2] == ["Ftp<0>", "Btp<1>"]  # (36 slabs of 5 nets: one XCD each)
    # only bf16 at H = 256, a batch of whole 64 rows, none of them padding
    assert P(256, 512, 8, "fp32", None)[0] == "F<2,1,0>" and P(128, 512, 8, "bf16", None)[0] == "F<2,1,0>"
    assert P(256, 288, 8, "bf16", None)[:2] == ["F<1,1,0>", "B<1,1,0>"]
    assert P(256, 250, 8, "bf16", None) == ["F<1,1,0>", "B<1,1,1>", "U<0,1>"] and P(256, 256, 8, "bf16", 0.1)[0] == "Ftp<1>"
    # a group launch: the 256-thread k_update whatever the table
    assert P(64, 16, 2, "fp32", None, n_seeds=2)[2] == "U<0,0>"


def test_update_table_slots():
    """The item count per net is (H/64)(H/32) + H/16 + ceil(out_pad/64)(H/32): 8, 20, 56.  TwinQ at H = 256: 224 items in
    28 rows of 8; 16 idle slots at batch 256 make 30 rows, 32 at batch 512 -- one slot per CU, exactly -- and 64 at batch
    1024 do not fit; with dropout 32 idle slots from the first slab on."""
    assert [helpers.ts_update_slots(H, 16, 2, None) for H in (64, 128, 256)] == [40, 88, 232]
    assert helpers.ts_update_slots(256, 256, 2, None) == 240 and helpers.ts_update_slots(256, 512, 2, None) == 256
    assert helpers.ts_update_slots(256, 528, 2, None) == 264 and helpers.ts_update_slots(256, 1024, 2, None) == 288
    assert helpers.ts_update_slots(256, 16, 2, 0.1) == 256 and helpers.ts_update_slots(256, 512, 2, 0.1) == 256
    assert helpers.ts_update_slots(256, 48, 8, None) == 568 and helpers.ts_update_slots(128, 16, 8, None) == 208  # 560 / 200 items
    lat = lambda B, **k: helpers.ts_plan(29, 8, 256, B, 2, "fp32", None, **k).split()[2]
    assert lat(512) == "U<1,0>" and lat(528) == "U<0,0>" and lat(512, cus=255) == "U<0,0>" and lat(1024, cus=304) == "U<1,0>"


def test_lds_batch_rule():
    """(round_up(B, 16) / 16)(E + 2 + A) + E + 2 <= 4608 floats: 1,744 rows at E = 8, A = 32; a deterministic policy has
    no log_std partials."""
    assert helpers.TS_UPDATE_LDS == 2 * max(64 * 36, 16 * 132)
    assert helpers.ts_max_batch(32, 8, False) == 1744 and 109 * 42 + 10 <= 4608 < 110 * 42 + 10
    assert helpers.ts_max_batch(32, 8, True) == 459 * 16 and helpers.ts_max_batch(1, 2, False) == 920 * 16


# ---- (a) the oracle at these shapes
def _first_step(case):
    hyper, nets, data, idx = helpers.gs_inputs(case)
    return hyper, nets + (nets[0],), orc.gather_batch(data, idx[0]), helpers.gs_keep_masks(hyper, 0)


@pytest.mark.parametrize("case", CASES)
def test_fp32_oracle_matches_float64_autograd(case):
    """Losses and every gradient within 5e-5 of the largest entry."""
    hyper, state, batch, keeps = _first_step(case)
    o = helpers.gs_oracle_at(hyper, state, "fp32", 0)
    losses = o.train(batch, keeps)
    want_losses, want, margin = helpers.gs_f64_step(hyper, state, batch, keeps)
    for k, v in want_losses.items():
        assert abs(losses[k] - v) <= helpers.GS_GRAD_TOL * abs(v), (k, losses[k], v)
    worst = 0.0
    for g in want:
        assert o.last_grads[g].keys() == want[g].keys()
        assert abs(o.last_margin[g] - margin[g]) <= 1e-5 + 1e-3 * margin[g], (g, o.last_margin[g], margin[g])
        for k, w in want[g].items():
            ok, text, rel, _ = helpers.gs_judge_grad("fp32", o.last_grads[g][k], w)
            worst = max(worst, rel)
            assert ok, f"{case} {g}/{k}: {text}"
    print(f"IQLTEST tuned-step host {case}: fp32 oracle vs float64 autograd max {worst:.2e} of the largest entry")


# ---- (b) the seeds
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_reference_alone_stays_away_from_the_kinks(case, mode):
    for t, m in enumerate(helpers.gs_trajectory_margins(case, mode)):
        assert min(m.values()) >= 2 * helpers.GS_MARGIN, (case, mode, t, m)


@pytest.mark.parametrize("case", CASES)
def test_reference_agrees_with_its_own_restatements(case):
    assert not helpers.gs_restatements_disagree(case)


@pytest.mark.parametrize("case", [c for c in CASES if c != "h256_b512_e8_off"])  # (that one: 36 seeds at ten nets of 512 x 256)
def test_committed_seed_is_what_the_picker_returns(case):
    assert helpers.gs_pick_seed(case) == helpers.TS_CASES[case][9]


def test_picker_leaves_the_general_table_as_it_was():
    """Batch 1024 without offset biases cannot avoid a kink: seed 0, unsearched, in either table's layout."""
    assert helpers.gs_pick_seed("2x129_b1024_e8") == 0 == helpers.GS_CASES["2x129_b1024_e8"][9]
    assert helpers.gs_pick_seed((12, 5, 2, 64, 1024, 2, False, None, False, 0)) == 0


# ---- (d) what the bounds reject
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", helpers.TS_DAMAGE_CASES)
def test_bounds_reject_a_damaged_gradient(case, mode):
    hyper, ref, stale = _step2_reference(case, mode, stale=True)
    B, H = hyper["batch"], hyper["hidden"]
    assert not helpers.gs_judge_grads(mode, _copy(ref["grads"]), ref, B)[0]  # (the undamaged copy passes)
    assert all(m >= helpers.GS_MARGIN for m in ref["margin"].values())       # (and is judged under the tight bounds)
    w1, w2, b2 = (lambda d: d["q"]["q1.net.0.weight"]), (lambda d: d["q"]["q1.net.2.weight"]), (lambda d: d["q"]["q1.net.2.bias"])
    damaged = {}
    d = _copy(ref["grads"]); w2(d)[:64, :32] = 0; damaged["one 64 x 32 layer-2 tile zeroed"] = d
    d = _copy(ref["grads"]); w2(d)[16:32, 32:48] = w2(d)[16:32, 32:48].T.copy(); damaged["one 16 x 16 block transposed"] = d
    d = _copy(ref["grads"]); w1(d)[32:48] = w1(ref["grads"])[16:32]; damaged["a layer-1 strip written 16 rows off"] = d
    d = _copy(ref["grads"]); b2(d)[16:32] = b2(d)[:16]; damaged["a bias block from the neighbouring wave"] = d
    damaged["backward through step 1's weights (a stale w2ct / w3t)"] = _copy(stale)
    for what, grads in damaged.items():
        bad, lines, loose, worst, _ = helpers.gs_judge_grads(mode, grads, ref, B)
        assert bad and not loose, f"{case} {mode}: {what} passes ({worst:.2e})"
        print(f"IQLTEST tuned-step host {case} {mode}: {what}: rejected, {len(bad)} tensors, worst {worst:.2e}")
