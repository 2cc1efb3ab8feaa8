"""iqlhip_forward (ImplicitQLearning.forward "q" | "v" | "actor" | "q_target") over the envelope
include/iqlhip.h states, against plain CPU references on the trainer's own parameters.  -m gpu.

Which kernel a case enters: n_hidden = 2 with hidden_dim 64 / 128 / 256 runs k_infer<BF16, H>
(csrc/iql_step.hip, "tuned"); every other depth / width runs kd_infer<BF16> (csrc/iql_deep.hip, "general").
Both stage their input into LDS themselves, guard the last rows of the store and loop over the critics,
critic e into column e of out[n][E]; none of it is entered by a training step.

References and bounds (none is fitted to what the kernels give):
  fp32  helpers.mlp_forward_ref in fp64.  The project's 2e-5 (rtol = atol) for nets of up to four Linear
        layers and width <= 256; deeper or wider: max(4 x gap, 2e-5) absolute, gap = the largest difference
        between an fp32 numpy forward of the same net on the same rows (another valid fp32 summation order)
        and the fp64 one.
  bf16  the oracle's autocast restatement (oracle/iql_oracle.py: critics_all, value_forward, policy_forward;
        fp32 sums).  Two correct bf16 forwards differ where a rounding tie flips: the yardstick is what the
        oracle and helpers.mlp_forward_bf16_f64 (same operands, fp64 sums) differ by on the case's rows.
        max |err|    <= max(4 x the largest gap, 2 bf16 ulps of the largest |reference output|): one flip
                        at the output rounding, one propagated;
        median |err| <= max(4 x the median gap, a quarter ulp at the median |reference output|): what a
                        wrong tile, head or column cannot meet.
Every test prints its figures (-s); the docstrings hold what an MI355X gave."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
N_ROWS = 100    # six full 16-row slabs and one of four rows
B = 16          # the smallest batch a trainer takes: a forward does not depend on it
MODES = ("fp32", "bf16")
WHICH = ("q", "v", "actor", "q_target")
SENTINEL = -12345.0
FORCED = bool(os.environ.get("IQLHIP_FORCE_GENERAL"))  # (set: every shape through the general kernel)


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _build(gh, mode, S, A, H, NH=2, E=2, det=False, dropout=None, kind="tuned"):
    """A trainer on forward_nets' weights (loaded through the modules' state_dicts) and N_ROWS input rows."""
    rng = np.random.default_rng([S, A, H, NH, E])
    nets = helpers.forward_nets(rng, S, A, H, NH, E, det, dropout)
    hyper = dict(s_dim=S, a_dim=A, hidden=H, n_hidden=NH, n_critics=E, deterministic=det, dropout=dropout,
                 iql_tau=0.7, beta=3.0, max_steps=1000, discount=0.99, tau=0.005, n_rows=64)
    tr = gh.make_trainer(hyper, nets, mode, seed=11)
    assert tr.step_kind(B) == ("general" if FORCED else kind)
    for mod, want in zip((tr.qf, tr.vf, tr.actor, tr.q_target), nets + (nets[0],)):
        have = gh.module_params(mod)
        assert have.keys() == want.keys() and all(np.array_equal(have[k], want[k]) for k in want)
    s = rng.standard_normal((N_ROWS, S)).astype(np.float32)
    a = rng.uniform(-1, 1, (N_ROWS, A)).astype(np.float32)
    return tr, hyper, s, a


def _forward_all(tr, ts, ta):
    return {w: tr.forward(w, ts, ta if w in ("q", "q_target") else None).cpu().numpy() for w in WHICH}


def _reference(gh, tr, mode, s, a):
    """helpers.forward_reference on the trainer's CURRENT parameters (the modules' and q_target's state_dicts)."""
    return helpers.forward_reference(tuple(gh.module_params(m) for m in (tr.qf, tr.vf, tr.actor, tr.q_target)), mode, s, a)


_judge = helpers.forward_judge  # (the bounds of the module docstring)


def _check(mode, got, ref, n_lin, width, label, rows=None):
    for which in WHICH:
        want, gap = ref[which] if rows is None else (ref[which][0][:rows], ref[which][1][:rows])
        ok, text = _judge(mode, got[which], want, gap, n_lin, width)
        print(f"FWD {label} {mode} {which}: {text}")
        assert ok, f"{label} {mode} {which}: {text}"


def _fresh_case(gh, mode, S, A, H, NH=2, kind="tuned", label="", **kw):
    """Build, run the four forwards on N_ROWS rows, compare; before any step the target equals q bit for bit."""
    tr, hyper, s, a = _build(gh, mode, S, A, H, NH, kind=kind, **kw)
    got = _forward_all(tr, _up(s), _up(a))
    ref = _reference(gh, tr, mode, s, a)
    _check(mode, got, ref, NH + 1, max(H, S + A), f"{label} S{S} A{A} {NH}x{H}")
    np.testing.assert_array_equal(_bits(got["q_target"]), _bits(got["q"]))
    q = got["q"]
    assert all(not np.array_equal(q[:, e], q[:, f]) for e in range(q.shape[1]) for f in range(e))  # critics differ
    return tr, hyper, s, a, got, ref


# ---- 1. the tuned kernel in every instantiation
TUNED_SHAPES = {
    "s17a6": (17, 6),
    "s100a28_input_limit": (100, 28),     # S + A = 128: the widest input
    "s20a32_two_output_tiles": (20, 32),  # A = 32: the second 16-column output tile
    "s3a1": (3, 1),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H", (64, 128, 256))
@pytest.mark.parametrize("shape", TUNED_SHAPES)
def test_tuned_kernel_every_instantiation(gh, shape, H, mode):
    """k_infer<fp32 | bf16, 64 | 128 | 256>; at H = 256 the layer-2 weights arrive in chunks.
    Observed on an MI355X (over the cases; bf16 per output array): fp32 max |err| 6.7e-7 (fp32 numpy vs fp64: 6.0e-7).
    bf16: 44 of the 48 output arrays bit-identical to the oracle, the others in >= 0.990 of their elements; max |err|
    1.95e-3 = a quarter of its bound, where the CPU pair differs by the same 1.95e-3; median 0 in every array."""
    _fresh_case(gh, mode, *TUNED_SHAPES[shape], H, label="tuned")


# ---- 2. input widths around the MFMA K step (Prec::KM: 16 in fp32, 32 in bf16).  V and the actor take S
# columns of a descriptor sized for S + A: their first layer is padded to less than the critics'
INPUT_WIDTHS = {f"s{S}a4": (S, 4) for S in (11, 12, 13, 27, 28, 29)}        # S + A = 15, 16, 17, 31, 32, 33
INPUT_WIDTHS.update({f"s{S}a4_s_boundary": (S, 4) for S in (16, 17, 32, 33)})
INPUT_KERNELS = {"tuned_h64": (2, 64, "tuned"), "general_2x48": (2, 48, "general")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", INPUT_KERNELS)
@pytest.mark.parametrize("shape", INPUT_WIDTHS)
def test_input_width_boundaries(gh, shape, kernel, mode):
    """Observed on an MI355X: fp32 max |err| 4.1e-7 (fp32 numpy vs fp64: 3.7e-7).  bf16: 78 of the 80 output
    arrays bit-identical to the oracle, the other two in 0.995 of their elements (1.5e-8 on an output next to zero,
    as in the CPU pair); median 0 in every array."""
    NH, H, kind = INPUT_KERNELS[kernel]
    _fresh_case(gh, mode, *INPUT_WIDTHS[shape], H, NH, kind=kind, label=kernel)


# ---- 3. the general kernel over depth 1..6 and width 1..1024
GENERAL_SHAPES = {
    "1x1": (1, 1), "1x15": (1, 15), "2x17": (2, 17), "3x96": (3, 96), "6x24": (6, 24),
    "1x1000": (1, 1000), "2x1024": (2, 1024),  # the envelope's end: 128.5 KiB of LDS rows in fp32
    "6x256": (6, 256), "2x257": (2, 257),
    "2x256_forced": (2, 256),                  # the tuned step's own shape: IQLHIP_FORCE_GENERAL only
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", GENERAL_SHAPES)
def test_general_kernel_depth_and_width(gh, shape, mode):
    """No shape of the table is refused in either precision (deep_shape_ok takes 1..6 x 1..1024, as
    include/iqlhip.h and iql_deep.h state).  Observed on an MI355X: fp32 max |err| 9.3e-7 at 2 x 1024 (fp32 numpy vs
    fp64: 5.8e-7; the derived bound is its floor, 2e-5).  bf16: 33 of the 36 output arrays bit-identical to the
    oracle, the others in >= 0.995 of their elements; max |err| 2.4e-4 = 1/64 of its bound; median 0 in every array."""
    NH, H = GENERAL_SHAPES[shape]
    if (NH, H) == (2, 256) and not FORCED:
        pytest.skip("the tuned kernel takes this shape")
    _fresh_case(gh, mode, 17, 6, H, NH, kind="general", label="general")


# ---- 4. critic ensembles: column e is critic e
ENSEMBLE_KERNELS = {"tuned_h128": (2, 128, "tuned"), "general_3x40": (3, 40, "general")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", (2, 3, 8))
@pytest.mark.parametrize("kernel", ENSEMBLE_KERNELS)
def test_critic_ensembles(gh, kernel, E, mode):
    """_reference computes column e from critic e's parameters alone; no other assignment of columns to
    critics passes the same bounds.  Observed on an MI355X: fp32 max |err| 3.8e-7; bf16: 23 of the 24 output arrays
    bit-identical to the oracle, the other in 0.990 of its elements (9.8e-4 = 1/16 of its bound, as in the CPU pair);
    median 0 in every array."""
    NH, H, kind = ENSEMBLE_KERNELS[kernel]
    tr, hyper, s, a, got, ref = _fresh_case(gh, mode, 17, 6, H, NH, kind=kind, E=E, label=f"{kernel} E{E}")
    for which in ("q", "q_target"):
        want, gap = ref[which]
        assert got[which].shape == (N_ROWS, E)
        for e in range(E):
            for f in range(E):
                ok, text = _judge(mode, got[which][:, [e]], want[:, [f]], gap[:, [f]], NH + 1, H)
                assert ok == (e == f), f"{which} column {e} against critic {f}: {text}"


# ---- 5. row counts around the 16-row slab
ROW_COUNTS = (1, 15, 16, 17, 33, 100)
ROW_KERNELS = {"tuned_h128": (2, 128, "tuned"), "general_3x40": (3, 40, "general")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", ROW_KERNELS)
def test_row_counts(gh, kernel, mode):
    """Every n against the reference (bounds from its own rows), and bit-identical to rows [:n] of the
    100-row call: a row's value does not depend on how full its slab is.  Observed on an MI355X:
    fp32 max |err| 2.5e-7; bf16: 46 of the 48 output arrays bit-identical to the oracle, the others in >= 0.97 of
    their elements (one of the 33 at n = 33; 9.8e-4 = 1/8 of its bound, as in the CPU pair); median 0 in every array."""
    NH, H, kind = ROW_KERNELS[kernel]
    tr, hyper, s, a, full, ref = _fresh_case(gh, mode, 17, 6, H, NH, kind=kind, label=kernel)
    ts, ta = _up(s), _up(a)
    for n in ROW_COUNTS:
        got = _forward_all(tr, ts[:n], ta[:n])
        for which in WHICH:
            assert got[which].shape == (n, full[which].shape[1])
            np.testing.assert_array_equal(_bits(got[which]), _bits(full[which][:n]), err_msg=f"{which} n={n}")
        _check(mode, got, ref, NH + 1, H, f"{kernel} n={n}", rows=n)


# ---- 6. rows beyond n are not written: only a C caller can hand over a larger buffer
def _c_forward(tr, which, ts, ta, n, out):
    from iqlpref_amd import _lib
    rc = _lib.load().iqlhip_forward(tr._handle, which, _lib.ptr(ts), _lib.ptr(ta), n, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", ROW_KERNELS)
def test_rows_beyond_n_are_not_written(gh, kernel, mode):
    NH, H, kind = ROW_KERNELS[kernel]
    tr, hyper, s, a = _build(gh, mode, 17, 6, H, NH, kind=kind)
    ts, ta = _up(s), _up(a)
    widths = {"q": 2, "v": 1, "actor": 6, "q_target": 2}
    for n in (1, 17):
        for i, which in enumerate(WHICH):
            # (the larger buffer first: a store beyond n shows here, inside an allocation that holds it)
            out = torch.full((n + 20, widths[which]), SENTINEL, dtype=torch.float32, device="cuda:0")
            assert _c_forward(tr, i, ts[:n + 20].contiguous(), ta[:n + 20].contiguous() if i in (0, 3) else None, n, out) == 0
            got = out.cpu().numpy()
            assert np.all(got[n:] == np.float32(SENTINEL)), f"{which} n={n}: rows beyond n were written"
            want = tr.forward(which, ts[:n], ta[:n] if i in (0, 3) else None).cpu().numpy()
            assert want.shape == (n, widths[which])
            np.testing.assert_array_equal(_bits(got[:n]), _bits(want), err_msg=f"{which} n={n}")


# ---- 7. the actor runs in eval mode
EVAL_KERNELS = {"tuned_h256": (2, 256, "tuned"), "general_3x100": (3, 100, "general")}


def _buffer(gh, hyper):
    data = helpers.synth_dataset(np.random.default_rng(5), hyper["n_rows"], hyper["s_dim"], hyper["a_dim"])
    data["terminals"] = data["terminals"].astype(np.float32)
    return gh.make_buffer(hyper, data)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("det", (False, True), ids=("gaussian", "deterministic"))
@pytest.mark.parametrize("kernel", EVAL_KERNELS)
def test_actor_forward_is_eval_mode(gh, kernel, det, mode):
    """Trainers built with dropout = 0.1: forward("actor") is the reference WITHOUT masks and the same bits
    on every call, before and after training steps that drew Philox masks.  Observed on an MI355X:
    fp32 max |err| 5.2e-7; bf16: 31 of the 32 output arrays bit-identical to the oracle, the other in 0.998 of its
    elements (2.4e-7 on an output next to zero); median 0 in every array."""
    NH, H, kind = EVAL_KERNELS[kernel]
    tr, hyper, s, a, first, _ = _fresh_case(gh, mode, 17, 6, H, NH, kind=kind, det=det, dropout=0.1,
                                            label=f"{kernel} dropout det={det}")
    ts, ta = _up(s), _up(a)
    again = _forward_all(tr, ts, ta)
    for which in WHICH:
        np.testing.assert_array_equal(_bits(again[which]), _bits(first[which]), err_msg=which)
    tr.train_steps(_buffer(gh, hyper), 3, B)
    after = _forward_all(tr, ts, ta)
    _check(mode, after, _reference(gh, tr, mode, s, a), NH + 1, H, f"{kernel} dropout det={det} after 3 steps")
    assert not np.array_equal(after["actor"], first["actor"])  # (the weights moved)
    again = _forward_all(tr, ts, ta)
    for which in WHICH:
        np.testing.assert_array_equal(_bits(again[which]), _bits(after[which]), err_msg=which)


# ---- 8. live weights: the compute copies that the update kernels write are what the forward reads
LIVE_KERNELS = {"tuned_h128": (2, 128, "tuned"), "general_3x40": (3, 40, "general")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", LIVE_KERNELS)
def test_forward_reads_the_live_weights(gh, kernel, mode):
    """After 5 train_steps every output matches the reference on the CURRENT state_dicts, q_target's
    included, and the target has left q; load_state_dict of the initial checkpoint brings the initial
    outputs back bit for bit.  Observed on an MI355X: after the steps fp32 max |err| 5.1e-7; bf16: all 8 output arrays
    bit-identical to the oracle on the trained weights."""
    NH, H, kind = LIVE_KERNELS[kernel]
    tr, hyper, s, a, first, _ = _fresh_case(gh, mode, 17, 6, H, NH, kind=kind, label=kernel)
    ts, ta = _up(s), _up(a)
    ckpt = copy.deepcopy(tr.state_dict())
    tr.train_steps(_buffer(gh, hyper), 5, B)
    assert tr.total_it == 5
    after = _forward_all(tr, ts, ta)
    _check(mode, after, _reference(gh, tr, mode, s, a), NH + 1, H, f"{kernel} after 5 steps")
    for which in WHICH:
        assert not np.array_equal(after[which], first[which]), which
    assert not np.array_equal(after["q_target"], after["q"])
    tr.load_state_dict(ckpt)
    back = _forward_all(tr, ts, ta)
    for which in WHICH:
        np.testing.assert_array_equal(_bits(back[which]), _bits(first[which]), err_msg=which)


# ---- 9. what the entry point refuses
@pytest.mark.parametrize("kernel", ROW_KERNELS)
def test_what_the_entry_point_refuses(gh, kernel):
    """IQLHIP_ERR_INVALID (ValueError through the binding), and out keeps what it held."""
    from iqlpref_amd import _lib
    NH, H, kind = ROW_KERNELS[kernel]
    tr, hyper, s, a = _build(gh, "bf16", 17, 6, H, NH, kind=kind)
    ts, ta = _up(s), _up(a)
    out = torch.full((N_ROWS, 6), SENTINEL, dtype=torch.float32, device="cuda:0")
    refused = [(0, ts, ta, 0, out), (1, ts, ta, -1, out),              # n = 0, n < 0
               (-1, ts, ta, 4, out), (4, ts, ta, 4, out),              # which outside 0..3
               (0, ts, None, 4, out), (3, ts, None, 4, out),           # critics without actions
               (1, None, ta, 4, out), (2, ts, ta, 4, None)]            # null s, null out
    for which, s_, a_, n, out_ in refused:
        rc = _c_forward(tr, which, s_, a_, n, out_)
        assert rc == _lib.ERR_INVALID, (which, n, rc)
        with pytest.raises(ValueError):
            _lib.check(rc)
        assert bool(torch.all(out == SENTINEL))
    assert _c_forward(tr, 2, ts, None, 4, out) == 0  # (and the same handle still works)
    assert bool(torch.all(out.view(-1)[:24] != SENTINEL)) and bool(torch.all(out.view(-1)[24:] == SENTINEL))
