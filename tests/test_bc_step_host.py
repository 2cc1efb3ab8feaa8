"""The reference side of the behaviour-cloning tests, checked on the CPU.

a. the torch-autograd restatement of the BC step (tests/minari_cases.py), run in float64 through the whole of
   ``minari_bc``'s host pipeline -- selection, row order, state statistics, the seed's initial weights, numpy's
   index stream -- reproduces the losses the REFERENCE logged (tests/golden/minari_bc_run.npz) within the replay
   bound, and the reference's own float64 run to 1e-9: what tests/test_gpu_bc_step.py judges the kernels by is
   the reference's arithmetic;
b. the inputs of the GPU step test keep away from the relu kinks: under the float64 restatement alone at most 1 in
   1,000 (row, hidden unit) pairs has a pre-activation within 1e-5 of zero in the three steps compared (about 2 in
   100,000 are expected), so the GPU test cannot hide a failure behind the pairs it leaves out;
c. the judge rejects what a wrong kernel would produce: a zeroed 16 x 16 tile, a transposed tile, a bias block
   of the wrong wave, a mean over the padded instead of the real rows.
"""
import numpy as np
import pytest
import torch

from iqlpref_amd import minari_bc
from iqlpref_amd.iql import compute_mean_std, normalize_states
from tests import minari_cases as mc, minari_env

RTOL, ATOL = 2e-5, 2e-8  # tests/test_gpu_custom_train.py's replay bound


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load(golden_dir, "minari_bc_run.npz")


@pytest.mark.parametrize("name", ["raw", "norm"])
def test_float64_restatement_reproduces_the_references_losses(golden, name):
    g = mc.run_of(golden, name)
    common = mc.run_of(golden, "common")
    seed, B, steps = int(g["train_seed"]), int(common["batch_size"]), int(common["update_steps"])
    ds = minari_env.MinariDataset(int(common["data_seed"]))
    q = minari_bc.qlearning_dataset(ds, minari_bc.best_trajectories_ids(ds, float(common["top_fraction"]), 0.99))
    mean, std = compute_mean_std(q["observations"], eps=1e-3)
    obs = normalize_states(q["observations"], mean, std).astype(np.float32)  # (the buffer stores fp32)
    np.random.seed(seed)
    torch.manual_seed(seed)
    actor = minari_bc.Actor(45, 24, 1.0)
    p = {k: v.detach().numpy().astype(np.float64) for k, v in actor.state_dict().items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    losses = []
    for t in range(steps):
        rows = np.random.randint(0, len(obs), size=B)
        loss, grads, _ = mc.bc_forward_backward(p, obs[rows], q["actions"][rows], 1.0, torch.float64)
        losses.append(loss)
        for k in p:
            p[k], m[k], v[k] = mc.adam_step(p[k], m[k], v[k], grads[k], t + 1, torch.float64)
    want = g["rec_value"][g["rec_key"] == "actor_loss"]
    assert len(want) == steps
    np.testing.assert_allclose(losses, want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(losses, g["f64_loss"], rtol=1e-9, atol=0)
    # and the generator ended where the reference's did: the same number of draws of the same size
    np.testing.assert_array_equal(np.random.get_state()[1], g["np_key"])
    frac = np.max(g["f64_gap"] / (ATOL + RTOL * np.abs(g["f64_loss"])))
    print(f"IQLTEST bc host {name}: reference fp32 against its float64 run, largest gap {frac:.3f} of the replay bound")
    assert frac < 1


@pytest.mark.parametrize("case", list(mc.CASES))
def test_step_case_inputs_keep_away_from_the_kinks(case):
    shares, losses = mc.bc_f64_trajectory(case)
    print(f"IQLTEST bc host {case}: share of (row, unit) pairs within {mc.KINK} of zero per step {shares}, losses {losses}")
    assert all(np.isfinite(losses))  # (no poisoned row is named by an index)
    assert max(shares) <= mc.KINK_CAP
    S, A, B, max_action, params, data, idx, poison = mc.bc_case_inputs(case)
    assert not np.isin(idx[:, :B], poison).any() and np.isin(idx[:, B:], poison).all()
    assert np.all(data["observations"][poison] == mc.POISON) and {0, 1, len(data["observations"]) - 1} <= set(poison)
    assert np.abs(data["actions"][idx[:, :B]]).max() <= max_action


def _first_step(case):
    S, A, B, max_action, params, data, idx, _ = mc.bc_case_inputs(case)
    rows = idx[0, :B]
    s, a = data["observations"][rows], data["actions"][rows]
    l64, g64, _ = mc.bc_forward_backward(params, s, a, max_action, torch.float64)
    l32, g32, _ = mc.bc_forward_backward(params, s, a, max_action, torch.float32)
    return B, A, (l64, g64), (l32, g32)


def test_judge_rejects_damaged_gradients():
    """(c) On the 17-row case; the undamaged fp32 gradients pass their own bound by construction (ratio 1/4)."""
    B, A, (l64, g64), (l32, g32) = _first_step("s17_a6_b17")
    for k in g64:
        assert mc.judge(g32[k], g64[k], g32[k])[0] <= 0.25 + 1e-12
    w2 = "net.2.weight"
    d = g32[w2].copy(); d[16:32, 32:48] = 0
    assert mc.judge(d, g64[w2], g32[w2])[0] > 100
    d = g32[w2].copy(); d[:16, 16:32] = d[:16, 16:32].T.copy()
    assert mc.judge(d, g64[w2], g32[w2])[0] > 100
    b = g32["net.2.bias"].copy(); b[16:32] = b[:16]
    assert mc.judge(b, g64["net.2.bias"], g32["net.2.bias"])[0] > 100
    # the mean over the 32 padded rows instead of the 17 real ones: every gradient and the loss off by 17 / 32
    assert mc.judge(g32[w2] * (17 / 32), g64[w2], g32[w2])[0] > 100
    assert mc.judge(l32 * (17 / 32), l64, l32)[0] > 100


def test_forced_slopes_change_only_the_named_pairs():
    """The restatement with relu' forced on chosen pairs (how the GPU test measures what the pairs it leaves out
    could contribute): forcing nothing changes nothing; forcing a pair to the slope it has changes nothing."""
    S, A, B, max_action, params, data, idx, _ = mc.bc_case_inputs("s3_a1_b1")
    s, a = data["observations"][idx[0, :B]], data["actions"][idx[0, :B]]
    loss, g, zs = mc.bc_forward_backward(params, s, a, max_action, torch.float64)
    none = tuple(np.zeros(z.shape, bool) for z in zs)
    for value in (0.0, 1.0):
        l2, g2, _ = mc.bc_forward_backward(params, s, a, max_action, torch.float64, force=(*none, value))
        assert l2 == loss and all(np.array_equal(g[k], g2[k]) for k in g)
    on = tuple(z > 0 for z in zs)
    l2, g2, _ = mc.bc_forward_backward(params, s, a, max_action, torch.float64, force=(*on, 1.0))
    assert all(np.allclose(g[k], g2[k], rtol=1e-12, atol=0) for k in g)
    l2, g2, _ = mc.bc_forward_backward(params, s, a, max_action, torch.float64, force=(*on, 0.0))
    assert np.all(g2["net.0.weight"] == 0) and np.any(g2["net.4.weight"] != 0)
