"""The BB flavour's evaluation rolled out on the device (csrc/bb_sim.hip, custom_offline_bb.bb_run_eval_device)
against the numpy simulator bb_run_eval_IQL and the reference's record.  -m gpu.

1. k_bb_step fed the recorded actions of tests/golden/bb_train_run.npz (2 episodes, horizon 40, a run of
   the reference's own iql_bb.py): every recorded state entry, every step, and the lengths.
2. levels 9 / 10 / 11 (50 / 100 / 150 obstacles) with n_near 1 and 6 against the numpy simulator on the
   same injected actions (clamped ones, headings of exactly 0, +-90, +-180, 270, 360 among them).
3. an episode that reaches its goal: length, return and final generator state of the numpy path; steps
   queued behind the goal, and behind max_horizon, write nothing.
4. the whole path against the host path with real actors and preference transformers.
5. train(eval_on="device") against train(eval_on="host").
6. the refusals of the entry points, with nothing launched.

Tolerances.  STATE_TOL, WHOLE_STATE_TOL and the tie and goal-test margins of the seeds: tests/bb_eval_env.py.
* RETURN_TOL: measured on the host path alone (measure_return_tolerance below: the host path twice, the
  second time with every fp32 actor input moved by one ulp), ten times the largest return difference seen,
  with a floor of 1e-5 (40 summed fp32 rewards of size O(1): 40 * 2^-23 = 5e-6).  Measured on an MI355X:
  1.4e-6 / 2.4e-6 (Gaussian policy, tuned / general PT), 7.0e-7 / 8.8e-7 (deterministic); MEASURED_RETURN_DIFF
  is the largest, RETURN_TOL = 2.4e-5.  The device path itself came out bit-equal to the host path in all four
  cases of that run (returns, states and actions).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bb_env
from tests.bb_eval_env import (DEV, GOAL_BEARING, GOAL_H, GOAL_HI, GOAL_SEED, HI, LEVEL_H, LEVEL_SEED, LO, MS,
                               SENTINEL, WHOLE_CL, WHOLE_H, WHOLE_SEED, WHOLE_STATE_TOL, ConstantActor,
                               _close_states, _goal_actor, _level_actions, _pt, _train, _train_args, _whole_case,
                               bb, golden, injected, numpy_run, spied)  # (bb, golden: the module-scoped fixtures)

pytestmark = pytest.mark.gpu
MEASURED_RETURN_DIFF = 2.4e-6  # largest |return difference| of measure_return_tolerance over its four cases
RETURN_TOL = max(10 * MEASURED_RETURN_DIFF, 1e-5)


# --------------------------------------------------------------------------- #
# 1. the reference's record
# --------------------------------------------------------------------------- #
def test_step_kernel_replays_the_reference_record(golden, bb):
    H, n_ep, seed = int(golden["eval/max_horizon"]), int(golden["eval/num_episodes"]), int(golden["eval/seed"])
    mean, std = golden["stats/state_mean"], golden["stats/state_std"]
    lo, hi = golden["stats/min_actions"], golden["stats/max_actions"]
    acts = golden["eval/actions"]
    (eps, _), = injected(bb, "pair", [acts], n_ep, H, [seed], mean=mean, std=std, lo=lo, hi=hi)
    assert [e["length"] for e in eps] == [H] * n_ep and len(golden["eval/states"]) == n_ep * H  # no step left out
    want_raw, _, _ = numpy_run(bb, bb_env.ReplayActor(acts), n_ep, H, seed)
    for k, e in enumerate(eps):
        rec = golden["eval/states"][k * H:(k + 1) * H]  # the normalised state the actor saw at every step
        _close_states((e["states"][:H] - mean) / std, rec, f"episode {k} against the record")
        _close_states(e["states"], want_raw[k], f"episode {k} against the numpy simulator")
        np.testing.assert_array_equal(e["states"][:, :2], want_raw[k][:, :2])  # the agent: float32 arithmetic, exact
        np.testing.assert_array_equal(e["obs_hist"], e["states"].astype(np.float32))
        np.testing.assert_array_equal(e["act_hist"], acts[k * H:(k + 1) * H])
        np.testing.assert_array_equal(e["actor_in"], ((e["states"][H] - mean) / std).astype(np.float32))
        assert not e["done"]


# --------------------------------------------------------------------------- #
# 2. levels and envelope
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n_near", [1, 6])
def test_levels_against_the_numpy_simulator(bb, n_near):
    raw = _level_actions()
    clamped = np.clip(raw, LO, HI)
    assert (clamped != raw).any(0).all()  # both components are clamped somewhere
    want, _, want_rng = numpy_run(bb, bb_env.ReplayActor(clamped), 3, LEVEL_H, LEVEL_SEED, n_near=n_near)
    (eps, got_rng), = injected(bb, "pair", [raw], 3, LEVEL_H, [LEVEL_SEED], n_near=n_near)
    assert [e["n_obs"] for e in eps] == [150, 100, 50]
    assert [e["length"] for e in eps] == [LEVEL_H] * 3
    for k, e in enumerate(eps):
        assert e["states"].shape == (LEVEL_H + 1, 2 + 3 * n_near + 6)
        _close_states(e["states"], want[k], f"n_near {n_near}, {e['n_obs']} obstacles")
        np.testing.assert_array_equal(e["states"][:, :2], want[k][:, :2])
        np.testing.assert_array_equal(e["act_hist"], clamped[k * LEVEL_H:(k + 1) * LEVEL_H])
        np.testing.assert_array_equal(e["obs_hist"], e["states"].astype(np.float32))
    assert got_rng == want_rng


# --------------------------------------------------------------------------- #
# 3. the goal
# --------------------------------------------------------------------------- #
def test_steps_behind_the_goal_write_nothing(bb):
    action = np.array([1.0, GOAL_BEARING], np.float32)
    actor = ConstantActor(action)
    want, _, want_rng = numpy_run(bb, actor, 2, GOAL_H, GOAL_SEED)
    lengths = [len(w) - 1 for w in want]
    assert lengths[0] < GOAL_H - 5 and lengths[1] == GOAL_H  # the first episode ends at its goal, the second runs out
    (eps, got_rng), = injected(bb, "pair", [np.tile(action, (2 * GOAL_H, 1))], 2, GOAL_H, [GOAL_SEED], hi=GOAL_HI,
                               extra_steps=5, sentinel=True)
    assert [e["length"] for e in eps] == lengths and [e["done"] for e in eps] == [True, False]
    assert got_rng == want_rng
    for e, w, n in zip(eps, want, lengths):
        _close_states(e["states"][:n + 1], w, f"episode of {n} steps")
        assert (e["states"][n + 1:] == SENTINEL).all() and (e["obs_hist"][n + 1:] == SENTINEL).all()
        assert (e["act_hist"][n:] == SENTINEL).all() and (e["act_hist"][:n] == action).all()


def test_goal_episode_through_the_whole_path(bb):
    """A policy whose net puts out (1, bearing) whatever it sees: equal action bits on both paths, so equal
    lengths and states; the second episode's set-up shows that the generator was left where numpy leaves it."""
    actor = _goal_actor(bb)
    pt = _pt(bb, 26, GOAL_H, seed=3)
    with spied(bb) as host:
        want = bb.bb_run_eval_IQL(actor, 2, bb.RewardPTContext(pt, 16), MS, max_horizon=GOAL_H, context_length=16,
                                  seed=GOAL_SEED, device=DEV)
    rec = {}
    with spied(bb) as dev:
        got = bb.bb_run_eval_device(actor, 2, pt, MS, max_horizon=GOAL_H, context_length=16, seed=GOAL_SEED,
                                    device=DEV, chunk=8, record=rec)
    assert actor.training
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    lengths = [len(e) - 1 for e in host["episodes"]]
    assert [e["length"] for e in rec["episodes"]] == lengths and lengths[0] < GOAL_H - 5 and lengths[1] == GOAL_H
    for e, w in zip(rec["episodes"], host["episodes"]):
        _close_states(e["states"], np.stack(w), "goal episode")
    assert dev["rng"].bit_generator.state == host["rng"].bit_generator.state
    print("returns", got.ravel(), want.ravel())
    np.testing.assert_allclose(got, want, rtol=0, atol=RETURN_TOL)


# --------------------------------------------------------------------------- #
# 4. whole path against the host path
# --------------------------------------------------------------------------- #
class RecordingActor:
    """The host path's actor with its fp32 inputs and actions kept; ``nudge`` moves every input by one ulp."""

    def __init__(self, actor, nudge=False):
        self.actor, self.nudge, self.inputs, self.actions = actor, nudge, [], []

    def eval(self):
        self.actor.eval()

    def train(self):
        self.actor.train()

    def act(self, state, device="cpu"):
        x = np.asarray(state, np.float64).astype(np.float32)  # (what act()'s torch.tensor(..., float32) forms)
        if self.nudge:
            x = np.nextafter(x, np.float32(np.inf))
        self.inputs.append(x.copy())
        a = self.actor.act(x, device)
        self.actions.append(a.copy())
        return a


def _host_run(bb, actor, pt, mean, std, nudge=False):
    rec = RecordingActor(actor, nudge)
    with spied(bb) as seen:
        ret = bb.bb_run_eval_IQL(rec, 2, bb.RewardPTContext(pt, WHOLE_CL), MS, state_mean=mean, state_std=std,
                                 max_horizon=WHOLE_H, context_length=WHOLE_CL, seed=WHOLE_SEED, device=DEV)
    return rec, [np.stack(e) for e in seen["episodes"]], ret


def measure_return_tolerance(bb, golden):
    """The yardstick's own sensitivity: the host path twice, the second time with every fp32 actor input one
    ulp up.  Returns the largest |return difference| over the four cases (run from a script, not a test)."""
    worst = 0.0
    for policy in ("gaussian", "deterministic"):
        for general in (False, True):
            actor, pt, mean, std = _whole_case(bb, golden, policy, general)
            a = _host_run(bb, actor, pt, mean, std)[2]
            b = _host_run(bb, actor, pt, mean, std, nudge=True)[2]
            print(f"{policy} general={general}: returns {a.ravel()} nudged {b.ravel()} diff {np.abs(a - b).max():.3e}")
            worst = max(worst, float(np.abs(a - b).max()))
    return worst


@pytest.mark.parametrize("general", [False, True], ids=["tuned_pt", "general_pt"])
@pytest.mark.parametrize("policy", ["gaussian", "deterministic"])
def test_whole_path_against_the_host_path(bb, golden, policy, general):
    actor, pt, mean, std = _whole_case(bb, golden, policy, general)
    host, want_states, want = _host_run(bb, actor, pt, mean, std)
    rec = {}
    got = bb.bb_run_eval_device(actor, 2, pt, MS, state_mean=mean, state_std=std, max_horizon=WHOLE_H,
                                context_length=WHOLE_CL, seed=WHOLE_SEED, device=DEV, chunk=16, record=rec)
    assert actor.training and got.shape == want.shape == (2, 1) and got.dtype == np.float64
    assert [e["length"] for e in rec["episodes"]] == [len(w) - 1 for w in want_states]
    t0 = 0
    for e, w in zip(rec["episodes"], want_states):
        n = e["length"]
        np.testing.assert_array_equal(e["states"][0], w[0])  # the set-up: no device arithmetic in it
        _close_states(e["states"], w, f"{policy} episode of {n} steps", tol=WHOLE_STATE_TOL)
        dev_in = ((e["states"][:n] - mean) / std).astype(np.float32)
        host_in, host_act = np.stack(host.inputs[t0:t0 + n]), np.stack(host.actions[t0:t0 + n])
        same = (dev_in.view(np.uint32) == host_in.view(np.uint32)).all(1)
        print(f"{policy}: {same.sum()} of {n} actor inputs bit-equal")
        assert same[0]
        assert (e["actions"].view(np.uint32)[same] == host_act.view(np.uint32)[same]).all()
        t0 += n
    print("returns", got.ravel(), want.ravel(), "diff", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=RETURN_TOL)
    again = bb.bb_run_eval_device(actor, 2, bb.RewardPTContext(pt, WHOLE_CL), MS, state_mean=mean, state_std=std,
                                  max_horizon=WHOLE_H, context_length=WHOLE_CL, seed=WHOLE_SEED, device=DEV)
    assert again.tobytes() == got.tobytes()  # one chunk of 64 or three of 16, a context or the bare model


# --------------------------------------------------------------------------- #
# 5. train(eval_on="device")
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("K", [1, 2])
def test_train_evaluates_on_the_device(bb, golden, tmp_path, K):
    host = _train(bb, golden, "host", K, tmp_path)
    dev = _train(bb, golden, "device", K, tmp_path)
    is_loss = lambda d: "value_loss" in d
    assert [r for r in host[0] if is_loss(r[1])] == [r for r in dev[0] if is_loss(r[1])]  # bit-identical losses
    assert len([r for r in host[0] if is_loss(r[1])]) == 12 * K
    for a, b in zip(host[1], dev[1]):
        for n in a:
            assert a[n].tobytes() == b[n].tobytes(), n
    assert host[2] == dev[2]  # torch's CPU and GPU generators and numpy's global one
    h_ret = [d["evaluation_return"] for _, d in host[0] if "evaluation_return" in d]
    d_ret = [d["evaluation_return"] for _, d in dev[0] if "evaluation_return" in d]
    print("evaluation returns", h_ret, d_ret)
    assert len(h_ret) == K
    np.testing.assert_allclose(d_ret, h_ret, rtol=0, atol=RETURN_TOL)


def test_train_refuses_a_plain_callable_before_the_first_step(bb, golden):
    records = []
    with pytest.raises(TypeError, match="bb_run_eval_IQL"):
        bb.train(bb.TrainConfig(update_steps=12, eval_every=12, batch_size=bb_env.BATCH),
                 _train_args(golden), bb_env.numpy_reward, MS,
                 logger=lambda d, step: records.append(step), perm=golden["perm"], device=DEV, eval_on="device")
    assert records == []


# --------------------------------------------------------------------------- #
# 6. argument checks
# --------------------------------------------------------------------------- #
BAD = [("null state", dict(state=None), ValueError), ("null drift", dict(drift=None), ValueError),
       ("null ctl", dict(ctl=None), ValueError), ("null obs_hist", dict(obs_hist=None), ValueError),
       ("null act_hist", dict(act_hist=None), ValueError), ("null record", dict(record=None), ValueError),
       ("null actor_in", dict(actor_in=None), ValueError), ("null actor_out", dict(actor_out=None), ValueError),
       ("null mean", dict(state_mean=None), ValueError), ("null std", dict(state_std=None), ValueError),
       ("null min", dict(min_actions=None), ValueError), ("null max", dict(max_actions=None), ValueError),
       ("n_obs 0", dict(n_obs=0), NotImplementedError), ("n_obs 1025", dict(n_obs=1025), NotImplementedError),
       ("n_near 0", dict(n_near=0, state_dim=8), NotImplementedError),
       ("n_near 17", dict(n_near=17, state_dim=59), NotImplementedError),
       ("n_near > n_obs", dict(n_obs=4), NotImplementedError),
       ("state_dim", dict(state_dim=25), ValueError), ("action_dim", dict(action_dim=3), NotImplementedError),
       ("max_horizon 0", dict(max_horizon=0), ValueError)]


@pytest.mark.parametrize("what,change,error", BAD, ids=[b[0] for b in BAD])
def test_entry_points_refuse_before_any_launch(bb, what, change, error):
    from iqlpref_amd import _lib
    lib = _lib.load()
    ep = bb.DeviceEpisode(6, 8, 0, 1, LO, HI, DEV, injected=np.zeros((8, 2), np.float32))
    rng = np.random.default_rng(0)
    n_obs, *setup = bb._episode_setup(rng, 181)
    ep.load(*setup, rng.normal(0.35, 0.1, (8, n_obs)))
    buffers = (ep.record, ep.obs_hist, ep.act_hist, ep.actor_in)
    for t in buffers:
        t.fill_(SENTINEL)
    ep.ctl.copy_(torch.tensor([3, 0], dtype=torch.int32))  # (a step that were launched would write row 4)
    for name, value in change.items():
        setattr(ep.sim, name, value)
    desc, keep = bb._actor_desc(bb.DeterministicPolicy(26, 2, torch.from_numpy(HI).to(DEV), torch.from_numpy(LO).to(DEV),
                                                       hidden_dim=16).to(DEV))
    stream = _lib.stream_ptr()
    for call in (lambda: lib.iqlhip_bb_sim_reset(C.byref(ep.sim), stream),
                 lambda: lib.iqlhip_bb_sim_step(C.byref(ep.sim), stream),
                 lambda: lib.iqlhip_bb_sim_rollout(C.byref(ep.sim), C.byref(desc), 2, stream)):
        with pytest.raises(error):
            _lib.check(call())
    assert lib.iqlhip_last_error()
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in buffers) and ep.ctl.tolist() == [3, 0]


def test_null_simulator_and_rollout_arguments(bb):
    from iqlpref_amd import _lib
    lib = _lib.load()
    ep = bb.DeviceEpisode(6, 8, 0, 1, LO, HI, DEV)
    rng = np.random.default_rng(0)
    n_obs, *setup = bb._episode_setup(rng, 181)
    ep.load(*setup, rng.normal(0.35, 0.1, (8, n_obs)))
    ep.ctl.copy_(torch.tensor([3, 0], dtype=torch.int32))
    stream = _lib.stream_ptr()
    for fn in (lib.iqlhip_bb_sim_reset, lib.iqlhip_bb_sim_step):
        with pytest.raises(ValueError):
            _lib.check(fn(None, stream))
    small = bb._actor_desc(bb.DeterministicPolicy(11, 2, torch.from_numpy(HI).to(DEV), torch.from_numpy(LO).to(DEV),
                                                  hidden_dim=16).to(DEV))
    good = bb._actor_desc(bb.DeterministicPolicy(26, 2, torch.from_numpy(HI).to(DEV), torch.from_numpy(LO).to(DEV),
                                                 hidden_dim=16).to(DEV))
    with pytest.raises(ValueError):
        _lib.check(lib.iqlhip_bb_sim_rollout(C.byref(ep.sim), None, 2, stream))
    with pytest.raises(ValueError):
        _lib.check(lib.iqlhip_bb_sim_rollout(C.byref(ep.sim), C.byref(small[0]), 2, stream))  # an 11 -> 2 actor
    with pytest.raises(ValueError):
        _lib.check(lib.iqlhip_bb_sim_rollout(C.byref(ep.sim), C.byref(good[0]), 0, stream))
    torch.cuda.synchronize()
    assert ep.ctl.tolist() == [3, 0]
    with pytest.raises(TypeError, match="bb_run_eval_IQL"):
        bb.bb_run_eval_device(bb_env.ReplayActor([]), 1, _pt(bb, 26, 8, seed=1), MS, max_horizon=8, device=DEV)
