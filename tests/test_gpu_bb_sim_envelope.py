"""The BB simulator kernels (csrc/bb_sim.hip: k_bb_step, k_bb_episodes) over their whole stated envelope: n_obs
1..1024, n_near 1..min(16, n_obs), actors of 1..8 layers and widths 1..256, groups of 16.  -m gpu.  Cases, set-ups,
the reference loop and the driver are tests/bb_envelope.py; what the comparisons rest on (the reference is the loop
of bb_run_eval_IQL, the margins of every set-up) is asserted on the CPU by tests/test_bb_envelope_host.py.

1. the envelope on injected tables, (n_obs, n_near) = (1, 1) (2, 2) (16, 16) (17, 16) (255, 6) (256, 16) (257, 1)
   (1024, 16) (1024, 1), 12 steps, launch pair and fused: every observation row and the final x, y, heading of ALL
   obstacles (the float64 isclose windows, the mirrored re-entries, the strided loops) within STATE_TOL of
   ``reference_run``; the agent, the clamped actions, the fp32 history and the next actor input bit for bit; the
   two rollouts bit-equal; nothing written behind the last obstacle of ``state``;
2. numpy's float32 sine and cosine: 4,560 one-step episodes from (0, 0) at speed 1, row 1 = (cos, sin) of the
   heading with nothing added, bit for bit against ``_cos_deg`` / ``_sin_deg`` on the float32 scalar -- the fused
   kernel in groups of 16, 256 of the headings (the window edges among them) through the launch pair as well;
3. the goal test: interior hit, u clamped to 1 and to 0 (hit and miss each), a hit by isclose alone and a miss just
   outside its window, u = NaN (speed 0) hit and miss; nothing is written behind the goal, by either rollout;
4. the fused forward at its edges (n_layers 1 and 8, widths 1 / 17 / 37 / 255 / 256 / 100, S = 11 / 26 / 56, tanh
   hidden layers, no output activation) against ONE iqlhip_mlp_forward call over the rows the run recorded, bit for
   bit; and the simulator under it against ``reference_run`` on the actions the run recorded;
5. one launch of 16 members of mixed n_obs / n_near / S / actors, and the same in reverse order: every buffer of
   every member bit-equal to its solo launch.

Tolerances: STATE_TOL = 1e-9 of tests/bb_eval_env.py (derived there for 500 steps; these run 12) wherever a
float64 state is compared with numpy; everything else bit for bit.  Margins of the inputs: the header of
tests/bb_envelope.py.

Recorded from the run on an MI355X (numpy 2.2.6 there as on the CPU host: no heading is decided differently).
Largest state error / STATE_TOL, launch pair = fused, and the re-entries the reference counts (the final x, y of all
obstacles agree, so the device took the same ones):
    case 1  (1, 1) (2, 2) (16, 16) (17, 16): 0, re-entries 0 / 0 / 1 / 1;  (255, 6) 7.1e-6, 85;  (256, 16) 1.8e-6, 87;
            (257, 1) 0, 90;  (1024, 16) 7.1e-6, 377;  (1024, 1) 7.1e-6, 377
    case 2  4,560 headings through the fused kernel and 256 through the launch pair, 0 differ
    case 3  0 on all nine goals
    case 4  direct 2.2e-7 / 0 (6 / 6 re-entries);  1: 3.6e-6 / 7.1e-6 (108 / 106);  17 x 37: 0 / 0 (20 / 19);
            255 x 256 x 100: 0 / 3.6e-6 (48 / 50);  48 x 7: 0 / 0 (1 / 1);  256 x 256: 7.1e-6 / 3.6e-6 (377 / 371)
The module takes 3 s; no test more than 0.4 s.

What the cases notice, tried once with the kernel changed on purpose: without the 270 degree window of
cos_deg_f64 every case from 16 obstacles on misses STATE_TOL by five decades (1.4e-4); with one coefficient of
np_trig_f32's cosine polynomial off by one bit 35 of the 4,560 headings differ, while the 12-step cases mostly
do not notice; without the clamp u > 1 the goals (3, 0) and (2.30002, 0) are touched; with a tanh on every
output layer the 17 x 37 actor's actions differ; with the ranking loop stopped at 256 entries the cases of 300
and 1024 obstacles are off by hundreds and a group no longer equals its members alone.
"""
import numpy as np
import pytest
import torch

from tests import bb_envelope as B

pytestmark = pytest.mark.gpu
E = B.E
DEV, SENTINEL, STATE_TOL, H = E.DEV, E.SENTINEL, E.STATE_TOL, B.H
bb = E.bb  # (the module-scoped fixture)
BUFFERS = ("states", "obs_hist", "act_hist", "actor_in")


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _judge(got, ref, m, what):
    """One device rollout that ran to its horizon against the reference loop."""
    s, n = m["setup"], m["setup"]["n_obs"]
    rows, state = got["states"], got["sim_state"]
    horizon = len(s["drift"])
    assert (got["length"], got["done"], got["ctl"]) == (horizon, False, [horizon, 0]) == (ref["length"], ref["done"],
                                                                                         [horizon, 0]), what
    assert rows.shape == ref["rows"].shape and state.shape == (8 + 3 * (n + 1),)
    err = max(np.abs(rows - ref["rows"]).max(), np.abs(state[8:8 + n] - ref["ox"]).max(),
              np.abs(state[8 + n:8 + 2 * n] - ref["oy"]).max())
    print(f"{what}: max |state error| {err:.3e} = {err / STATE_TOL:.2e} STATE_TOL, "
          f"{ref['margins']['reentries']} re-entries")
    assert err <= STATE_TOL, what
    _same_bits(state[8 + 2 * n:8 + 3 * n], ref["oang"], f"{what}: headings")
    assert (state[8 + 3 * n:] == SENTINEL).all(), f"{what}: written behind the last obstacle"
    _same_bits(state[:8], np.concatenate([ref["rows"][-1, :2], s["goal"], np.asarray(s["tail"], np.float64)]), what)
    _same_bits(rows[:, :2], ref["rows"][:, :2], f"{what}: the agent")
    _same_bits(got["act_hist"], ref["actions"], f"{what}: act_hist")
    _same_bits(got["obs_hist"], rows.astype(np.float32), f"{what}: obs_hist")
    _same_bits(got["actor_in"], ((rows[-1] - m["mean"]) / m["std"]).astype(np.float32), f"{what}: actor_in")


def _rollouts_equal(a, b, what):
    for name in BUFFERS + ("sim_state",):
        _same_bits(a[name], b[name], f"{what}: {name}")
    assert a["ctl"] == b["ctl"] and (a["length"], a["done"]) == (b["length"], b["done"]), what


# --------------------------------------------------------------------------- #
# 1. the envelope on injected tables
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", B.ENVELOPE, ids=B.case_id)
def test_envelope_on_injected_tables(bb, case):
    m = B.table_member(*case)
    ref = B.member_reference(bb, m)
    pair, = B.device_run(bb, "pair", [m], extra_steps=2)  # (the two behind max_horizon write nothing)
    fused, = B.device_run(bb, "fused", [m])
    _judge(pair, ref, m, f"{B.case_id(case)}, launch pair")
    _judge(fused, ref, m, f"{B.case_id(case)}, fused")
    _rollouts_equal(fused, pair, B.case_id(case))


# --------------------------------------------------------------------------- #
# 2. numpy's float32 sine and cosine
# --------------------------------------------------------------------------- #
def _trig_sweep(bb, headings, K):
    """Row 1, columns 0 and 1 of one one-step episode per heading, K per launch (K = 1: the launch pair) on ONE set
    of buffers: the K states, tables and records are the rows of three tensors, restored by one copy per launch."""
    s = B.trig_setup()
    n = len(headings)
    assert n % K == 0
    eps = [bb.DeviceEpisode(1, 1, 0, 1, B.TRIG_LO, B.TRIG_HI, DEV, n_obs_max=1, injected=np.zeros((1, 2), np.float32))
           for _ in range(K)]
    states = torch.zeros((K, 11), dtype=torch.float64, device=DEV)
    tables = torch.zeros((K, 1, 2), dtype=torch.float32, device=DEV)
    records = torch.full((K, 2, 11), SENTINEL, dtype=torch.float64, device=DEV)
    for k, ep in enumerate(eps):  # (load() builds the struct from them)
        ep.state, ep.injected, ep.record = states[k], tables[k], records[k]
    fused = bb.FusedEpisodes(eps) if K > 1 else None
    for ep in eps:
        ep.load(s["ox"], s["oy"], s["oang"], s["px"], s["py"], s["goal"], s["tail"], s["drift"])
    start = states.clone()
    actions = np.stack([np.ones(n, np.float32), headings], 1).reshape(n // K, K, 1, 2)
    actions = torch.from_numpy(actions).to(DEV)
    got = torch.full((n // K, K, 2), SENTINEL, dtype=torch.float64, device=DEV)
    ctl = torch.full((n // K, K, 2), -1, dtype=torch.int32, device=DEV)
    for g in range(n // K):
        states.copy_(start)
        tables.copy_(actions[g])
        if fused is not None:
            fused.run([None] * K)
            ctl[g].copy_(fused.ctl)
        else:
            eps[0].reset()
            eps[0].step()
            ctl[g, 0].copy_(eps[0].ctl)
        got[g].copy_(records[:, 1, :2])
    assert (ctl.cpu().numpy() == [1, 0]).all()
    _same_bits(records[:, 0].cpu().numpy(), np.tile(np.concatenate([[0.0, 0.0, 10.0, -10.0, 45.0, 40.0, 0.0],
                                                                    B.TAIL]), (K, 1)), "row 0")
    return got.cpu().numpy().reshape(n, 2)


def _trig_compare(got, want, headings, what):
    bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).any(1))
    print(f"{what}: {len(headings)} headings compared, {len(bad)} differ (numpy {np.__version__})")
    for i in bad[:20]:
        print(f"  heading {float(headings[i])!r}: kernel {got[i].tolist()}, numpy {want[i].tolist()}")
    assert len(bad) == 0, what


def test_agent_move_is_numpys_float32_sine_and_cosine(bb):
    headings = B.trig_headings()
    want = B.trig_expected(bb, headings)
    _trig_compare(_trig_sweep(bb, headings, 16), want, headings, "fused, 16 episodes per launch")
    sub = np.concatenate([np.arange(len(headings) - 104, len(headings)), np.arange(0, len(headings) - 104, 29)[:152]])
    assert len(sub) == 256
    _trig_compare(_trig_sweep(bb, headings[sub], 1), want[sub], headings[sub], "launch pair")


# --------------------------------------------------------------------------- #
# 3. the goal test
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("i", range(len(B.GOALS)), ids=[f"{g[0][0]}_{g[0][1]}_speed{g[1]}" for g in B.GOALS])
def test_goal_test_on_every_branch(bb, i):
    goal, speed, hit = B.GOALS[i]
    s = B.goal_setup(i)
    mean, std = B.stats(i, 1)
    m = {"setup": s, "n_near": 1, "mean": mean, "std": std}
    ref = B.member_reference(bb, m)
    assert (ref["length"], ref["done"]) == ((1, True) if hit else (B.GOAL_ROWS, False))
    pair, = B.device_run(bb, "pair", [m], extra_steps=2)  # (queued behind the goal, or behind max_horizon)
    fused, = B.device_run(bb, "fused", [m])
    _rollouts_equal(fused, pair, f"goal {goal}")
    for what, got in (("launch pair", pair), ("fused", fused)):
        n = ref["length"]
        assert got["ctl"] == [n, int(hit)] and (got["length"], got["done"]) == (n, hit), (what, goal)
        E._close_states(got["states"][:n + 1], ref["rows"], f"goal {goal}, {what}")
        _same_bits(got["states"][:n + 1, :2], ref["rows"][:, :2], what)
        _same_bits(got["act_hist"][:n], ref["actions"], what)
        assert (got["states"][n + 1:] == SENTINEL).all() and (got["obs_hist"][n + 1:] == SENTINEL).all(), what
        assert (got["act_hist"][n:] == SENTINEL).all(), what
        assert not (got["states"][:n + 1] == SENTINEL).any()
        _same_bits(got["obs_hist"][:n + 1], got["states"][:n + 1].astype(np.float32), what)
        _same_bits(got["actor_in"], ((got["states"][n] - mean) / std).astype(np.float32), what)


# --------------------------------------------------------------------------- #
# 4. the fused forward at its edges
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", B.FORWARD, ids=B.forward_id)
def test_fused_forward_at_its_edges(bb, case):
    from iqlpref_amd.iql import mlp_forward_f32
    members = B.forward_members(bb, case)
    runs = [B.device_run(bb, "fused", [m])[0] for m in members]
    actor = members[0]["actor"]
    net = actor.net
    assert len(net.linears()) == len(case[2]) + 1 and net._hidden_act == int(case[3] == "tanh")
    assert net._out_act == int(case[4] == "tanh")
    for e, (m, got) in enumerate(zip(members, runs)):
        assert (got["length"], got["done"], got["ctl"]) == (H, False, [H, 0])  # every step of both is compared
        # the simulator under the forward: the reference loop on the actions this run recorded
        s = m["setup"]
        ref = B.reference_run(bb, s, got["act_hist"], s["drift"], m["n_near"], m["mean"], m["std"])
        _judge(got, ref, m, f"{B.forward_id(case)}, episode {e}")
    # the kernel forms the input in float64 and rounds once
    rows = np.concatenate([((g["states"][:H] - m["mean"]) / m["std"]).astype(np.float32)
                           for m, g in zip(members, runs)])
    lin = net.linears()
    raw = mlp_forward_f32([l.weight for l in lin], [l.bias for l in lin], torch.from_numpy(rows).to(DEV),
                          w_in_out=False, hidden_act=net._hidden_act, out_act=net._out_act)
    want = torch.clamp(raw, torch.from_numpy(B.LO).to(DEV), torch.from_numpy(B.HI).to(DEV)).cpu().numpy()
    got = np.concatenate([g["act_hist"] for g in runs])
    assert len(np.unique(got, axis=0)) > H // 2  # (not a constant policy)
    _same_bits(got, want, "actions")


# --------------------------------------------------------------------------- #
# 5. groups
# --------------------------------------------------------------------------- #
def test_group_of_16_mixed_members_equals_their_solo_launches(bb):
    members = B.group_members(bb)
    assert len(members) == 16
    solo = [B.device_run(bb, "fused", [m])[0] for m in members]
    group = B.device_run(bb, "fused", members)
    backwards = B.device_run(bb, "fused", members[::-1])[::-1]
    for k, m in enumerate(members):
        what = f"member {k} ({m['setup']['n_obs']} obstacles, n_near {m['n_near']}, {'actor' if 'actor' in m else 'table'})"
        assert solo[k]["ctl"] == [H, 0], what
        _rollouts_equal(group[k], solo[k], what)
        _rollouts_equal(backwards[k], solo[k], what + ", reverse order")
    assert len({g["states"].tobytes() for g in group}) == 16  # the group did not hand one result to all
