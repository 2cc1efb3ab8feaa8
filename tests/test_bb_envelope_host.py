"""Host side of tests/test_gpu_bb_sim_envelope.py (no GPU): what its comparisons rest on, asserted on the
reference alone.

1. ``bb_envelope.reference_run`` is the step loop of ``bb_run_eval_IQL``: with ``_episode_setup`` handing out the
   same set-up and a ReplayActor on the clamped actions, every observation the evaluation forms equals the loop's
   rows bit for bit (three cases of the table, n_obs 17 / 257 / 1024).
2. The conditions on the inputs, for every episode of cases 1, 4 and 5 (a decision taken the other way is another
   trajectory, not an error of 1e-9): nearest-obstacle gap >= 1e-4, rim margin >= 1e-4, goal margin >= 1, at least
   one re-entry from 16 obstacles on and 50 from 255 on, every special heading that fits is present, an obstacle
   inside a window has not moved along that axis after 12 steps and one just outside has, by more than 1e-7;
   the last obstacle of a set-up of more than 17 is the nearest one of the first observation.
   Case 4's margins are taken with an fp32 torch restatement of its actors.
3. The nine goals of case 3 are decided as the issue states them, the sixth by ``isclose`` alone (d2 > 1.69).
4. The headings of case 2: at least 4,096, float32, the 104 neighbours of the window edges among them, on which
   the rule csrc/bb_sim.hip states for ``isclose_f32`` agrees with ``np.isclose(float32, int)``.
5. Every actor of case 4 is inside ``bb_actor_check``'s envelope, with n_layers 1 and 8 and widths 1 and 256
   among them; the group of case 5 has 16 members of mixed shapes.
"""
import ctypes as C

import numpy as np
import pytest

from tests import bb_env
from tests import bb_envelope as B

bb = B.E.bb  # (the module-scoped fixture)


def _episodes(bb):
    """(name, member) of every episode of cases 1, 4 and 5."""
    out = [(B.case_id(c), B.table_member(*c)) for c in B.ENVELOPE + B.GROUP_EXTRA]
    for c in B.FORWARD:
        out += [(f"{B.forward_id(c)}, episode {e}", m) for e, m in enumerate(B.forward_members(bb, c))]
    return out


@pytest.mark.parametrize("case", [c for c in B.ENVELOPE if c[0] in (17, 257) or c[:2] == (1024, 16)], ids=B.case_id)
def test_reference_loop_is_the_loop_of_bb_run_eval_IQL(bb, monkeypatch, case):
    n_obs, n_near, _ = case
    m = B.table_member(*case)
    s = m["setup"]
    ref = B.member_reference(bb, m)
    assert ref["length"] == B.H and not ref["done"] and ref["rows"].shape == (B.H + 1, 8 + 3 * n_near)
    seen = []
    real_observe = bb._observe
    monkeypatch.setattr(bb, "_episode_setup", lambda rng, days: (
        n_obs, s["ox"].copy(), s["oy"].copy(), s["oang"].copy(), s["px"], s["py"], s["goal"], s["tail"]))
    monkeypatch.setattr(bb, "_observe", lambda *a: (seen.append(real_observe(*a)), seen[-1])[1])
    actor = bb_env.ReplayActor(np.clip(s["actions"], B.LO, B.HI))
    bb.bb_run_eval_IQL(actor, 1, bb_env.numpy_reward, B.MS, state_mean=m["mean"], state_std=m["std"],
                       max_horizon=B.H, n_min_obstacles=n_near, seed=s["drift_seed"])
    got = np.stack(seen)
    assert got.dtype == np.float64 and got.tobytes() == ref["rows"].tobytes()
    assert np.stack(actor.states).tobytes() == ((ref["rows"][:-1] - m["mean"]) / m["std"]).tobytes()
    assert ref["actions"].tobytes() == np.stack(actor.actions).tobytes()


def test_conditions_on_the_inputs(bb):
    for name, m in _episodes(bb):
        s, n_obs = m["setup"], m["setup"]["n_obs"]
        ref = B.member_reference(bb, m)
        got = B.summary(ref)
        print(f"{name}: gap {got['gap']:.1e}, rim {got['rim']:.1e}, goal {got['goal']:.1e}, "
              f"re-entries {got['reentries']}")
        assert ref["length"] == B.H and not ref["done"], name
        assert got["gap"] >= B.MIN_GAP and got["rim"] >= B.MIN_RIM and got["goal"] >= B.MIN_GOAL, name
        assert got["reentries"] >= (50 if n_obs >= 255 else 1 if n_obs >= 16 else 0), name
        assert (np.hypot(s["ox"], s["oy"]) <= 50.0).all() and np.hypot(s["px"], s["py"]) <= 20.0, name
        if n_obs > len(B.SPECIAL):  # the last obstacle is the nearest one
            assert ref["rows"][0, 2:5].tolist() == [s["ox"][-1], s["oy"][-1], s["oang"][-1]], name
        if "actor" in m:
            assert len(np.unique(ref["actions"], axis=0)) > B.H // 2, name
        for i, (heading, kind, axis) in enumerate(B.SPECIAL[:n_obs]):
            assert s["oang"][i] == heading and ref["oang"][i] == heading, name
            before, after = (s["ox"][i], ref["ox"][i]) if axis == 0 else (s["oy"][i], ref["oy"][i])
            if kind in ("exact", "inside"):
                assert after == before, (name, heading)
            elif kind == "outside":
                assert abs(after - before) > 1e-7, (name, heading)
    # the windows themselves: the inside headings are off the exact angle and inside, the outside ones outside
    for heading, kind, _ in B.SPECIAL:
        close = any(np.isclose(heading, b) for b in B.WINDOWS)
        assert close == (kind in ("exact", "inside")) and (kind != "inside" or heading not in B.WINDOWS)


def test_goal_cases_are_decided_as_stated(bb):
    for i, (goal, speed, hit) in enumerate(B.GOALS):
        s = B.goal_setup(i)
        assert (s["px"], s["py"]) == (0.0, 0.0) and s["actions"][0].tolist() == [speed, 0.0]
        ref = B.reference_run(bb, s, s["actions"], s["drift"], 1, *B.stats(i, 1))
        assert (ref["length"], ref["done"]) == ((1, True) if hit else (B.GOAL_ROWS, False)), goal
        assert ref["rows"][1, :2].tolist() == [speed, 0.0]
        d2 = ref["margins"]["d2"][0]
        assert (d2 < B.LIM or bool(np.isclose(d2, B.LIM))) == hit
    window = 1e-8 + 1e-5 * B.LIM
    by_isclose = B.goal_setup(B.GOAL_BY_ISCLOSE)
    d2 = B._d2(0.0, 0.0, 1.0, 0.0, *by_isclose["goal"])
    assert B.LIM < d2 <= B.LIM + window and abs(d2 - B.LIM - 1.3e-5) < 1e-8  # touched by isclose alone
    d2 = B._d2(0.0, 0.0, 1.0, 0.0, *B.goal_setup(B.GOAL_BY_ISCLOSE + 1)["goal"])
    assert d2 > B.LIM + window and abs(d2 - B.LIM - 5.2e-5) < 1e-8


def test_headings_of_the_sweep(bb):
    h = B.trig_headings()
    assert h.dtype == np.float32 and len(h) >= 4096 and len(h) % 16 == 0 and np.abs(h[:-104]).max() <= 360.0
    edges = B.window_edges()
    assert len(edges) == 104 and len(np.unique(edges)) == 104 and (h[-104:] == edges).all()
    # the rule stated in csrc/bb_sim.hip: |a - (float) b| <= (float) (1e-8 + 1e-5 |b|), both sides float32
    decided = {True: 0, False: 0}
    for a in edges:
        for b in B.WINDOWS:
            rule = bool(np.abs(a - np.float32(b)) <= np.float32(1e-8 + 1e-5 * b))
            assert rule == bool(np.isclose(a, int(b))), (a, b)
            decided[rule] += 1
    assert decided[True] >= 40 and decided[False] >= 40  # the neighbours straddle every edge
    want = B.trig_expected(bb, h)
    assert want.shape == (len(h), 2) and want.dtype == np.float64
    assert (want.astype(np.float32) == want).all() and np.abs(np.hypot(want[:, 0], want[:, 1]) - 1).max() < 1e-3


def test_actors_of_the_table_are_inside_the_fused_envelope(bb):
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    lib = _lib.load()
    shapes = []
    for c in B.FORWARD:
        m, = B.forward_members(bb, c, episodes=(0,))
        d, keep = bb._actor_desc(m["actor"])
        need = C.c_size_t(0)
        arr = (C.POINTER(_lib.MlpDesc) * 1)(C.pointer(d))
        assert lib.iqlhip_bb_sim_episodes_scratch_bytes(arr, 1, C.byref(need)) == 0, lib.iqlhip_last_error()
        dims = [d.dims[i] for i in range(d.n_layers + 1)]
        assert dims == [8 + 3 * c[1], *c[2], 2] and need.value > 0
        assert (d.hidden_act, d.out_act) == (int(c[3] == "tanh"), int(c[4] == "tanh"))
        shapes.append(dims)
    assert {len(d) - 1 for d in shapes} >= {1, 8} and {11, 26, 56} == {d[0] for d in shapes}
    assert {1, 17, 37, 255, 256} <= {w for d in shapes for w in d[1:-1]}
    members = B.group_members(bb)
    assert len(members) == _lib.MAX_GROUP == 16 and sum("actor" in m for m in members) == 6
    assert {1, 1024} <= {m["setup"]["n_obs"] for m in members}
    assert len({(m["setup"]["n_obs"], m["n_near"]) for m in members}) >= 14
