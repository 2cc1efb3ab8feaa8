"""The host driver of the training step (csrc/api.hip: StepQueue, run_tuned, deep_run): one road from
``train_steps`` to the stream for a lone trainer and for the K members of a group, on the tuned and on the
general step.  What the other files do not pin: the timed diagnostic mode changes no bit, a group of one is
a trainer, one handle taken through every branch of the driver in one sequence, and a ``multi.Solo`` stepper is
its trainer.  Everything is compared bit for bit against plain launches from the same seeds.  -m gpu."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
STATE = ("_params", "_target", "_exp_avg", "_exp_avg_sq")
DEV = "cuda:0"
TUNED, GENERAL = "traj_antmaze", "traj_deep3_w96"


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


@functools.lru_cache(maxsize=None)
def _traj(name, mode):
    _, hyper, data, nets = helpers.load_traj(name, mode)
    return hyper, data, nets


def _make(gh, name, mode, kind, seeds):
    """(what is stepped, its trainers): a lone trainer (kind "solo") or a SeedGroup of mode ``kind``."""
    import iqlpref_amd as ia
    hyper, _, nets = _traj(name, mode)
    trs = [gh.make_trainer(hyper, nets, mode, seed=s) for s in seeds]
    assert trs[0].step_kind(hyper["batch"]) == ("tuned" if name == TUNED else "general")
    return (trs[0] if kind == "solo" else ia.SeedGroup(trs, mode=kind)), trs


def _same_state(a, b, where=""):
    torch.cuda.synchronize()
    for ta, tb in zip(a, b):
        assert ta.total_it == tb.total_it, where
        for name in STATE:
            assert torch.equal(getattr(ta, name), getattr(tb, name)), f"{where}{name}"


def _timing(h, on):
    """Switch the per-kernel timing of a trainer's / a group's launches; off: (averages in ms, launches) first."""
    import iqlpref_amd as ia
    lib, group = ia._lib.load(), isinstance(h, ia.SeedGroup)
    handle = h._group if group else h._handle
    got = None
    if not on:
        avg, n = (C.c_double * 3)(), C.c_int64()
        ia._lib.check((lib.iqlhip_group_get_timing if group else lib.iqlhip_trainer_get_timing)(
            handle, C.byref(avg), C.byref(n)))
        got = (list(avg), int(n.value))
    ia._lib.check((lib.iqlhip_group_set_timing if group else lib.iqlhip_trainer_set_timing)(handle, int(on)))
    return got


# ---- 1. the timed diagnostic mode ---------------------------------------------------------------------------- #
@pytest.mark.parametrize("name,mode,kind", [
    (TUNED, "fp32", "solo"), (TUNED, "bf16", "solo"), (GENERAL, "bf16", "solo"),
    (TUNED, "bf16", "group"), (GENERAL, "bf16", "general")])
def test_timed_mode_changes_no_bit(gh, name, mode, kind):
    """5 steps with the per-kernel timing on (eager, whatever graph_unroll says), then 5 with it off that
    continue them = 10 untimed steps from the same seeds; the timing reports its 5 launches."""
    import iqlpref_amd as ia
    hyper, data, _ = _traj(name, mode)
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    seeds = (21,) if kind == "solo" else (21, 22)
    plain, want = _make(gh, name, mode, kind, seeds)
    plain.train_steps(buf, 10, B, return_losses=False, graph_unroll=0)
    timed, got = _make(gh, name, mode, kind, seeds)
    if kind == "solo":
        timed._ensure_handle(B)
    else:
        timed._ensure_group(B)
    _timing(timed, True)
    timed.train_steps(buf, 5, B, return_losses=False, graph_unroll=4)
    assert timed.launch_counts() == (5, 0)
    avg_ms, launches = _timing(timed, False)
    assert launches == 5
    assert all(math.isfinite(v) and v >= 0 for v in avg_ms), avg_ms
    timed.train_steps(buf, 5, B, return_losses=False, graph_unroll=4)
    assert timed.launch_counts() == (5 + 1, 1)
    _same_state(want, got, f"{name}/{mode}/{kind}: ")
    if kind != "solo":
        assert not torch.equal(got[0]._params, got[1]._params)
        assert isinstance(timed, ia.SeedGroup) and all(t.launch_counts() == (0, 0) for t in got)
        timed.close(), plain.close()


# ---- 2. a group of one --------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name,group_mode", [(TUNED, "group"), (GENERAL, "general")])
def test_a_group_of_one_is_a_trainer(gh, name, group_mode):
    hyper, data, _ = _traj(name, "bf16")
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    lone, want = _make(gh, name, "bf16", "solo", (31,))
    group, got = _make(gh, name, "bf16", group_mode, (31,))
    lone.train_steps(buf, 9, B, return_losses=False, graph_unroll=4)
    group.train_steps(buf, 9, B, return_losses=False, graph_unroll=4)
    _same_state(want, got, f"{name}: ")
    assert group.launch_counts() == lone.launch_counts() == (1, 2)  # 9 = 2 replays of 4 steps + 1 plain step
    group.close()


# ---- 3. every branch of the driver on one handle --------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["solo", "group"])
def test_one_handle_through_every_branch_of_the_driver(gh, kind):
    """Plain launches, a graph, a call with outputs (which re-sends the arguments), another unroll (captured
    again), valid-row counts that are all the whole batch (the counted graph, never continued; whole-batch counts
    change no bit) and plain launches again, on the same handle = the same number of steps in one eager call."""
    hyper, data, _ = _traj(TUNED, "fp32")
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    seeds = (41,) if kind == "solo" else (41, 42)
    whole = lambda n: torch.full((n,), B, dtype=torch.int32, device=gh.DEV)
    # (steps, graph_unroll, return_losses, counts) and what the call issues: (plain steps, replays)
    calls = [((3, 0, False, False), (3, 0)),
             ((7, 3, False, False), (1, 2)),   # 2 replays of 3 + 1
             ((2, 0, True, False), (2, 0)),
             ((5, 2, False, False), (1, 2)),   # 2 replays of 2 + 1
             ((4, 2, False, True), (0, 2)),    # the same unroll, the counted k_backward: 2 replays of another graph
             ((3, 0, False, False), (3, 0))]
    total = sum(c[0][0] for c in calls)
    assert total == 24
    plain, want = _make(gh, TUNED, "fp32", kind, seeds)
    plain.train_steps(buf, total, B, return_losses=False, graph_unroll=0)
    assert plain.launch_counts() == (total, 0)
    h, got = _make(gh, TUNED, "fp32", kind, seeds)
    kept = []  # (the calls are asynchronous: their inputs and outputs stay alive until the comparison)
    for (n, unroll, losses, counts), _ in calls:
        valid = whole(n) if counts else None
        out = h.train_steps(buf, n, B, return_losses=losses, graph_unroll=unroll, n_valid=valid)
        assert (out is not None) == losses
        kept += [valid, out]
    assert h.launch_counts() == (3 + 1 + 2 + 1 + 0 + 3, 0 + 2 + 0 + 2 + 2 + 0)
    assert h.launch_counts() == tuple(sum(c[1][i] for c in calls) for i in (0, 1))
    _same_state(want, got, f"{kind}: ")
    if kind == "group":
        assert not torch.equal(got[0]._params, got[1]._params)
        h.close(), plain.close()


# ---- 4. a Solo stepper is its trainer -------------------------------------------------------------------------- #
def _small_trainer(seed, S=11, A=3, H=64):
    import iqlpref_amd as ia
    torch.manual_seed(seed)
    q, v, actor = (ia.TwinQ(S, A, hidden_dim=H).to(DEV), ia.ValueFunction(S, hidden_dim=H).to(DEV),
                   ia.GaussianPolicy(S, A, 1.0, hidden_dim=H).to(DEV))
    adam = lambda mod: torch.optim.Adam(mod.parameters(), lr=3e-4)
    return ia.ImplicitQLearning(1.0, actor, adam(actor), q, adam(q), v, adam(v), max_steps=1000, device=DEV,
                                precision="fp32", seed=seed)


def _tensors(x, prefix=""):
    if isinstance(x, dict):
        for k, v in x.items():
            yield from _tensors(v, f"{prefix}/{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _tensors(v, f"{prefix}/{i}")
    elif isinstance(x, torch.Tensor):
        yield prefix, x


@pytest.mark.parametrize("short_last", [False, True])
def test_a_solo_stepper_is_its_trainer(gh, short_last):
    """40 steps on explicit indices, once by ``trainer.train_steps`` and once through ``stepper([trainer])``: the
    same losses, state and launch counts, and the trainer joins no group.  ``short_last``: per-step valid-row
    counts, the last step 13 rows of 32."""
    import numpy as np
    import iqlpref_amd as ia
    from iqlpref_amd import multi
    S, A, B, N, steps = 11, 3, 32, 500, 40
    rng = np.random.default_rng(17)
    buf = ia.ReplayBuffer(S, A, N, DEV)
    buf.load_d4rl_dataset({"observations": rng.standard_normal((N, S)).astype(np.float32),
                           "actions": rng.uniform(-1, 1, (N, A)).astype(np.float32),
                           "rewards": rng.standard_normal(N).astype(np.float32),
                           "next_observations": rng.standard_normal((N, S)).astype(np.float32),
                           "terminals": (rng.uniform(size=N) < 0.1).astype(np.float32)})
    idx = torch.from_numpy(rng.integers(0, N, (steps, B))).to(DEV)
    valid = torch.tensor([B] * (steps - 1) + [13], dtype=torch.int32, device=DEV) if short_last else None
    lone, member = _small_trainer(5), _small_trainer(5)
    assert lone.step_kind(B) == "tuned"
    want = lone.train_steps(buf, steps, B, indices=idx, n_valid=valid)
    solo = multi.stepper([member])
    assert isinstance(solo, multi.Solo) and solo.trainers == [member]
    got = solo.train_steps([buf], steps, B, indices=[idx], n_valid=valid, return_losses=True)
    solo.synchronize()
    assert len(got) == 1 and torch.equal(got[0], want) and torch.isfinite(want).all()
    a, b = dict(_tensors(member.state_dict())), dict(_tensors(lone.state_dict()))
    assert a.keys() == b.keys() and len(a) > 20
    for name in b:
        assert torch.equal(a[name], b[name]), name
    _same_state([lone], [member])
    assert member.launch_counts() == lone.launch_counts() != (0, 0)
    assert member._group_owner is None
    solo.close()
    assert member.total_it == lone.total_it == steps
