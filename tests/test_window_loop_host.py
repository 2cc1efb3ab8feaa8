"""_window_loop: the train / log / evaluate / checkpoint / resume loop of ``train()`` and ``sweep.train_runs``,
driven with fakes.  No GPU, no library load.

Every fake writes into one event list: ("group", active) when the factory is called, ("steps", t, n, active),
("sync", members) / ("close", members) of a group, ("log", record, step), ("eval", k, t), ("state_dict", k),
("resume_state", k) and ("exchange", records).  Step s of member k has the losses (s, 10 s + k, 100 s + k)."""
import os

import numpy as np
import pytest
import torch

from iqlpref_amd import _resume
from iqlpref_amd import _window_loop as wl

OWN = [(8, 4, 4), (12, 4, 6), (10, 5, 10)]  # (total, log_every, eval_every) of three members with their own settings


class Cut(Exception):
    pass


class Trainer:
    def __init__(self, k, events):
        self.k, self.total_it, self.events = k, 0, events

    def state_dict(self):
        self.events.append(("state_dict", self.k))
        return {"w": torch.tensor([float(self.k), float(self.total_it)])}

    def resume_state(self):
        self.events.append(("resume_state", self.k))
        return {"k": self.k, "total_it": self.total_it}

    def load_resume_state(self, state):
        assert state["k"] == self.k
        self.total_it = state["total_it"]


class Group:
    def __init__(self, members, events):
        self.members, self.events = members, events

    def synchronize(self):
        self.events.append(("sync", self.members))

    def close(self):
        self.events.append(("close", self.members))


def rows(k, first, n):
    s = torch.arange(first, first + n, dtype=torch.float32)
    return torch.stack([s, 10 * s + k, 100 * s + k], dim=1)


def strip(x):
    if isinstance(x, dict):
        return {n: strip(v) for n, v in x.items() if n != "steps_per_sec"}
    return [strip(v) for v in x] if isinstance(x, (list, tuple)) else x


def scores_at(k, t):
    return np.array([t + k, t + k + 1.0])


def drive(settings, path=None, *, grouped=True, resume=False, scores=True, cut_at=None, at_most=None,
          keep_previous=False, goal_env=False):
    """One start of the loop over ``len(settings)`` fake members; ``settings``: (total, log_every, eval_every)
    each.  -> (events, trainers, ckpt_dirs, state).  ``grouped`` False: the factory gives None (one seed)."""
    K = len(settings)
    events, cut = [], Cut()
    trainers = [Trainer(k, events) for k in range(K)]
    dirs = [None if path is None else str(path / f"m{k}") for k in range(K)]
    for d in dirs:
        if d is not None:
            os.makedirs(d, exist_ok=True)

    def make_group(active):
        events.append(("group", active))
        return Group(tuple(active), events) if grouped else None

    def steps(group, active, t, n):
        assert (group is not None) == grouped
        events.append(("steps", t, n, active))
        for k in active:
            trainers[k].total_it += n
        return [rows(k, t, n) for k in active]

    def evaluate(k, trainer, t):
        assert trainer is trainers[k] and trainer.total_it == t
        if t == cut_at:
            events.append(("raise", k, t))
            raise cut
        events.append(("eval", k, t))
        return (scores_at(k, t), [] if t == 6 else [t, t + 2]) if scores else (None, [])

    state = wl.restore(trainers, dirs, at_most=at_most) if resume else wl.State(K)
    total, log_every, eval_every = ([s[i] for s in settings] for i in range(3))
    try:
        wl.run(state, trainers, [40 + k for k in range(K)], total, log_every, eval_every,
               lambda rec, step: events.append(("log", strip(rec), step)), dirs, make_group, steps, evaluate,
               lambda rec, k: dict(rec, who=k), goal_env=goal_env,
               exchange=lambda records: events.append(("exchange", strip(records))), resume=resume,
               keep_previous=keep_previous)
    except Cut as e:  # (the loop hands on what evaluate raised)
        assert cut_at is not None and e is cut
    return events, trainers, dirs, state


def window_record(k, first, n):
    """The window record of steps first .. first + n - 1 of member k, as the loop must compute it."""
    v, q, a = rows(k, first, n).mean(dim=0).tolist()
    return {"value_loss": v, "q_loss": q, "actor_loss": a}


def window_log(k, first, n):
    return ("log", dict(window_record(k, first, n), who=k), first + n)


def files(dirs):
    """{member: {file name: loaded contents}} without the wall-clock field."""
    return {k: {f: strip(torch.load(os.path.join(d, f), weights_only=True)) for f in sorted(os.listdir(d))}
            for k, d in enumerate(dirs)}


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[n], b[n]) for n in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_next_boundary_and_one_entry_per_member():
    assert [wl.next_boundary(t, 12, 4, 6) for t in (0, 4, 6, 8)] == [4, 6, 8, 12]
    assert wl.next_boundary(8, 10, 4, 6) == 10
    with pytest.raises(ValueError, match="one entry per member"):
        wl.run(wl.State(2), [None, None], [0, 1], [4, 4, 4], 2, 2, None, [None, None], None, None, None, None)


# --------------------------------------------------------------------------- #
# 1. the whole observable order
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("K", [1, 3])
def test_order_of_everything_observable(K, scores, tmp_path):
    events, trainers, dirs, state = drive([(12, 4, 6)] * K, tmp_path, grouped=K > 1, scores=scores, goal_env=True)
    everyone = list(range(K))

    def boundary(t, window_first):
        """What happens at the evaluation boundary t; the last window record is that of window_first .. + 3."""
        out = [("sync", tuple(everyone))] if K > 1 else []
        records = []
        for k in everyone:
            out.append(("eval", k, t))
            log = {}
            if scores:  # (no success at step 6: -1)
                log = {"mean_score": t + k + 0.5, "avg_steps_to_goal": -1.0 if t == 6 else t + 1.0}
                out.append(("log", dict(log, who=k), t))
            out.append(("state_dict", k))
            records.append(dict(window_record(k, window_first, 4), seed=40 + k, total_it=t, **log))
        return out + [("exchange", records)]

    assert events == (
        [("group", everyone), ("steps", 0, 4, everyone)] + [window_log(k, 0, 4) for k in everyone]
        + [("steps", 4, 2, everyone)] + boundary(6, 0)
        + [("steps", 6, 2, everyone)] + [window_log(k, 4, 4) for k in everyone]  # a window over two chunks
        + [("steps", 8, 4, everyone)] + [window_log(k, 8, 4) for k in everyone] + boundary(12, 8)
        + ([("sync", tuple(everyone)), ("close", tuple(everyone))] if K > 1 else []))
    assert window_record(1, 4, 4) == {"value_loss": 5.5, "q_loss": 56.0, "actor_loss": 551.0}
    assert state.t == 12 and [tr.total_it for tr in trainers] == [12] * K
    got = files(dirs)
    for k in everyone:  # checkpoints also without scores; no resume file without resume
        assert list(got[k]) == ["checkpoint_11.pt", "checkpoint_5.pt"]
        assert [got[k][f"checkpoint_{s}.pt"]["w"].tolist() for s in (5, 11)] == [[k, 6.0], [k, 12.0]]


def test_no_directory_no_exchange_no_goal_env():
    K = 2
    events = []
    trainers = [Trainer(k, events) for k in range(K)]
    wl.run(wl.State(K), trainers, [7, 8], 6, 3, 6, lambda rec, step: events.append(("log", rec, step)), [None] * K,
           lambda active: None, lambda g, active, t, n: [rows(k, t, n) for k in active],
           lambda k, trainer, t: (scores_at(k, t), [1]), lambda rec, k: rec)
    assert [e for e in events if e[0] != "log"] == []  # no state_dict without a directory
    assert [e[1] for e in events if "mean_score" in e[1]] == [{"mean_score": 6.5}, {"mean_score": 7.5}]


# --------------------------------------------------------------------------- #
# 2. members with their own settings
# --------------------------------------------------------------------------- #
def test_members_with_their_own_settings(tmp_path):
    events, trainers, dirs, _ = drive(OWN, tmp_path)
    all3, two, one = (0, 1, 2), (1, 2), (1,)
    assert [e for e in events if e[0] in ("group", "steps", "sync", "close")] == [
        ("group", [0, 1, 2]), ("steps", 0, 4, [0, 1, 2]), ("sync", all3),  # member 0 evaluates at 4
        ("steps", 4, 1, [0, 1, 2]), ("steps", 5, 1, [0, 1, 2]), ("sync", all3),  # member 1 at 6
        ("steps", 6, 2, [0, 1, 2]), ("sync", all3), ("sync", all3), ("close", all3),  # member 0 at 8, and leaves
        ("group", [1, 2]), ("steps", 8, 2, [1, 2]), ("sync", two), ("sync", two), ("close", two),  # member 2 at 10
        ("group", [1]), ("steps", 10, 2, [1]), ("sync", one), ("sync", one), ("close", one)]  # the lone survivor's
    assert [e for e in events if e[0] == "log" and "value_loss" in e[1]] == [
        window_log(0, 0, 4), window_log(1, 0, 4), window_log(2, 0, 5), window_log(0, 4, 4), window_log(1, 4, 4),
        window_log(2, 5, 5), window_log(1, 8, 4)]
    assert [e[1:] for e in events if e[0] == "eval"] == [(0, 4), (1, 6), (0, 8), (2, 10), (1, 12)]
    assert [len(e[1]) for e in events if e[0] == "exchange"] == [1] * 5
    assert [tr.total_it for tr in trainers] == [8, 12, 10]
    assert [sorted(os.listdir(d)) for d in dirs] == [["checkpoint_3.pt", "checkpoint_7.pt"],
                                                     ["checkpoint_11.pt", "checkpoint_5.pt"], ["checkpoint_9.pt"]]


# --------------------------------------------------------------------------- #
# 3. resume, run without interruption
# --------------------------------------------------------------------------- #
def test_generations_of_an_uninterrupted_run(tmp_path):
    events, trainers, dirs, _ = drive([(14, 4, 10)], tmp_path / "a", resume=True, keep_previous=True)
    assert [e for e in events if e[0] in ("steps", "resume_state")] == [
        ("steps", 0, 4, [0]), ("steps", 4, 4, [0]), ("steps", 8, 2, [0]), ("resume_state", 0), ("steps", 10, 2, [0]),
        ("steps", 12, 2, [0]), ("resume_state", 0)]
    assert _resume.steps_in(dirs[0]) == [10, 14]  # (keep_previous: both are still there to be looked at)
    seen = files(dirs)[0]
    assert same(seen["resume_10.pt"], {"finished": False, "trainer": {"k": 0, "total_it": 10}, "sampler": None,
                                       "loop": {"window": rows(0, 8, 2), "last": window_record(0, 4, 4)}, "step": 10})
    assert same(seen["resume_14.done.pt"], {"finished": True, "trainer": {"k": 0, "total_it": 14}, "sampler": None,
                                            "loop": {"window": rows(0, 12, 2), "last": window_record(0, 8, 4)},
                                            "step": 14})
    # without keep_previous only the newest file remains; with it the two newest
    _, _, dirs, _ = drive([(14, 4, 10)], tmp_path / "b", resume=True)
    assert sorted(os.listdir(dirs[0])) == ["checkpoint_9.pt", "resume_14.done.pt"]
    _, _, dirs, _ = drive([(14, 4, 4)], tmp_path / "c", resume=True, keep_previous=True)
    assert sorted(os.listdir(dirs[0])) == ["checkpoint_11.pt", "checkpoint_3.pt", "checkpoint_7.pt", "resume_12.pt",
                                           "resume_14.done.pt"]
    # a window is None in a generation written at a log boundary
    assert _resume.read(dirs[0], 12)["loop"]["window"] is None
    for name in ("a", "b", "c"):  # started again: nothing is trained, evaluated, built or written
        before = sorted(os.listdir(tmp_path / name / "m0"))
        events, trainers, dirs, state = drive([(14, 4, 10 if name != "c" else 4)], tmp_path / name, resume=True,
                                              keep_previous=name != "b")
        assert events == [] and state.t == 14 and trainers[0].total_it == 14
        assert sorted(os.listdir(dirs[0])) == [f for f in before if f.startswith("checkpoint")] + ["resume_14.done.pt"]


# --------------------------------------------------------------------------- #
# 4. resume, interrupted
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cut_at,restored,going_on", [(6, 4, [0, 1, 2]), (10, 8, [1, 2])])
def test_an_interrupted_run_resumed_is_the_uninterrupted_run(tmp_path, cut_at, restored, going_on):
    whole, whole_trainers, whole_dirs, _ = drive(OWN, tmp_path / "whole", resume=True)
    first, _, dirs, _ = drive(OWN, tmp_path / "cut", resume=True, cut_at=cut_at)
    # every member holds a file of the generation before the cut, due at that boundary or not
    assert [_resume.steps_in(d) for d in dirs] == [[restored]] * 3
    assert [_resume.status(d) for d in dirs] == ["done" if k not in going_on else f"at step {restored}"
                                                 for k in range(3)]
    second, trainers, _, state = drive(OWN, tmp_path / "cut", resume=True)
    assert second[0] == ("group", going_on)  # a finished member is left out
    start = whole.index(("steps", restored, second[1][2], going_on))
    assert second[1:] == whole[start:]  # records, evaluations, exchanges, synchronizes, files written: all of it
    assert first[:first.index(("steps", restored, second[1][2], going_on))] == whole[:start]
    assert [tr.total_it for tr in trainers] == [tr.total_it for tr in whole_trainers] == [8, 12, 10]
    assert same(files(dirs), files(whole_dirs))
    assert [sorted(f for f in os.listdir(d) if f.startswith("resume"))[0] for d in dirs] == [
        "resume_8.done.pt", "resume_12.done.pt", "resume_10.done.pt"]


def test_at_most_picks_the_older_generation(tmp_path):
    whole, _, dirs, _ = drive([(14, 4, 4)] * 2, tmp_path, resume=True, keep_previous=True)
    assert [_resume.steps_in(d) for d in dirs] == [[12, 14]] * 2
    again, trainers, _, state = drive([(14, 4, 4)] * 2, tmp_path, resume=True, keep_previous=True, at_most=13)
    assert again[0] == ("group", [0, 1]) and again[1:] == whole[whole.index(("steps", 12, 2, [0, 1])):]
    assert state.t == 14 and [tr.total_it for tr in trainers] == [14, 14]
    assert [_resume.steps_in(d) for d in dirs] == [[12, 14]] * 2


@pytest.mark.parametrize("grouped", [True, False])
def test_an_exception_closes_the_group_once_without_a_synchronize(grouped):
    events, *_ = drive(OWN, grouped=grouped, cut_at=10)  # member 0 left at 8: the second group is the open one
    assert events[events.index(("raise", 2, 10)) + 1:] == ([("close", (1, 2))] if grouped else [])
    assert [e for e in events if e[0] == "close"] == ([("close", (0, 1, 2)), ("close", (1, 2))] if grouped else [])


# --------------------------------------------------------------------------- #
# 5. a generation that sweep.train_runs wrote before this loop: no "last"
# --------------------------------------------------------------------------- #
def test_an_old_sweep_generation_restores(tmp_path):
    d = tmp_path / "m0"
    d.mkdir()
    _resume.write(str(d), 10, {"finished": False, "trainer": {"k": 0, "total_it": 10}, "sampler": None,
                               "loop": {"window": rows(0, 8, 2)}})
    events, trainers, _, state = drive([(14, 4, 10)], tmp_path, resume=True)
    assert events[:3] == [("group", [0]), ("steps", 10, 2, [0]), window_log(0, 8, 4)]
    assert state.t == 14 and sorted(os.listdir(d)) == ["resume_14.done.pt"]
    assert same(strip(_resume.read(str(d), 14)["loop"]), {"window": rows(0, 12, 2), "last": window_record(0, 8, 4)})
    # and one of a finished run
    _resume.write(str(d), 14, {"finished": True, "trainer": {"k": 0, "total_it": 14}, "sampler": None,
                               "loop": {"window": rows(0, 12, 2)}})
    events, trainers, _, state = drive([(14, 4, 10)], tmp_path, resume=True)
    assert events == [] and state.last == [{}] and trainers[0].total_it == 14


# --------------------------------------------------------------------------- #
# 6. a synchronize always comes first
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("settings", [[(12, 4, 6)] * 3, OWN, [(7, 4, 5), (12, 4, 6)]],
                         ids=["seeds", "own", "no_eval_at_end"])
def test_a_synchronize_precedes_every_read_of_a_member(tmp_path, settings):
    events, *_ = drive(settings, tmp_path, resume=True)
    queued, reads = False, 0
    for e in events:
        if e[0] == "steps":
            queued = True
        elif e[0] == "sync":
            queued = False
        elif e[0] in ("eval", "state_dict", "resume_state"):
            assert not queued, e
            reads += 1
    assert reads > 0
    if settings[0][0] == 7:  # member 0 ends at 7 without an evaluation: the generation's own synchronize
        at = events.index(("steps", 6, 1, [0, 1]))
        assert events[at + 1:at + 4] == [("sync", (0, 1)), ("resume_state", 0), ("resume_state", 1)]
