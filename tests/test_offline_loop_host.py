"""_offline_loop: the chunked train / evaluate / checkpoint loop of the custom-offline flavours and its
checkpoint directories, driven with fakes.  No GPU, no library load."""
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

from iqlpref_amd import _offline_loop as ol
from iqlpref_amd import _resume

LOSS_KEYS = ("value_loss", "q_loss", "actor_loss")


@dataclass
class Config:
    name: str = "fake"
    checkpoints_path: Optional[str] = None


class Trainer:
    def __init__(self, k):
        self.k, self.done, self.actor = k, 0, object()

    def state_dict(self):
        return {"w": torch.tensor([float(self.k), float(self.done)])}

    def resume_state(self):
        return {"done": self.done}

    def load_resume_state(self, state):
        self.done = state["done"]


class Failure(Exception):
    pass


class Group:
    def __init__(self, events):
        self.events = events

    def synchronize(self):
        self.events.append(("sync",))

    def close(self):
        self.events.append(("close",))


def drive(K, returns, path=None, total=12, normalized=None, best_by_return=False, fail_at=None, records=None,
          resume=False):
    """Run the loop (every=6, chunk=4) over fakes; ``returns[b]`` is the mean return of every seed at
    boundary b.  -> (events, trainers, seeds, ckpt_dirs); events are ("group", active) of every ``make_group``
    call (which gives None for K = 1), ("steps", t, n), ("sync",), ("close",), ("eval", k, step) and
    ("log", record, step) in the order they happened.  ``fail_at``: the evaluation at that step raises.
    ``records(ckpt_dirs)``: the recorder, instead of ``BestModelRecords``."""
    events = []
    seeds = [40 + k for k in range(K)]
    trainers = [Trainer(k) for k in range(K)]
    group = []

    def make_group(active):
        events.append(("group", active))
        group[:] = [Group(events) if K > 1 else None]
        return group[0]

    def steps(got, active, t, n):
        assert got is group[0] and active == list(range(K))
        events.append(("steps", t, n))
        for tr in trainers:
            tr.done += n
        s = torch.arange(t, t + n, dtype=torch.float32)
        return [torch.stack([s, 10 * s + k, 100 * s + k], dim=1) for k in range(K)]

    def evaluate(k, trainer, step):
        assert trainer is trainers[k]
        if step == fail_at:
            events.append(("raise",))
            raise Failure(events)
        events.append(("eval", k, step))
        r = returns[step // 6]
        return np.array([r - 0.5, r + 0.5])

    ckpt_dirs = ol.checkpoint_dirs(Config(checkpoints_path=None if path is None else str(path)), seeds)
    ol.run(trainers, seeds, make_group, total, 6, 4,
           lambda rec, step: events.append(("log", dict(rec), step)), ckpt_dirs, steps, evaluate,
           ol.BestModelRecords(ckpt_dirs, normalized, best_by_return) if records is None else records(ckpt_dirs),
           resume=resume)
    return events, trainers, seeds, ckpt_dirs


def loss_records(K, seeds, t, n):
    """What the flush of chunk (t, n) logs: seeds are the outer loop."""
    out = []
    for k in range(K):
        for s in range(t, t + n):
            rec = {"value_loss": float(s), "q_loss": float(10 * s + k), "actor_loss": float(100 * s + k)}
            out.append(("log", dict(rec, seed=seeds[k]) if K > 1 else rec, s))
    return out


def eval_records(K, seeds, step, per_seed):
    """The records of one boundary: ``per_seed`` is the list of (key, value) pairs every seed logs."""
    out = [("sync",)] if K > 1 else []
    for k in range(K):
        out.append(("eval", k, step))
        for key, value in per_seed:
            out.append(("log", dict({key: value}, seed=seeds[k]) if K > 1 else {key: value}, step))
    return out


def pos(events, ev):
    return events.index(ev)


@pytest.mark.parametrize("K", [1, 3])
def test_order_of_everything_observable(K, tmp_path):
    events, trainers, seeds, dirs = drive(K, (2.0, 1.0), tmp_path)
    assert [e for e in events if e[0] == "steps"] == [("steps", 0, 4), ("steps", 4, 2), ("steps", 6, 4),
                                                      ("steps", 10, 2)]
    # the overlap: the losses of chunk (0, 4) come back after chunk (4, 2) is queued, before the evaluation
    first_chunk = loss_records(K, seeds, 0, 4)
    first_eval = next(i for i, e in enumerate(events) if e[0] == "log" and "evaluation_return" in e[1])
    for rec in first_chunk:
        assert pos(events, ("steps", 4, 2)) < pos(events, rec) < first_eval
    # one loss record per step and seed, with its values at its step
    losses = [e for e in events if e[0] == "log" and "value_loss" in e[1]]
    want = sum((loss_records(K, seeds, t, n) for t, n in ((0, 4), (4, 2), (6, 4), (10, 2))), [])
    assert losses == want and len(losses) == 12 * K
    assert all(("seed" in e[1]) == (K > 1) for e in events if e[0] == "log")
    assert all(set(e[1]) - {"seed"} == set(LOSS_KEYS) for e in losses)
    # the whole sequence: queue, flush, [flush, synchronize, evaluate] -- the best model stays that of step 5
    at = lambda step, ret: eval_records(K, seeds, step, [("evaluation_return", ret), ("best_score_so_far", 2.0),
                                                           ("best_step_so_far", 5)])
    everyone = list(range(K))
    assert events == ([("group", everyone), ("steps", 0, 4), ("steps", 4, 2)] + first_chunk + loss_records(K, seeds, 4, 2) + at(5, 2.0)
                      + [("steps", 6, 4), ("steps", 10, 2)] + loss_records(K, seeds, 6, 4)
                      + loss_records(K, seeds, 10, 2) + at(11, 1.0)
                      + ([("sync",), ("close",)] if K > 1 else []))  # all end: the group is dissolved, none built
    if K > 1:  # synchronize comes before the first evaluation of each boundary
        syncs = [i for i, e in enumerate(events) if e == ("sync",)]
        assert syncs[:2] == [pos(events, ("eval", 0, 5)) - 1, pos(events, ("eval", 0, 11)) - 1]
    else:  # None as the group: nothing is synchronized or closed
        assert not [e for e in events if e[0] in ("sync", "close")]

    # files: best_model.pt written once, with the state at step 5 (6 steps done)
    files = ["best_model.pt", "checkpoint_11.pt", "checkpoint_5.pt", "config.yaml"]
    if K == 1:
        assert dirs == [str(tmp_path)] and sorted(os.listdir(tmp_path)) == files
    else:
        assert dirs == [str(tmp_path / f"seed_{s}") for s in seeds]
        assert sorted(os.listdir(tmp_path)) == ["config.yaml"] + [f"seed_{s}" for s in seeds]
        for d in dirs:
            assert sorted(os.listdir(d)) == files[:3]
    for k, d in enumerate(dirs):
        load = lambda name: torch.load(os.path.join(d, name), weights_only=True)["w"].tolist()
        assert load("best_model.pt") == load("checkpoint_5.pt") == [float(k), 6.0]
        assert load("checkpoint_11.pt") == [float(k), 12.0]
    import yaml
    with open(tmp_path / "config.yaml") as f:
        assert yaml.safe_load(f) == {"name": "fake", "checkpoints_path": str(tmp_path)}


@pytest.mark.parametrize("K", [1, 3])
def test_an_exception_closes_the_group_once_without_a_synchronize(K):
    with pytest.raises(Failure) as err:
        drive(K, (2.0, 1.0), fail_at=11)
    events = err.value.args[0]  # what had happened when evaluate raised, and what the loop did on its way out:
    assert events[events.index(("raise",)) + 1:] == ([("close",)] if K > 1 else [])  # no synchronize, no log
    assert events.count(("close",)) == (1 if K > 1 else 0)
    assert [e for e in events if e[0] == "group"] == [("group", list(range(K)))]


def test_members_lifecycle_and_spread():
    calls = []

    class G:
        def __init__(self, active):
            self.active = tuple(active)

        def synchronize(self):
            calls.append(("sync", self.active))

        def close(self):
            calls.append(("close", self.active))

    def make(active):
        calls.append(("group", active))
        return G(active)

    with ol.Members(make, [0, 1, 2]) as live:
        live.keep([0, 1, 2])  # nobody left: nothing happens
        assert not live.commit_due([], [0, 1, 2]) and live.commit_due([1], [0, 1, 2]) and calls == [("group", [0, 1, 2])]
        assert live.commit_due([], [0, 2]) and calls[-1] == ("sync", (0, 1, 2))  # no evaluation synchronized
        live.keep([0, 2])
        assert live.active == [0, 2] and live.group.active == (0, 2)
        live.keep([])
        assert live.active == [] and live.group is None
    assert calls == [("group", [0, 1, 2]), ("sync", (0, 1, 2)), ("sync", (0, 1, 2)), ("close", (0, 1, 2)),
                     ("group", [0, 2]), ("sync", (0, 2)), ("close", (0, 2))]  # nothing built for nobody
    del calls[:]
    with ol.Members(make, [4]):
        pass
    assert calls == [("group", [4]), ("sync", (4,)), ("close", (4,))]
    with ol.Members(lambda active: None, [0]) as live:  # None: nothing to synchronize or close
        live.synchronize()
    assert ol.Members(make, []).group is None and calls[-1] == ("close", (4,))
    assert ol.spread(3, 2) == [3, 3] and ol.spread([1, 2.0], 2) == [1, 2] and ol.spread(True, 1) == [1]


@pytest.mark.parametrize("K", [1, 3])
def test_an_equal_score_does_not_replace_the_best(K, tmp_path):
    events, _, seeds, dirs = drive(K, (1.0, 1.0), tmp_path)
    best = [(e[1]["best_step_so_far"], e[2]) for e in events if e[0] == "log" and "best_step_so_far" in e[1]]
    assert best == [(5, 5)] * K + [(5, 11)] * K
    for k, d in enumerate(dirs):
        assert torch.load(os.path.join(d, "best_model.pt"), weights_only=True)["w"].tolist() == [float(k), 6.0]


def scripted(values):
    """A ``normalized`` whose call number c returns values[c], or raises it."""
    calls = iter(values)

    def normalized(scores):
        v = next(calls)
        if isinstance(v, Exception):
            raise v
        return v
    return normalized


def evaluation_logs(events):
    return [(next(iter(e[1].items())), e[2]) for e in events if e[0] == "log" and "value_loss" not in e[1]]


def test_normalized_score_rules():
    # no score at the first boundary (the raw return counts), 0.5 at the second
    events, *_ = drive(1, (3.0, 1.0), normalized=scripted([ValueError("no reference score"), 0.5]))
    assert evaluation_logs(events) == [
        (("evaluation_return", 3.0), 5), (("best_score_so_far", 3.0), 5), (("best_step_so_far", 5), 5),
        (("evaluation_return", 1.0), 11), (("normalized_score", 50.0), 11), (("best_score_so_far", 50.0), 11),
        (("best_step_so_far", 11), 11)]
    # best_by_return: the score is logged, the best model goes by the raw mean at both boundaries
    events, *_ = drive(1, (3.0, 1.0), normalized=scripted([ValueError("no reference score"), 0.5]),
                       best_by_return=True)
    assert evaluation_logs(events) == [
        (("evaluation_return", 3.0), 5), (("best_score_so_far", 3.0), 5), (("best_step_so_far", 5), 5),
        (("evaluation_return", 1.0), 11), (("normalized_score", 50.0), 11), (("best_score_so_far", 3.0), 11),
        (("best_step_so_far", 5), 11)]
    # a score once obtained stays for its seed: it is not logged again, and a greater raw return does not beat it
    events, *_ = drive(1, (1.0, 70.0), normalized=scripted([0.5, ValueError("no reference score")]))
    assert evaluation_logs(events) == [
        (("evaluation_return", 1.0), 5), (("normalized_score", 50.0), 5), (("best_score_so_far", 50.0), 5),
        (("best_step_so_far", 5), 5),
        (("evaluation_return", 70.0), 11), (("best_score_so_far", 50.0), 11), (("best_step_so_far", 5), 11)]


def test_normalized_score_is_kept_per_seed():
    # calls: seed 0 and 1 at step 5, then at step 11; only seed 1 ever gets a score
    err = ValueError("no reference score")
    events, _, seeds, _ = drive(2, (3.0, 1.0), normalized=scripted([err, 0.5, err, err]))
    best = {s: [e[1]["best_score_so_far"] for e in events
                if e[0] == "log" and "best_score_so_far" in e[1] and e[1]["seed"] == s] for s in seeds}
    assert best == {seeds[0]: [3.0, 3.0], seeds[1]: [50.0, 50.0]}


@pytest.mark.parametrize("K", [1, 3])
def test_without_checkpoints_path_nothing_is_written(K, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _, _, _, dirs = drive(K, (2.0, 1.0))
    assert dirs == [None] * K and os.listdir(tmp_path) == []


@pytest.mark.parametrize("K", [1, 3])
def test_total_that_is_no_multiple_of_every(K):
    events, _, seeds, _ = drive(K, (2.0,), total=10)
    assert [e for e in events if e[0] == "steps"] == [("steps", 0, 4), ("steps", 4, 2), ("steps", 6, 4)]
    assert [e[2] for e in events if e[0] == "eval"] == [5] * K  # none at step 9
    # the last chunk's losses are flushed at the end
    assert events[-4 * K:] == loss_records(K, seeds, 6, 4)
    assert len([e for e in events if e[0] == "log" and "value_loss" in e[1]]) == 10 * K


@pytest.mark.parametrize("K", [1, 3])
def test_step_offset_moves_every_record_and_no_file_name(K, tmp_path):
    class Shifted(ol.BestModelRecords):
        step_offset = 7

    plain, *_ = drive(K, (2.0, 1.0), tmp_path / "plain")
    events, _, _, dirs = drive(K, (2.0, 1.0), tmp_path / "shifted", records=Shifted)
    assert any(e[0] == "log" and "value_loss" in e[1] for e in plain) and any("evaluation_return" in e[1] for e in plain
                                                                               if e[0] == "log")
    assert events == [("log", e[1], e[2] + 7) if e[0] == "log" else e for e in plain]
    # what a record says stays zero-based (best_step_so_far), and so do the files
    assert {e[1]["best_step_so_far"] for e in events if e[0] == "log" and "best_step_so_far" in e[1]} == {5}
    for d in dirs:
        assert sorted(f for f in os.listdir(d) if f.endswith(".pt")) == ["best_model.pt", "checkpoint_11.pt",
                                                                         "checkpoint_5.pt"]


def test_resume_generation_loop_entry_is_best_score_best_step_norm(tmp_path):
    # seed 0 never gets a normalized score, seed 1 gets 0.5 at step 5 (the calls: 0 and 1 at step 5, then at 11)
    err = ValueError("no reference score")
    _, _, _, dirs = drive(2, (3.0, 1.0), tmp_path, normalized=scripted([err, 0.5, err, err]), resume=True)
    step, payloads = _resume.latest(dirs)
    assert step == 12 and sorted(payloads) == [0, 1]
    loops = [payloads[k]["loop"] for k in (0, 1)]
    assert loops == [{"best_score": 3.0, "best_step": 5, "norm": None}, {"best_score": 50.0, "best_step": 5, "norm": 50.0}]
    for loop in loops:
        assert sorted(loop) == ["best_score", "best_step", "norm"]
        assert type(loop["best_score"]) is float and type(loop["best_step"]) is int
        assert loop["norm"] is None or type(loop["norm"]) is float


def test_a_generation_of_the_parent_format_restores_into_best_model_records(tmp_path):
    """The payload below is written by hand in the format of the commit before the recorders (``run`` built the
    ``"loop"`` entry itself there): ``BestModelRecords`` must take it as its own."""
    _resume.write(str(tmp_path), 6, {"finished": False, "trainer": {"done": 6}, "sampler": None,
                                     "loop": {"best_score": 40.0, "best_step": 5, "norm": 40.0}})
    # the evaluation at step 11 returns 90 and gets no normalized score: the kept 40 still counts, and 40 is not
    # beaten -- without the restored norm the raw 90 would be the best, without the restored best 40 would be new
    events, trainers, _, _ = drive(1, (None, 90.0), tmp_path, normalized=scripted([ValueError("no reference score")]),
                                   resume=True)
    assert [e for e in events if e[0] == "steps"] == [("steps", 6, 4), ("steps", 10, 2)] and trainers[0].done == 12
    assert evaluation_logs(events) == [(("evaluation_return", 90.0), 11), (("best_score_so_far", 40.0), 11),
                                       (("best_step_so_far", 5), 11)]
    assert "best_model.pt" not in os.listdir(tmp_path)
    assert _resume.latest([str(tmp_path)])[1][0]["loop"] == {"best_score": 40.0, "best_step": 5, "norm": 40.0}


def test_tag_and_print_logger(capsys, monkeypatch):
    import sys
    assert ol.tag([7])({"a": 1.0}, 0) == {"a": 1.0}
    assert ol.tag([7, 8])({"a": 1.0}, 1) == {"a": 1.0, "seed": 8}
    monkeypatch.setitem(sys.modules, "wandb", None)  # (import wandb raises ImportError)
    ol.default_logger(Config(), 1)({"q_loss": 0.25}, 3)
    assert capsys.readouterr().out == "[3] q_loss=0.25\n"
