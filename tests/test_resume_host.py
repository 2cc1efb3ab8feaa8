"""Resume generations on the host: ``_offline_loop.run(resume=True)`` over stub trainers (the state is a
counter) and a stub sampler (a counter of draws), the config checks, and ``--list --resume``.  No GPU, no
library load.

An interruption is an exception raised from the injected ``evaluate`` callback, or from ``_resume.write``
(between two members' files).  The contract checked everywhere: the records of the first part up to its last
committed generation, followed by the records of the resumed part, are the uninterrupted run's records; the
files, the trainers and the samplers end as the uninterrupted run's do.
"""
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

from iqlpref_amd import _offline_loop as ol
from iqlpref_amd import _resume


@dataclass
class Config:
    name: str = "fake"
    beta: float = 3.0
    reward_model_path: str = "somewhere"
    checkpoints_path: Optional[str] = None


class Trainer:
    """The state is a counter of steps done and a running sum that depends on every index ever drawn."""

    def __init__(self, k):
        self.k, self.done, self.acc, self.actor = k, 0, 0.0, object()

    def state_dict(self):
        return {"w": torch.tensor([float(self.k), float(self.done), self.acc], dtype=torch.float64)}

    def resume_state(self):
        return {"done": self.done, "acc": self.acc}

    def load_resume_state(self, state):
        self.done, self.acc = state["done"], state["acc"]


class Interrupt(Exception):
    pass


class World:
    """Trainers, per-member samplers (a counter of draws: draw number c of member k is 7 c + k) and everything
    observable of one ``run`` call."""

    def __init__(self, K, path, totals, everys):
        self.K, self.totals, self.everys = K, totals, everys
        self.trainers = [Trainer(k) for k in range(K)]
        self.draws = [0] * K
        self.records, self.evals, self.regroups = [], [], []  # regroups: the members of every make_group call
        self.seeds = [40 + k for k in range(K)]
        self.dirs = [os.path.join(str(path), f"run{k}") for k in range(K)]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)

    def steps(self, group, active, t, n):
        assert group is None and active == self.regroups[-1]
        out = []
        for k in active:
            tr, rows = self.trainers[k], []
            assert tr.done == t, "a member is stepped from the common step"
            for _ in range(n):
                tr.acc = 0.5 * tr.acc + (7 * self.draws[k] + k)
                self.draws[k] += 1
                tr.done += 1
                rows.append([tr.acc, float(tr.done), float(k)])
            out.append(torch.tensor(rows, dtype=torch.float64))
        return out

    def make_group(self, active):
        self.regroups.append(list(active))
        return None

    def run(self, resume, stop_at=None, chunk=4):
        """``stop_at`` = (k, step): the evaluation of member k at that step raises."""
        def evaluate(k, trainer, step):
            if stop_at == (k, step):
                raise Interrupt(f"member {k} at step {step}")
            self.evals.append((k, step))
            return np.array([trainer.acc - step, trainer.acc + k])

        ol.run(self.trainers, self.seeds, self.make_group, self.totals, self.everys, chunk,
               lambda rec, step: self.records.append((dict(rec), step)), self.dirs, self.steps, evaluate,
               ol.BestModelRecords(self.dirs, lambda scores: scores / 8.0), resume=resume,
               sampler_state=lambda k: {"draws": self.draws[k]},
               set_sampler_state=lambda k, st: self.draws.__setitem__(k, st["draws"]))
        return self

    def files(self):
        return {os.path.join(f"run{k}", f): torch.load(os.path.join(d, f), weights_only=True)
                for k, d in enumerate(self.dirs) for f in sorted(os.listdir(d))}

    def final(self):
        return [(tr.done, tr.acc) for tr in self.trainers], list(self.draws)


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def committed(records, t):
    """The records of a first part up to its generation at step t (losses are logged at the 0-based step,
    evaluations at t - 1)."""
    return [(rec, step) for rec, step in records if step < t]


def check_resumed(first, second, whole, t):
    assert committed(first.records, t) + second.records == whole.records
    assert second.final() == whole.final()
    got, want = second.files(), whole.files()
    assert list(got) == list(want)
    assert all(same(got[f], want[f]) for f in want)
    assert not any(f.endswith(_resume.TMP_SUFFIX) for f in got)


TOTALS, EVERYS = [12, 24, 18], [6, 12, 6]


def whole_run(tmp_path, K=3, totals=TOTALS, everys=EVERYS, resume=True):
    return World(K, tmp_path / "whole", totals[:K], everys[:K]).run(resume)


def test_interrupt_at_a_boundary(tmp_path):
    whole = whole_run(tmp_path)
    first = World(3, tmp_path / "cut", TOTALS, EVERYS)
    with pytest.raises(Interrupt):
        first.run(True, stop_at=(0, 11))  # generation 6 is committed, the boundary at 12 is not
    assert [_resume.steps_in(d) for d in first.dirs] == [[6], [6], [6]]
    second = World(3, tmp_path / "cut", TOTALS, EVERYS).run(True)
    check_resumed(first, second, whole, 6)
    assert second.evals[0] == (0, 11) and second.regroups == whole.regroups == [[0, 1, 2], [1, 2], [1]]
    # what the finished run leaves: every member's final file, marked finished, at its own last step
    assert [_resume.steps_in(d) for d in second.dirs] == [[12], [24], [18]]
    assert [_resume.status(d) for d in second.dirs] == ["done"] * 3


def test_interrupt_between_two_members_file_writes(tmp_path, monkeypatch):
    whole = whole_run(tmp_path)
    first = World(3, tmp_path / "cut", TOTALS, EVERYS)
    real, calls = _resume.write, []

    def write(directory, step, payload):
        if step == 12 and len([c for c in calls if c == 12]) == 1:
            raise Interrupt("between member 0's file and member 1's")
        calls.append(step)
        return real(directory, step, payload)

    monkeypatch.setattr(_resume, "write", write)
    with pytest.raises(Interrupt):
        first.run(True)
    monkeypatch.setattr(_resume, "write", real)
    # generation 12 is half there (member 0 only), generation 6 is still whole
    assert [_resume.steps_in(d) for d in first.dirs] == [[6, 12], [6], [6]]
    found = _resume.latest(first.dirs)
    assert found[0] == 6 and not found[1][0]["finished"]
    second = World(3, tmp_path / "cut", TOTALS, EVERYS).run(True)
    check_resumed(first, second, whole, 6)
    assert (0, 11) in second.evals  # member 0 was NOT taken as finished from its stale file of step 12


def test_a_half_written_file_is_no_generation(tmp_path):
    first = World(3, tmp_path / "cut", TOTALS, EVERYS)
    with pytest.raises(Interrupt):
        first.run(True, stop_at=(2, 17))  # generations 6 and 12 were committed, 12 is the one kept
    assert _resume.latest(first.dirs)[0] == 12
    with open(_resume.file_of(first.dirs[1], 12), "r+b") as f:
        f.truncate(100)
    with open(_resume.file_of(first.dirs[2], 18) + _resume.TMP_SUFFIX, "wb") as f:
        f.write(b"half")
    assert _resume.latest(first.dirs) is None  # (the generation before 12 is gone: from step 0 then)
    second = World(3, tmp_path / "cut", TOTALS, EVERYS).run(True)
    whole = whole_run(tmp_path)
    assert second.records == whole.records and second.final() == whole.final()
    assert not any(f.endswith(_resume.TMP_SUFFIX) for f in second.files())


def test_a_finished_member_is_not_evaluated_again(tmp_path):
    whole = whole_run(tmp_path)
    first = World(3, tmp_path / "cut", TOTALS, EVERYS)
    with pytest.raises(Interrupt):
        first.run(True, stop_at=(2, 17))  # member 0 finished at step 12
    assert _resume.status(first.dirs[0]) == "done" and _resume.status(first.dirs[1]) == "at step 12"
    second = World(3, tmp_path / "cut", TOTALS, EVERYS).run(True)
    check_resumed(first, second, whole, 12)
    assert all(k != 0 for k, _ in second.evals) and second.evals[0] == (2, 17)
    assert second.regroups == [[1, 2], [1]]  # rebuilt over the members still active, then member 2 leaves
    assert second.trainers[0].done == 12  # the returned trainer: loaded from its final state, not stepped
    # a run that is finished altogether does nothing at all
    third = World(3, tmp_path / "cut", TOTALS, EVERYS).run(True)
    assert third.records == [] and third.evals == [] and third.final() == whole.final()


def test_members_that_are_not_due_write_their_file_too(tmp_path):
    """every = 6 / 12 / 6: at step 6 member 1 is not due, at step 18 it is not either; a total that is no
    multiple of every (member 0: 9 of 6) ends without an evaluation and still leaves its finished file."""
    totals, everys = [9, 24, 18], [6, 12, 6]
    whole = World(3, tmp_path / "whole", totals, everys).run(True)
    first = World(3, tmp_path / "cut", totals, everys)
    with pytest.raises(Interrupt):
        first.run(True, stop_at=(2, 11))
    assert [_resume.steps_in(d) for d in first.dirs] == [[9], [9], [9]]
    assert _resume.read(first.dirs[0], 9)["finished"] and not _resume.read(first.dirs[1], 9)["finished"]
    second = World(3, tmp_path / "cut", totals, everys).run(True)
    check_resumed(first, second, whole, 9)
    assert second.regroups[0] == [1, 2] and all(k != 0 for k, _ in second.evals)


def test_resume_without_checkpoints_path_raises(tmp_path):
    with pytest.raises(ValueError, match="checkpoints_path"):
        ol.checkpoint_dirs(Config(), [0], resume=True)
    w = World(2, tmp_path, [6, 6], [6, 6])
    w.dirs = [w.dirs[0], None]
    with pytest.raises(ValueError, match="checkpoint directory"):
        w.run(True)
    assert w.records == []


def test_a_changed_config_raises(tmp_path):
    path = str(tmp_path / "run")
    assert ol.checkpoint_dirs(Config(checkpoints_path=path), [0], resume=True) == [path]
    ol.checkpoint_dirs(Config(checkpoints_path=path), [0], resume=True)  # the same config again
    # paths may differ: the directory was moved, the reward model lies elsewhere
    os.rename(path, path + "_moved")
    ol.checkpoint_dirs(Config(checkpoints_path=path + "_moved", reward_model_path="elsewhere", name="other"), [0],
                       resume=True)
    with pytest.raises(ValueError, match="beta"):
        ol.checkpoint_dirs(Config(checkpoints_path=path + "_moved", beta=5.0), [0], resume=True)
    # (and the refused start did not overwrite the config.yaml of the run that is there)
    assert _resume.saved_config(path + "_moved")["beta"] == 3.0
    ol.checkpoint_dirs(Config(checkpoints_path=path + "_moved", beta=5.0), [0])  # without resume: as before


def test_without_resume_the_directory_listing_is_todays(tmp_path):
    w = World(2, tmp_path, [12, 12], [6, 6]).run(False)
    for d in w.dirs:
        assert sorted(os.listdir(d)) == ["best_model.pt", "checkpoint_11.pt", "checkpoint_5.pt"]
    with_resume = World(2, tmp_path / "r", [12, 12], [6, 6]).run(True)
    assert with_resume.records == w.records and with_resume.final() == w.final()
    for d in with_resume.dirs:
        assert sorted(os.listdir(d)) == ["best_model.pt", "checkpoint_11.pt", "checkpoint_5.pt", "resume_12.done.pt"]
    path = str(tmp_path / "one")
    ol.checkpoint_dirs(Config(checkpoints_path=path), [0, 1])
    assert sorted(os.listdir(path)) == ["config.yaml", "seed_0", "seed_1"]


# kind of sweep file -> (seed field, step-count field, the line that names the flavour)
SWEEPS = {"offline": ("seed", "max_timesteps", ""),
          "custom": ("train_seed", "update_steps", "program: algorithms/custom_offline/iql.py\n")}


@pytest.mark.parametrize("kind", sorted(SWEEPS))
def test_list_resume_prints_done_partial_and_new(kind, tmp_path, capsys):
    from iqlpref_amd import sweep as sw
    seed_field, steps_field, program = SWEEPS[kind]
    sweep_file = tmp_path / "sweep.yaml"
    sweep_file.write_text(f"{program}method: grid\nparameters:\n  {seed_field}:\n    values: [0, 1, 2]\n"
                          f"  {steps_field}:\n    value: 40\n")
    base = str(tmp_path / "ck")
    # an earlier start of the same sweep: run 0 finished, run 1 got to step 20, run 2 never began
    earlier = sw.expand_sweep(str(sweep_file), checkpoints_path=base)
    for cfg, (step, finished) in zip(earlier[:2], ((40, True), (20, False))):
        d = ol.checkpoint_dirs(cfg, [0])[0]
        _resume.write(d, step, {"finished": finished, "trainer": {}, "sampler": None, "loop": {}})
    capsys.readouterr()
    cuda_before = torch.cuda.is_initialized()
    sw.main([str(sweep_file), "--list", "--resume", "--checkpoints_path", base])
    lines = capsys.readouterr().out.strip().splitlines()
    assert [line.split("\t")[0] for line in lines] == ["0", "1", "2"]
    assert [line.split("\t")[-1] for line in lines] == ["done", "at step 20", "new"]
    assert torch.cuda.is_initialized() == cuda_before  # no GPU touched
    sw.main([str(sweep_file), "--list", "--checkpoints_path", base])  # without --resume: the lines of before
    assert all(line.split("\t")[-1].startswith("batch") for line in capsys.readouterr().out.strip().splitlines())
    # another sweep value: none of the earlier runs is this config's
    sw.main([str(sweep_file), "--list", "--resume", "--checkpoints_path", base, f"--{steps_field}", "50"])
    assert [line.split("\t")[-1] for line in capsys.readouterr().out.strip().splitlines()] == ["new"] * 3


def test_two_generations_kept_and_the_newest_below_a_bound(tmp_path):
    """What the ranks of one job use: the generation before stays, and ``latest`` can be asked for the newest
    generation at or below the step the other ranks have."""
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        os.makedirs(d)
    kept = {}
    payload = lambda: {"finished": False, "trainer": {}, "sampler": None, "loop": {}}
    for t in (10, 20, 30):
        _resume.commit(dirs, t, {0: payload(), 1: payload()}, kept, keep_previous=True)
    assert [_resume.steps_in(d) for d in dirs] == [[20, 30]] * 2 and kept == {0: 30, 1: 30}
    assert _resume.latest(dirs)[0] == 30 and _resume.latest(dirs, at_most=29)[0] == 20
    assert _resume.latest(dirs, at_most=19) is None
    os.remove(_resume.file_of(dirs[1], 30))  # this rank died between its two files of generation 30
    assert _resume.latest(dirs)[0] == 20
    _resume.clean(dirs, {0: 20, 1: 20})
    assert [_resume.steps_in(d) for d in dirs] == [[20]] * 2


def test_command_line_finds_the_directory_of_its_earlier_start(tmp_path):
    """A config made anew has a fresh random name: ``adopt_run_dir`` takes the directory of the same config
    (paths aside) that holds a generation -- of this rank's seeds, of several the one that got furthest."""
    from iqlpref_amd.iql import TrainConfig
    base = str(tmp_path / "ck")
    payload = lambda seed: {"finished": False, "trainer": {"seed": seed}, "sampler": None, "loop": {}}
    made = []
    for seed, step in ((0, 10), (0, 30), (1, 20), (None, None)):
        cfg = TrainConfig(checkpoints_path=base, beta=3.0)
        d = ol.checkpoint_dirs(cfg, [0])[0]
        if step is not None:
            _resume.write(d, step, payload(seed))
        made.append(cfg)
    again = TrainConfig(checkpoints_path=base, beta=3.0)
    assert again.checkpoints_path not in [c.checkpoints_path for c in made]
    assert _resume.adopt_run_dir(again, seeds=[0])
    assert (again.checkpoints_path, again.name) == (made[1].checkpoints_path, made[1].name)
    rank1 = TrainConfig(checkpoints_path=base, beta=3.0)
    assert _resume.adopt_run_dir(rank1, seeds=[1]) and rank1.checkpoints_path == made[2].checkpoints_path
    other = TrainConfig(checkpoints_path=base, beta=5.0)
    before = other.checkpoints_path
    assert not _resume.adopt_run_dir(other) and other.checkpoints_path == before
    assert not _resume.adopt_run_dir(TrainConfig(checkpoints_path=base, beta=3.0), seeds=[7])
    ol.checkpoint_dirs(again, [0], resume=True)  # the adopted directory passes the config check


def test_runs_of_a_pen_sweep_that_differ_in_the_reward_model_path_alone(tmp_path, capsys):
    """The ten runs of a pen sweep differ in ``reward_model_path`` and nothing else: every run finds the directory
    of ITS earlier start, no directory goes to two runs, and a run without an earlier start stays new."""
    from iqlpref_amd import sweep as sw
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pen_sweeps")
    sweep_file = os.path.join(golden, "sweep_pen_human_pt.yaml")
    base = str(tmp_path / "ck")
    earlier = sw.expand_sweep(sweep_file, config_root=golden, checkpoints_path=base)
    assert len(earlier) == 10 and len({c.reward_model_path for c in earlier}) == 10
    others = [{k: v for k, v in _resume.config_dict(c).items() if k not in ("name", "checkpoints_path",
                                                                           "reward_model_path")} for c in earlier]
    assert all(o == others[0] for o in others)
    state = {2: (10, False), 5: (30, False), 7: (20, True)}
    for i, (step, finished) in state.items():
        d = ol.checkpoint_dirs(earlier[i], [earlier[i].train_seed])[0]
        _resume.write(d, step, {"finished": finished, "trainer": {}, "sampler": None, "loop": {}})
    again = sw.expand_sweep(sweep_file, config_root=golden, checkpoints_path=base)
    taken = set()
    adopted = [_resume.adopt_run_dir(c, taken=taken) for c in again]
    assert adopted == [i in state for i in range(10)]
    for i in state:
        assert again[i].checkpoints_path == earlier[i].checkpoints_path and again[i].name == earlier[i].name
    assert len({c.checkpoints_path for c in again}) == 10
    capsys.readouterr()
    sw.main([sweep_file, "--config_root", golden, "--list", "--resume", "--checkpoints_path", base])
    lines = capsys.readouterr().out.strip().splitlines()
    want = {2: "at step 10", 5: "at step 30", 7: "done"}
    assert [line.split("\t")[-1] for line in lines] == [want.get(i, "new") for i in range(10)]
    # two earlier starts of ONE config: the two runs of an invocation that are that config get one each
    twice = [earlier[5], sw.expand_sweep(sweep_file, config_root=golden, checkpoints_path=base)[5]]
    _resume.write(ol.checkpoint_dirs(twice[1], [0])[0], 10, {"finished": False, "trainer": {}, "sampler": None,
                                                            "loop": {}})
    fresh = [sw.expand_sweep(sweep_file, config_root=golden, checkpoints_path=base)[5] for _ in range(3)]
    taken = set()
    assert [_resume.adopt_run_dir(c, taken=taken) for c in fresh] == [True, True, False]
    assert [c.checkpoints_path for c in fresh[:2]] == [twice[0].checkpoints_path, twice[1].checkpoints_path]


def test_members_without_a_common_generation_are_refused_and_keep_their_files(tmp_path):
    """Members that were interrupted in different batches hold files of different steps: starting them at step
    0 would delete hours of evaluations, so the loop refuses and removes nothing."""
    first = World(3, tmp_path / "cut", TOTALS, EVERYS)
    with pytest.raises(Interrupt):
        first.run(True, stop_at=(0, 11))  # all three at step 6
    os.rename(_resume.file_of(first.dirs[1], 6), _resume.file_of(first.dirs[1], 8))  # (as if of another batch)
    before = [sorted(os.listdir(d)) for d in first.dirs]
    second = World(3, tmp_path / "cut", TOTALS, EVERYS)
    with pytest.raises(ValueError, match="no generation in common"):
        second.run(True)
    assert [sorted(os.listdir(d)) for d in first.dirs] == before and second.records == []


def test_a_file_that_cannot_be_read_is_an_error_not_an_absent_file(tmp_path, monkeypatch):
    d = str(tmp_path)
    _resume.write(d, 10, {"finished": False, "trainer": {}, "sampler": None, "loop": {}})
    assert _resume.read(d, 10)["step"] == 10 and _resume.read(d, 20) is None
    os.rename(_resume.file_of(d, 10), _resume.file_of(d, 12))
    with pytest.raises(ValueError, match="step 12"):
        _resume.read(d, 12)
    os.rename(_resume.file_of(d, 12), _resume.file_of(d, 10))

    def refuse(*a, **k):
        raise PermissionError("no access")

    monkeypatch.setattr(torch, "load", refuse)
    with pytest.raises(PermissionError):
        _resume.latest([d])
    monkeypatch.undo()
    with open(_resume.file_of(d, 10), "r+b") as f:
        f.truncate(64)
    assert _resume.read(d, 10) is None  # cut short: as good as not there


def test_the_bayesian_reward_flavour_refuses_resume():
    from iqlpref_amd import custom_offline_br as br
    with pytest.raises(NotImplementedError, match="does not resume"):
        br.train(br.TrainConfig(), resume=True)
