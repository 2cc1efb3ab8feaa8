"""The chunked train / evaluate / checkpoint loop of every offline ``train()`` but the window loop's
(``custom_offline.train`` and ``train_runs``, ``custom_offline_br``, ``custom_offline_bb``, ``minari_iql``,
``minari_bc``, ``offline_bc``, ``awac``, ``td3_bc``), once, and the setup every ``train()`` shares: the ``sampler`` check, the
seeds of a rank, the checkpoint directories, the default logger and the ``seed`` tag of K > 1 records.  The
offline flavour (``train``, ``sweep.train_runs``) takes that setup from here and runs ``_window_loop``: window
means instead of every step's losses, a metric exchange instead of a best model.

``run`` knows no trainer class, buffer or sampler, and no record name: a flavour hands in how a group is built,
how a chunk of steps is queued, how one seed is evaluated and a ``Records`` that logs what the flavour logs
(``EvalRecords``, ``BestModelRecords``, or its own).  Its members are the K seeds of one config (one step count and
evaluation period for all) or the runs of a sweep's launch batch (``custom_offline.train_runs``: one of each per
member).  ``Members`` is the group lifecycle of both loops: built over the members that start, rebuilt when one
leaves, closed at the end.  Nothing here touches the GPU or loads the library.
"""
import contextlib
import os
import uuid
from dataclasses import asdict
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _resume
from . import distributed as D
from ._lib import MAX_GROUP

Logger = Callable[[Dict[str, float], int], None]
PerMember = Union[int, Sequence[int]]  # one value for all members of a loop, or one per member
LOSS_NAMES = ("value_loss", "q_loss", "actor_loss")  # the columns of an IQL step's loss tensor


def check_sampler(sampler: str) -> None:
    if sampler not in ("host", "device"):
        raise ValueError("sampler must be 'host' or 'device'")


def group_seeds(train_seed: int, seeds_per_gpu: int) -> List[int]:
    """The seeds of the K runs of this rank: ``rank_seed(train_seed, K) + k``.  ValueError for a K no group holds."""
    K = int(seeds_per_gpu)
    if not 1 <= K <= MAX_GROUP:
        raise ValueError(f"seeds_per_gpu must be in 1..{MAX_GROUP}")
    first = D.rank_seed(train_seed, K)
    return [first + k for k in range(K)]


def checkpoint_dirs(config, seeds: Sequence[int], resume: bool = False) -> List[Optional[str]]:
    """The checkpoint directory of every seed (None each without ``config.checkpoints_path``): the path
    itself for one seed, ``seed_<seed>/`` under it for several.  Makes them and writes ``config.yaml``.
    ``resume``: first ``_resume.check_config`` -- ValueError without a ``checkpoints_path``, or when the
    ``config.yaml`` already there was written for another config (paths aside)."""
    if resume:
        _resume.check_config(config)
    if config.checkpoints_path is None:
        return [None] * len(seeds)
    print(f"Checkpoints path: {config.checkpoints_path}")
    os.makedirs(config.checkpoints_path, exist_ok=True)
    import yaml
    with open(os.path.join(config.checkpoints_path, "config.yaml"), "w") as f:
        yaml.safe_dump(asdict(config), f)
    if len(seeds) == 1:
        return [config.checkpoints_path]
    dirs = [os.path.join(config.checkpoints_path, f"seed_{s}") for s in seeds]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    return dirs


def default_logger(config, K: int, run_id: bool = True) -> Logger:
    """wandb when importable (one run, under a fresh uuid with ``run_id``; with K > 1 the records of seed s go
    under ``seed<s>/``, one without a ``seed`` under its own names), else print."""
    try:
        import wandb
        wandb.init(config=asdict(config), project=config.project, group=config.group, name=config.name,
                   **({"id": str(uuid.uuid4())} if run_id else {}))
    except ImportError:
        return lambda d, step: print(f"[{step}] " + " ".join(f"{n}={v:.5g}" for n, v in d.items()))
    if K == 1:
        return lambda d, step: wandb.log(d, step=step)
    return lambda d, step: wandb.log({(f"seed{int(d['seed'])}/{n}" if "seed" in d else n): v
                                      for n, v in d.items() if n != "seed"}, step=step)


def tag(seeds: Sequence[int]) -> Callable[[Dict[str, float], int], Dict[str, float]]:
    """``(record, k) -> record`` as the logger gets it: with several seeds it carries ``seed``."""
    if len(seeds) == 1:
        return lambda rec, k: rec
    return lambda rec, k: dict(rec, seed=seeds[k])


def spread(x, K: int) -> List[int]:
    """One int per member: ``x`` for all K of them, or its entries."""
    return [int(x)] * K if np.ndim(x) == 0 else [int(v) for v in x]


class Members:
    """The members a loop still trains (``active``) and what steps them together: ``group``, from
    ``make_group(active)`` -- None where there is nothing to synchronize or close, and for no member nothing is
    built.  As a context manager it dissolves the group at the end: synchronized and closed on a normal exit,
    only closed on an exception (``iqlhip_group_destroy`` waits for the device itself, and a ``synchronize``
    that fails must not mask the first error)."""

    def __init__(self, make_group: Callable[[List[int]], object], active: Sequence[int]):
        self._make, self.active = make_group, list(active)
        self.group = make_group(list(active)) if self.active else None

    def synchronize(self) -> None:
        if self.group is not None:
            self.group.synchronize()

    def commit_due(self, due: Sequence[int], left: Sequence[int]) -> bool:
        """Whether this boundary ends with a resume generation: a member evaluated or left.  If so the members
        can be read when this returns (no evaluation has synchronized them: it is done here)."""
        gone = len(left) != len(self.active)
        if gone and not due:
            self.synchronize()
        return bool(due) or gone

    def keep(self, left: Sequence[int]) -> None:
        """``left`` are the members that go on: if one has left, the group is synchronized, closed and rebuilt."""
        if len(left) != len(self.active):
            self.__exit__()
            self.active = list(left)
            self.group = self._make(list(left)) if self.active else None

    def __enter__(self):
        return self

    def __exit__(self, exc_type=None, exc=None, tb=None):
        group, self.group = self.group, None
        if group is not None:
            if exc_type is None:
                group.synchronize()
            group.close()


class Records:
    """What a flavour logs under ``run``.  ``loss_names``: the columns of the loss tensors.  ``step_offset`` is
    added to the zero-based step of every record, losses and evaluations alike, never to a file name.
    ``evaluated`` logs member k's evaluation through ``log(record)``, bound by ``run`` to the member's tag and to
    ``step + step_offset``.  For ``resume``, ``state(k)`` / ``load_state(k, state)``: member k's ``"loop"`` entry."""
    loss_names: Sequence[str] = LOSS_NAMES
    step_offset = 0

    def loss_record(self, k: int, row: Sequence[float], step: int) -> Dict[str, float]:
        """The loss record of member k at the zero-based ``step`` from its row of the loss tensor (a flavour whose
        steps do not all log every column overrides this; it is logged at ``step + step_offset``)."""
        return dict(zip(self.loss_names, row))

    def evaluated(self, k: int, trainer, step: int, returns: np.ndarray, log: Callable) -> None:
        raise NotImplementedError


class EvalRecords(Records):
    """``evaluation_return``, then ``normalized_score``: the mean of ``normalized(returns)`` (one callable, or one
    per member) x 100.  A ``ValueError`` from it logs nothing and keeps ``norm[k]``.  ``minari_bc``'s recorder."""

    def __init__(self, normalized=None, loss_names: Sequence[str] = LOSS_NAMES):
        self.normalized, self.loss_names = normalized, loss_names
        self.norm: Dict[int, Optional[float]] = {}

    def evaluated(self, k, trainer, step, returns, log):
        log({"evaluation_return": returns.mean()})
        normalized = self.normalized[k] if isinstance(self.normalized, (list, tuple)) else self.normalized
        if normalized is not None:
            with contextlib.suppress(ValueError):
                self.norm[k] = np.asarray(normalized(returns)).mean() * 100
                log({"normalized_score": self.norm[k]})


class BestModelRecords(EvalRecords):
    """``EvalRecords`` plus the best model of every member -- that of the strictly greatest kept normalized score,
    or mean return without one or with ``best_by_return`` --, saved as ``best_model.pt`` into ``ckpt_dirs[k]``
    (None: nowhere) ahead of ``best_score_so_far`` and ``best_step_so_far``.  The custom-offline flavours' recorder."""

    def __init__(self, ckpt_dirs: Sequence[Optional[str]], normalized=None, best_by_return: bool = False):
        super().__init__(normalized)
        self.ckpt_dirs, self.best_by_return = ckpt_dirs, best_by_return
        self.best_score, self.best_step = [-np.inf] * len(ckpt_dirs), [0] * len(ckpt_dirs)

    def evaluated(self, k, trainer, step, returns, log):
        super().evaluated(k, trainer, step, returns, log)
        norm = self.norm.get(k)
        score = norm if norm is not None and not self.best_by_return else returns.mean()
        if score > self.best_score[k]:
            self.best_score[k], self.best_step[k] = score, step
            if self.ckpt_dirs[k] is not None:
                torch.save(trainer.state_dict(), os.path.join(self.ckpt_dirs[k], "best_model.pt"))
        log({"best_score_so_far": self.best_score[k]})
        log({"best_step_so_far": self.best_step[k]})

    def state(self, k):
        norm = self.norm.get(k)
        return {"best_score": float(self.best_score[k]), "best_step": int(self.best_step[k]),
                "norm": None if norm is None else float(norm)}

    def load_state(self, k, state):
        self.best_score[k], self.best_step[k], self.norm[k] = state["best_score"], state["best_step"], state["norm"]


def run(trainers: Sequence, seeds: Sequence[int], make_group: Callable, total: PerMember, every: PerMember,
        chunk: int, logger: Logger, ckpt_dirs: Sequence[Optional[str]], steps: Callable, evaluate: Callable,
        records: Records, *, tagged: Optional[Callable] = None, resume: bool = False,
        sampler_state: Optional[Callable] = None, set_sampler_state: Optional[Callable] = None) -> None:
    """``total`` steps in chunks of at most ``chunk`` that end on the evaluation boundaries (every ``every``
    steps); the losses of a chunk come back to the host once, after the next chunk has been queued.

    ``make_group(active)`` builds what steps the members that start together (``multi.stepper``; None: nothing to
    synchronize or close); ``steps(group, active, t, n)`` queues steps t .. t + n - 1 and returns the loss tensors
    [n, len(records.loss_names)] of the active members in member order; the group is synchronized before an
    evaluation (``Members``).  ``evaluate(k, trainer, step)`` gives the returns of member k.

    The loop schedules, ``records`` (a ``Records``) names and logs: one ``logger(record, step)`` call per step and
    member for the losses; at a boundary, per due member in member order, ``evaluate``, ``records.evaluated`` --
    that flavour's evaluation records and best model, if it keeps one -- and ``checkpoint_{step}.pt``.
    ``tagged(record, k)`` makes the record the logger gets (default: ``tag(seeds)``).

    ``total`` / ``every`` may be one entry per member (a sweep's runs): all members start at step 0, a chunk
    ends on the next evaluation boundary or end of ANY active member, and a member whose ``total`` is reached
    leaves after its evaluation: the group is synchronized and closed, and ``make_group`` is called with the
    member indices that go on (for none, nothing is built).  With scalars every member is active to the end.

    ``resume`` (every entry of ``ckpt_dirs`` must be a directory, else ValueError): at the end of every
    boundary at which a member evaluated or left -- after the evaluations, records and ``checkpoint_{step}.pt``
    files of all due members -- every member active in the chunk, due or not, writes one file of a resume
    generation (``_resume``) at the common step: its ``trainer.resume_state()``, ``sampler_state(k)`` (what
    its index sampler needs to stand where it stands now; ``steps`` draws exactly the steps it queues, so
    nothing is drawn ahead of the boundary), ``records.state(k)`` (its best score and step, its kept normalized
    score) and whether it has finished.  No loss record is pending then.  And the loop starts from the newest
    complete generation (``_resume.latest``) instead of step 0: every member is restored with
    ``trainer.load_resume_state``, ``set_sampler_state(k, state)`` and ``records.load_state(k, state)``, files of
    later, incomplete generations are removed, finished members are neither trained nor evaluated again, and
    ``make_group`` is first called after the restore, with the members that go on.  Without any generation the
    run starts at step 0; members that hold generations of different steps and none in common were not
    interrupted together: ValueError, and their files stay (``_resume.restore``).  Without ``resume`` nothing of
    this happens and no such file is written."""
    K = len(trainers)
    totals, everys = spread(total, K), spread(every, K)
    if not len(totals) == len(everys) == K:
        raise ValueError("total / every: one entry per member")
    if tagged is None:
        tagged = tag(seeds)
    offset = int(records.step_offset)
    pending = None  # (first step, members, their device losses) of the chunk whose records are still to be logged

    def flush():
        nonlocal pending
        if pending is None:
            return
        t0, members, losses = pending
        pending = None
        for k, arr in zip(members, (l.cpu().numpy() for l in losses)):
            for i, row in enumerate(arr.tolist(), t0):
                logger(tagged(records.loss_record(k, row, i), k), i + offset)

    t = 0
    finished = set()
    kept: Dict[int, int] = {}  # member -> step of the generation file it holds
    if resume:
        t, payloads = _resume.restore(ckpt_dirs, kept, [k for k in range(K) if totals[k] > 0])
        for k, p in payloads.items():
            trainers[k].load_resume_state(p["trainer"])
            if set_sampler_state is not None:
                set_sampler_state(k, p["sampler"])
            records.load_state(k, p["loop"])
            if p["finished"]:
                finished.add(k)

    def commit(members):
        flush()
        payloads = {k: {"finished": t >= totals[k], "trainer": trainers[k].resume_state(),
                        "sampler": None if sampler_state is None else sampler_state(k),
                        "loop": records.state(k)} for k in members}
        _resume.commit(ckpt_dirs, t, payloads, kept)

    with Members(make_group, [k for k in range(K) if t < totals[k] and k not in finished]) as live:
        while live.active:
            active = live.active
            nxt = min(t + int(chunk), *[min(totals[k], (t // everys[k] + 1) * everys[k]) for k in active])
            losses = steps(live.group, list(active), t, nxt - t)
            flush()
            pending = (t, list(active), losses)
            t = nxt
            due = [k for k in active if t % everys[k] == 0]
            if due:
                flush()
                live.synchronize()
            step = t - 1
            for k in due:
                returns = evaluate(k, trainers[k], step)
                records.evaluated(k, trainers[k], step, returns, lambda d: logger(tagged(d, k), step + offset))
                if ckpt_dirs[k] is not None:
                    torch.save(trainers[k].state_dict(), os.path.join(ckpt_dirs[k], f"checkpoint_{step}.pt"))
            left = [k for k in active if t < totals[k]]
            if resume and live.commit_due(due, left):
                commit(active)
            live.keep(left)
    flush()
