"""The chunked train / evaluate / checkpoint loop of the custom-offline flavours (``custom_offline.train`` and
``train_runs``, ``custom_offline_br``, ``custom_offline_bb``), once, and the setup every ``train()`` shares: the
``sampler`` check, the seeds of a rank, the checkpoint directories, the default logger and the ``seed`` tag of
K > 1 records.  The offline flavour (``train``,
``sweep.train_runs``) takes that setup from here and runs ``_window_loop``: window means instead of every step's
losses, a metric exchange instead of a best model.

``run`` knows no trainer class, buffer or sampler: a flavour hands in how a group is built, how a chunk of steps
is queued and how one seed is evaluated.  Its members are the K seeds of one config (one step count and
evaluation period for all) or the runs of a sweep's launch batch (``custom_offline.train_runs``: one of each per
member).  ``Members`` is the group lifecycle of both loops: built over the members that start, rebuilt when one
leaves, closed at the end.  Nothing here touches the GPU or loads the library.
"""
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


def run(trainers: Sequence, seeds: Sequence[int], make_group: Callable, total: PerMember, every: PerMember,
        chunk: int, logger: Logger, ckpt_dirs: Sequence[Optional[str]], steps: Callable, evaluate: Callable,
        normalized: Union[None, Callable, Sequence[Optional[Callable]]] = None, best_by_return: bool = False, *,
        tagged: Optional[Callable] = None, resume: bool = False, sampler_state: Optional[Callable] = None,
        set_sampler_state: Optional[Callable] = None, loss_names: Sequence[str] = LOSS_NAMES,
        best_model: bool = True) -> None:
    """``total`` steps in chunks of at most ``chunk`` that end on the evaluation boundaries (every ``every``
    steps); the losses of a chunk come back to the host once, after the next chunk has been queued.

    ``make_group(active)`` builds what steps the members that start together (``multi.stepper``; None: nothing to
    synchronize or close); ``steps(group, active, t, n)`` queues steps t .. t + n - 1 and returns the loss tensors
    [n, 3] of the active members in member order; the group is synchronized before an evaluation (``Members``).
    ``evaluate(k, trainer, step)`` gives the returns of member k.  ``normalized(returns)``: the normalized
    scores, logged x 100 (one callable, or one per member); a ``ValueError`` from it keeps what the member had
    (at first the raw mean return), and a value once obtained stays.  The best model is the one of the
    strictly greatest normalized score, or mean return without one or with ``best_by_return``.  One
    ``logger(record, step)`` call per step and member for the losses, then per evaluation record;
    ``tagged(record, k)`` makes the record the logger gets (default: ``tag(seeds)``).

    ``loss_names``: the names of the columns of the loss tensors (default: the three losses of an IQL step;
    ``minari_bc`` logs one ``actor_loss``).  ``best_model=False``: no best-model bookkeeping -- no
    ``best_model.pt``, no ``best_score_so_far`` / ``best_step_so_far`` records (``minari_bc``: the reference's
    loop there has none); the default leaves every record as it was.

    ``total`` / ``every`` may be one entry per member (a sweep's runs): all members start at step 0, a chunk
    ends on the next evaluation boundary or end of ANY active member, and a member whose ``total`` is reached
    leaves after its evaluation: the group is synchronized and closed, and ``make_group`` is called with the
    member indices that go on (for none, nothing is built).  With scalars every member is active to the end.

    ``resume`` (every entry of ``ckpt_dirs`` must be a directory, else ValueError): at the end of every
    boundary at which a member evaluated or left -- after the evaluations, records and ``checkpoint_{step}.pt``
    files of all due members -- every member active in the chunk, due or not, writes one file of a resume
    generation (``_resume``) at the common step: its ``trainer.resume_state()``, ``sampler_state(k)`` (what
    its index sampler needs to stand where it stands now; ``steps`` draws exactly the steps it queues, so
    nothing is drawn ahead of the boundary), its best score and step, its kept normalized score and whether
    it has finished.  No loss record is pending then.  And the loop starts from the newest complete
    generation (``_resume.latest``) instead of step 0: every member is restored with
    ``trainer.load_resume_state`` and ``set_sampler_state(k, state)``, files of later, incomplete
    generations are removed, finished members are neither trained nor evaluated again, and ``make_group`` is
    first called after the restore, with the members that go on.  Without any generation the run starts at step
    0; members that hold generations of different steps and none in common were not interrupted together:
    ValueError, and their files stay (``_resume.restore``).  Without ``resume`` nothing of this happens and no
    such file is written."""
    K = len(trainers)
    totals, everys = spread(total, K), spread(every, K)
    norms = list(normalized) if isinstance(normalized, (list, tuple)) else [normalized] * K
    if not len(totals) == len(everys) == len(norms) == K:
        raise ValueError("total / every / normalized: one entry per member")
    if tagged is None:
        tagged = tag(seeds)
    best_score, best_step = [-np.inf] * K, [0] * K
    norm = [None] * K
    pending = None  # (first step, members, their device losses) of the chunk whose records are still to be logged

    def flush():
        nonlocal pending
        if pending is None:
            return
        t0, members, losses = pending
        pending = None
        for k, arr in zip(members, (l.cpu().numpy() for l in losses)):
            for i, row in enumerate(arr.tolist()):
                logger(tagged(dict(zip(loss_names, row)), k), t0 + i)

    t = 0
    finished = set()
    kept: Dict[int, int] = {}  # member -> step of the generation file it holds
    if resume:
        t, payloads = _resume.restore(ckpt_dirs, kept, [k for k in range(K) if totals[k] > 0])
        for k, p in payloads.items():
            trainers[k].load_resume_state(p["trainer"])
            if set_sampler_state is not None:
                set_sampler_state(k, p["sampler"])
            best_score[k], best_step[k], norm[k] = p["loop"]["best_score"], p["loop"]["best_step"], p["loop"]["norm"]
            if p["finished"]:
                finished.add(k)

    def commit(members):
        flush()
        payloads = {k: {"finished": t >= totals[k], "trainer": trainers[k].resume_state(),
                        "sampler": None if sampler_state is None else sampler_state(k),
                        "loop": {"best_score": float(best_score[k]), "best_step": int(best_step[k]),
                                 "norm": None if norm[k] is None else float(norm[k])}} for k in members}
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
                trainer = trainers[k]
                log = lambda d: logger(tagged(d, k), step)
                eval_scores = evaluate(k, trainer, step)
                mean_eval = eval_scores.mean()
                log({"evaluation_return": mean_eval})
                if norms[k] is not None:
                    try:
                        norm[k] = np.asarray(norms[k](eval_scores)).mean() * 100
                        log({"normalized_score": norm[k]})
                    except ValueError:
                        pass
                score = norm[k] if norm[k] is not None and not best_by_return else mean_eval
                if best_model and score > best_score[k]:
                    best_score[k], best_step[k] = score, step
                    if ckpt_dirs[k] is not None:
                        torch.save(trainer.state_dict(), os.path.join(ckpt_dirs[k], "best_model.pt"))
                if best_model:
                    log({"best_score_so_far": best_score[k]})
                    log({"best_step_so_far": best_step[k]})
                if ckpt_dirs[k] is not None:
                    torch.save(trainer.state_dict(), os.path.join(ckpt_dirs[k], f"checkpoint_{step}.pt"))
            left = [k for k in active if t < totals[k]]
            if resume and live.commit_due(due, left):
                commit(active)
            live.keep(left)
    flush()
