"""The chunked train / evaluate / checkpoint loop of the custom-offline flavours (``custom_offline.train`` and
``train_runs``, ``custom_offline_br``, ``custom_offline_bb``), once, and the setup every ``train()`` shares: the
checkpoint directories, the default logger and the ``seed`` tag of K > 1 records.  The offline flavour (``train``,
``sweep.train_runs``) takes that setup from here and runs ``_window_loop``: window means instead of every step's
losses, a metric exchange instead of a best model.

``run`` knows no trainer class, buffer or sampler: a flavour hands in how a chunk of steps is queued and how
one seed is evaluated.  Its members are the K seeds of one config (one step count and evaluation period for all)
or the runs of a sweep's launch batch (``custom_offline.train_runs``: one of each per member, and a hook that
rebuilds the group when a member leaves).  Nothing here touches the GPU or loads the library.
"""
import os
import uuid
from dataclasses import asdict
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _resume

Logger = Callable[[Dict[str, float], int], None]


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


def default_logger(config, K: int) -> Logger:
    """wandb when importable (one run; with K > 1 the records of seed s go under ``seed<s>/``), else print."""
    try:
        import wandb
        wandb.init(config=asdict(config), project=config.project, group=config.group, name=config.name,
                   id=str(uuid.uuid4()))
    except ImportError:
        return lambda d, step: print(f"[{step}] " + " ".join(f"{n}={v:.5g}" for n, v in d.items()))
    if K == 1:
        return lambda d, step: wandb.log(d, step=step)
    return lambda d, step: wandb.log({f"seed{int(d['seed'])}/{n}": v for n, v in d.items() if n != "seed"}, step=step)


def tag(seeds: Sequence[int]) -> Callable[[Dict[str, float], int], Dict[str, float]]:
    """``(record, k) -> record`` as the logger gets it: with several seeds it carries ``seed``."""
    if len(seeds) == 1:
        return lambda rec, k: rec
    return lambda rec, k: dict(rec, seed=seeds[k])


def run(trainers: Sequence, seeds: Sequence[int], group, total: Union[int, Sequence[int]],
        every: Union[int, Sequence[int]], chunk: int, logger: Logger, ckpt_dirs: Sequence[Optional[str]],
        steps: Callable[[int, int], List[torch.Tensor]], evaluate: Callable[[int, object, int], np.ndarray],
        normalized: Union[None, Callable, Sequence[Optional[Callable]]] = None, best_by_return: bool = False, *,
        regroup: Optional[Callable[[List[int]], object]] = None,
        tagged: Optional[Callable[[Dict[str, float], int], Dict[str, float]]] = None,
        resume: bool = False, sampler_state: Optional[Callable[[int], object]] = None,
        set_sampler_state: Optional[Callable[[int, object], None]] = None) -> None:
    """``total`` steps in chunks of at most ``chunk`` that end on the evaluation boundaries (every ``every``
    steps); the losses of a chunk come back to the host once, after the next chunk has been queued.

    ``steps(t, n)`` queues steps t .. t + n - 1 and returns the loss tensors [n, 3] of the active members in
    member order; ``group`` (a ``SeedGroup`` or None) is synchronized before an evaluation.
    ``evaluate(k, trainer, step)`` gives the returns of member k.  ``normalized(returns)``: the normalized
    scores, logged x 100 (one callable, or one per member); a ``ValueError`` from it keeps what the member had
    (at first the raw mean return), and a value once obtained stays.  The best model is the one of the
    strictly greatest normalized score, or mean return without one or with ``best_by_return``.  One
    ``logger(record, step)`` call per step and member for the losses, then per evaluation record;
    ``tagged(record, k)`` makes the record the logger gets (default: ``tag(seeds)``).

    ``total`` / ``every`` may be one entry per member (a sweep's runs): all members start at step 0, a chunk
    ends on the next evaluation boundary or end of ANY active member, and a member whose ``total`` is reached
    leaves after its evaluation.  ``regroup(active)`` is then called with the member indices that go on; it
    returns the group (or None) that ``steps`` drives from there.  With scalars every member is active to the
    end and ``regroup`` is never called.

    ``resume`` (every entry of ``ckpt_dirs`` must be a directory, else ValueError): at the end of every
    boundary at which a member evaluated or left -- after the evaluations, records and ``checkpoint_{step}.pt``
    files of all due members -- every member active in the chunk, due or not, writes one file of a resume
    generation (``_resume``) at the common step: its ``trainer.resume_state()``, ``sampler_state(k)`` (what
    its index sampler needs to stand where it stands now; ``steps`` draws exactly the steps it queues, so
    nothing is drawn ahead of the boundary), its best score and step, its kept normalized score and whether
    it has finished.  No loss record is pending then.  And the loop starts from the newest complete
    generation (``_resume.latest``) instead of step 0: every member is restored with
    ``trainer.load_resume_state`` and ``set_sampler_state(k, state)``, files of later, incomplete
    generations are removed, finished members are neither trained nor evaluated again, and ``regroup`` is
    handed the members that go on.  Without any generation the run starts at step 0; members that
    hold generations of different steps and none in common were not interrupted together: ValueError, and their
    files stay (``_resume.restore``).  Without ``resume``
    nothing of this happens and no such file is written."""
    K = len(trainers)
    totals = [int(total)] * K if np.ndim(total) == 0 else [int(x) for x in total]
    everys = [int(every)] * K if np.ndim(every) == 0 else [int(x) for x in every]
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
            for i, (v, q, a) in enumerate(arr.tolist()):
                logger(tagged({"value_loss": v, "q_loss": q, "actor_loss": a}, k), t0 + i)

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

    active = [k for k in range(K) if t < totals[k] and k not in finished]
    if len(active) != K and active and regroup is not None:
        group = regroup(list(active))
    while active:
        nxt = min(t + int(chunk), *[min(totals[k], (t // everys[k] + 1) * everys[k]) for k in active])
        losses = steps(t, nxt - t)
        flush()
        pending = (t, list(active), losses)
        t = nxt
        due = [k for k in active if t % everys[k] == 0]
        if due:
            flush()
            if group is not None:
                group.synchronize()
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
            if score > best_score[k]:
                best_score[k], best_step[k] = score, step
                if ckpt_dirs[k] is not None:
                    torch.save(trainer.state_dict(), os.path.join(ckpt_dirs[k], "best_model.pt"))
            log({"best_score_so_far": best_score[k]})
            log({"best_step_so_far": best_step[k]})
            if ckpt_dirs[k] is not None:
                torch.save(trainer.state_dict(), os.path.join(ckpt_dirs[k], f"checkpoint_{step}.pt"))
        left = [k for k in active if t < totals[k]]
        if resume and (due or len(left) != len(active)):
            if not due and group is not None:
                group.synchronize()
            commit(active)
        if len(left) != len(active):
            active = left
            if active and regroup is not None:
                group = regroup(list(active))
    flush()
