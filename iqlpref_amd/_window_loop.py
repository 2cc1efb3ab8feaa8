"""The train / log / evaluate / checkpoint / resume loop of the offline flavour, once: ``train()`` (K seeds of
one config, metrics exchanged across ranks) and ``sweep.train_runs`` (the runs of a launch batch, each with its
own length and periods, that leave when they end).  ``_offline_loop`` is its sibling for the custom-offline
flavours.  Nothing here touches the GPU or loads the library, and the loop knows no trainer class, buffer, env
or ``SeedGroup``: the caller hands in how a group is built, how a chunk is queued and how a member is evaluated.
"""
import os
import time
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _resume
from ._offline_loop import Members, PerMember, spread


def next_boundary(t: int, total: int, log_every: int, eval_every: int) -> int:
    """ref:1533-1544 as the loop chunks it: a member's next log boundary, evaluation boundary or end."""
    return min(total, (t // log_every + 1) * log_every, (t // eval_every + 1) * eval_every)


class State:
    """Where K members stand: the common step ``t``, every member's loss window since its last log boundary
    (None at one) and last window record, and the step of the resume file each holds (``kept``)."""

    def __init__(self, K: int):
        self.t, self.kept = 0, {}
        self.windows: List[Optional[torch.Tensor]] = [None] * K
        self.last: List[Dict[str, float]] = [{} for _ in range(K)]


def restore(trainers: Sequence, ckpt_dirs: Sequence[Optional[str]], at_most: Optional[int] = None) -> State:
    """The state of the newest complete resume generation under ``ckpt_dirs`` (``_resume.restore``; of a step <=
    ``at_most`` when given) with every trainer loaded from it, or the fresh state when there is none.  To be
    called before the trainers join a group."""
    state = State(len(trainers))
    state.t, payloads = _resume.restore(ckpt_dirs, state.kept, at_most=at_most)
    for k, p in payloads.items():
        trainers[k].load_resume_state(p["trainer"])
        state.windows[k] = p["loop"]["window"]
        state.last[k] = dict(p["loop"].get("last", {}))  # (sweep generations of before this module have none)
    return state


def run(state: State, trainers: Sequence, seeds: Sequence[int], total: PerMember, log_every: PerMember,
        eval_every: PerMember, logger: Callable, ckpt_dirs: Sequence[Optional[str]], make_group: Callable,
        steps: Callable, evaluate: Callable, tagged: Callable, *, goal_env: Union[bool, Sequence[bool]] = False,
        exchange: Optional[Callable] = None, resume: bool = False, keep_previous: bool = False) -> None:
    """Train members 0 .. K-1 from ``state`` to their ``total`` steps (``total`` / ``log_every`` / ``eval_every`` /
    ``goal_env``: one value for all, or one per member).  The members with steps to go are active; a finished one
    is neither trained nor evaluated again.  ``make_group(active)`` builds what steps them together (a
    ``SeedGroup``, or None); ``steps(group, active, t, n)`` queues steps t .. t + n - 1 and returns the loss
    tensors [n, 3] of the active members in their order.  A chunk ends at the next log boundary, evaluation
    boundary or end of ANY active member.  Then, in this order:

    * every member at a log boundary logs the means of its window (the one host read of a window) at
      ``trainer.total_it``: ``logger(tagged(record, k), step)``.  ``state.last`` keeps that plus ``steps_per_sec``;
    * with members at an evaluation boundary the group is synchronized; each of them then calls
      ``evaluate(k, trainer, t) -> (scores, steps_to_goal)`` or ``(None, [])``, logs ``mean_score`` (and, a
      ``goal_env``, ``avg_steps_to_goal``) if there are scores, and saves ``trainer.state_dict()`` as
      ``checkpoint_{t - 1}.pt`` if it has a directory; ``exchange`` then gets one record per evaluated member;
    * ``resume``: if a member evaluated or ended, every active member -- due or not -- writes its file of resume
      generation t (``_resume.commit`` with ``keep_previous``), after a synchronize if no evaluation made one.
      So every run ends with a generation at its last step that says ``finished``;
    * a member at its end leaves: the group is synchronized and closed, and ``make_group`` is called with the
      members that go on (for none, nothing is built).  An exception closes the group without a synchronize
      (``_offline_loop.Members``)."""
    K = len(trainers)
    totals, logs, evals, goal = spread(total, K), spread(log_every, K), spread(eval_every, K), spread(goal_env, K)
    if not len(totals) == len(logs) == len(evals) == len(goal) == K:
        raise ValueError("total / log_every / eval_every / goal_env: one entry per member")
    windows, last = state.windows, state.last
    t_window = [time.perf_counter()] * K
    with Members(make_group, [k for k in range(K) if state.t < totals[k]]) as live:
        while live.active:
            active, t0 = live.active, state.t
            t = state.t = min(next_boundary(t0, totals[k], logs[k], evals[k]) for k in active)
            for k, l in zip(active, steps(live.group, list(active), t0, t - t0)):
                windows[k] = l if t0 % logs[k] == 0 else torch.cat([windows[k].to(l.device), l])
            logged = [k for k in active if t % logs[k] == 0]
            means = [windows[k].mean(dim=0).tolist() for k in logged]  # the only host syncs of the window
            now = time.perf_counter()
            for k, mean in zip(logged, means):
                rec = {"value_loss": mean[0], "q_loss": mean[1], "actor_loss": mean[2]}
                logger(tagged(dict(rec), k), trainers[k].total_it)
                last[k] = dict(rec, steps_per_sec=windows[k].shape[0] / max(now - t_window[k], 1e-9))
                t_window[k] = now
            due = [k for k in active if t % evals[k] == 0]
            if due:
                live.synchronize()
            records = []
            for k in due:
                trainer, eval_log = trainers[k], {}
                scores, steps_to_goal = evaluate(k, trainer, t)
                if scores is not None:
                    eval_log["mean_score"] = float(np.mean(scores))
                    if goal[k]:
                        eval_log["avg_steps_to_goal"] = float(np.mean(steps_to_goal)) if steps_to_goal else -1.0
                    logger(tagged(dict(eval_log), k), trainer.total_it)
                if ckpt_dirs[k] is not None:
                    torch.save(trainer.state_dict(), os.path.join(ckpt_dirs[k], f"checkpoint_{t - 1}.pt"))
                records.append(dict(last[k] if t >= logs[k] else {}, seed=seeds[k], total_it=trainer.total_it,
                                    **eval_log))
            if due and exchange is not None:
                exchange(records)
            left = [k for k in active if t < totals[k]]
            if resume and live.commit_due(due, left):
                payloads = {k: {"finished": t >= totals[k], "trainer": trainers[k].resume_state(), "sampler": None,
                                "loop": {"window": None if t % logs[k] == 0 or windows[k] is None else windows[k].cpu(),
                                         "last": dict(last[k])}} for k in active}
                _resume.commit(ckpt_dirs, t, payloads, state.kept, keep_previous=keep_previous)
            live.keep(left)
