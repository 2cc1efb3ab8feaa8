"""The chunked train / evaluate / checkpoint loop of the custom-offline flavours (``custom_offline``,
``custom_offline_br``, ``custom_offline_bb``), once, and the setup every ``train()`` shares: the checkpoint
directories, the default logger and the ``seed`` tag of K > 1 records.

``run`` knows no trainer class, buffer or sampler: a flavour hands in how a chunk of steps is queued and how
one seed is evaluated.  Nothing here touches the GPU or loads the library.
"""
import os
import uuid
from dataclasses import asdict
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

Logger = Callable[[Dict[str, float], int], None]


def checkpoint_dirs(config, seeds: Sequence[int]) -> List[Optional[str]]:
    """The checkpoint directory of every seed (None each without ``config.checkpoints_path``): the path
    itself for one seed, ``seed_<seed>/`` under it for several.  Makes them and writes ``config.yaml``."""
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


def run(trainers: Sequence, seeds: Sequence[int], group, total: int, every: int, chunk: int, logger: Logger,
        ckpt_dirs: Sequence[Optional[str]], steps: Callable[[int, int], List[torch.Tensor]],
        evaluate: Callable[[int, object, int], np.ndarray], normalized: Optional[Callable] = None,
        best_by_return: bool = False) -> None:
    """``total`` steps in chunks of at most ``chunk`` that end on the evaluation boundaries (every ``every``
    steps); the losses of a chunk come back to the host once, after the next chunk has been queued.

    ``steps(t, n)`` queues steps t .. t + n - 1 and returns the K loss tensors [n, 3]; ``group`` (a
    ``SeedGroup`` or None) is synchronized before an evaluation.  ``evaluate(k, trainer, step)`` gives the
    returns of seed k.  ``normalized(returns)``: the normalized scores, logged x 100; a ``ValueError`` from
    it keeps what the seed had (at first the raw mean return), and a value once obtained stays.  The best
    model is the one of the strictly greatest normalized score, or mean return without one or with
    ``best_by_return``.  One ``logger(record, step)`` call per step and seed for the losses, then per
    evaluation record."""
    K = len(trainers)
    tagged = tag(seeds)
    best_score, best_step = [-np.inf] * K, [0] * K
    norm = [None] * K
    pending = None  # (first step, [K] device losses) of the chunk whose records are still to be logged

    def flush():
        nonlocal pending
        if pending is None:
            return
        t0, losses = pending
        pending = None
        for k, arr in enumerate(l.cpu().numpy() for l in losses):
            for i, (v, q, a) in enumerate(arr.tolist()):
                logger(tagged({"value_loss": v, "q_loss": q, "actor_loss": a}, k), t0 + i)

    t = 0
    while t < total:
        nxt = min(total, t + int(chunk), (t // every + 1) * every)
        losses = steps(t, nxt - t)
        flush()
        pending = (t, losses)
        t = nxt
        if t % every != 0:
            continue
        flush()
        if group is not None:
            group.synchronize()
        step = t - 1
        for k, trainer in enumerate(trainers):
            log = lambda d: logger(tagged(d, k), step)
            eval_scores = evaluate(k, trainer, step)
            mean_eval = eval_scores.mean()
            log({"evaluation_return": mean_eval})
            if normalized is not None:
                try:
                    norm[k] = np.asarray(normalized(eval_scores)).mean() * 100
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
    flush()
