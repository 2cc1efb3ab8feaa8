"""Resume generations: what the training loops write at an evaluation boundary so that a killed run can go on
from there bit for bit (``resume=True`` of ``train`` / ``sweep.train_runs`` / ``custom_offline.train`` /
``custom_offline.train_runs``).  Host only: nothing here touches the GPU or loads the library.

One generation = one file ``resume_{t}.pt`` per member (a seed of a group, a run of a launch batch) under the
member's own checkpoint directory, all at one common step ``t`` (the number of steps done); the file of a member
whose run is over at ``t`` is named ``resume_{t}.done.pt``, so that a run's progress is read off a directory
listing.  A file holds

    step      t
    finished  whether the member's run is over at t (it is then neither trained nor evaluated again)
    trainer   ``ImplicitQLearning.resume_state()``
    sampler   what the member's index sampler needs besides seed and step (None for the Philox stream)
    loop      the loop's own per-member state (best score and step, kept normalized score, loss window, ...)

Files are written under a temporary name and renamed with ``os.replace``; the files of the generation before
are removed only after every member's new file exists, and the file of a finished member stays.  So at any
moment the newest step at which EVERY unfinished member has a readable file is a complete generation.
"""
import os
import re
from dataclasses import asdict, is_dataclass
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import torch

_NAME = re.compile(r"^resume_(\d+)(\.done)?\.pt$")
TMP_SUFFIX = ".tmp"
# config fields that only say where files lie (a run directory may be moved, a reward model re-exported
# elsewhere); ``name`` is the run directory's own name.  Every other field must be equal to resume.
PATH_FIELDS = ("name", "checkpoints_path", "load_model", "config_path")
PATH_ENDINGS = ("_path", "_root")


def file_of(directory: str, step: int, finished: bool = False) -> str:
    """The name says what ``--list --resume`` asks of a run, so that nobody loads a state to learn it: the step,
    and ``.done`` when the member's run is over at that step."""
    return os.path.join(directory, f"resume_{int(step)}{'.done' if finished else ''}.pt")


def _entries(directory: Optional[str]) -> Dict[int, Tuple[str, bool]]:
    """step -> (path, finished) of the generation files in ``directory`` (temporary files do not count)."""
    if directory is None or not os.path.isdir(directory):
        return {}
    out = {}
    for name in sorted(os.listdir(directory)):
        m = _NAME.match(name)
        if m:
            out[int(m.group(1))] = (os.path.join(directory, name), m.group(2) is not None)
    return out


def steps_in(directory: Optional[str]) -> List[int]:
    """The steps of the generation files in ``directory``, ascending."""
    return sorted(_entries(directory))


def write(directory: str, step: int, payload: Mapping[str, Any]) -> str:
    """One member's file of generation ``step``: complete under its final name, or not there."""
    path = file_of(directory, step, bool(payload["finished"]))
    tmp = path + TMP_SUFFIX
    torch.save(dict(payload, step=int(step)), tmp)
    os.replace(tmp, path)
    return path


def read(directory: str, step: int) -> Optional[Dict[str, Any]]:
    """The file of ``step``; None when there is none or when it is cut short (what a crash of the file system
    can leave under the final name).  Every other failure -- an I/O error, a file this torch refuses, a file
    of another step -- is raised: a state that cannot be read is not a state that is not there."""
    entry = _entries(directory).get(int(step))
    if entry is None:
        return None
    path, finished = entry
    try:
        payload = torch.load(path, map_location="cpu", weights_only=True)
    except FileNotFoundError:
        return None
    except (EOFError, RuntimeError) as e:
        # torch's zip reader on a truncated archive ("failed finding central directory", "unexpected EOF", ...)
        if isinstance(e, EOFError) or "PytorchStreamReader" in str(e) or "central directory" in str(e):
            return None
        raise
    if not isinstance(payload, dict) or payload.get("step") != int(step) or "trainer" not in payload or \
            bool(payload.get("finished")) != finished:
        raise ValueError(f"{path} is not the resume file of step {step} its name says it is")
    return payload


def latest(dirs: Sequence[Optional[str]], members: Optional[Sequence[int]] = None, at_most: Optional[int] = None
           ) -> Optional[Tuple[int, Dict[int, Dict[str, Any]]]]:
    """The newest complete generation over ``members`` (indices into ``dirs``; default all): the greatest
    step t (<= ``at_most`` when given) at which every member has a readable file of step t, or a readable
    file of an earlier step that says the member finished there.  -> (t, {member: payload}), or None when
    there is none."""
    members = list(range(len(dirs))) if members is None else list(members)
    if not members:
        return None
    have = {k: steps_in(dirs[k]) for k in members}
    cache: Dict[Tuple[int, int], Optional[Dict[str, Any]]] = {}

    def get(k, s):
        if (k, s) not in cache:
            cache[(k, s)] = read(dirs[k], s)
        return cache[(k, s)]

    for t in sorted({s for k in members for s in have[k] if at_most is None or s <= at_most}, reverse=True):
        found = {}
        for k in members:
            p = get(k, t) if t in have[k] else None
            if p is None:
                for s in sorted((s for s in have[k] if s < t), reverse=True):
                    q = get(k, s)
                    if q is not None:
                        p = q if q.get("finished") else None
                        break
            if p is None:
                break
            found[k] = p
        if len(found) == len(members):
            return t, found
    return None


def clean(dirs: Sequence[Optional[str]], keep: Mapping[int, int]) -> None:
    """Remove every generation file and temporary file of member k other than the file of step ``keep[k]``
    (members not in ``keep`` lose all of theirs)."""
    for k, d in enumerate(dirs):
        if d is None or not os.path.isdir(d):
            continue
        for name in os.listdir(d):
            m = _NAME.match(name)
            stale_tmp = name.startswith("resume_") and name.endswith(".pt" + TMP_SUFFIX)
            if stale_tmp or (m and int(m.group(1)) != keep.get(k, -1)):
                try:
                    os.remove(os.path.join(d, name))
                except FileNotFoundError:
                    pass


def restore(dirs: Sequence[Optional[str]], kept: Dict[int, int], members: Optional[Sequence[int]] = None,
            at_most: Optional[int] = None) -> Tuple[int, Dict[int, Dict[str, Any]]]:
    """How every loop starts under ``resume``: -> (t, {member: payload}) of the newest complete generation
    (``latest``), with ``kept`` filled and whatever a later, half-written generation left behind removed; (0, {})
    when there is no generation -- the members hold no file, or files of ONE step that some of them lack (the
    first generation, cut between two files).  Members that hold files of different steps and no step in common
    were not written by this batch of members (another ``--only`` / ``runs_per_gpu``, directories of two earlier
    starts): ValueError, and nothing is removed -- those files are hours of evaluations."""
    if any(d is None for d in dirs):
        raise ValueError("resume=True needs a checkpoint directory for every member (config.checkpoints_path)")
    members = list(range(len(dirs))) if members is None else list(members)
    found = latest(dirs, members, at_most)
    if found is None and at_most is None:
        held = {k: steps_in(dirs[k]) for k in members if steps_in(dirs[k])}
        if len({s for steps in held.values() for s in steps}) > 1:
            raise ValueError(
                "resume=True: these runs hold resume files but no generation in common ("
                + "; ".join(f"{dirs[k]}: steps {held[k]}" for k in held) + "): they were not interrupted as "
                "members of this batch.  Resume them in the batch they ran in (the same runs and runs_per_gpu), or "
                "remove their resume_*.pt files to start them at step 0")
    t, payloads = (0, {}) if found is None else found
    kept.update({k: int(p["step"]) for k, p in payloads.items()})
    clean([d if k in members else None for k, d in enumerate(dirs)], kept)
    return t, payloads


def commit(dirs: Sequence[Optional[str]], step: int, payloads: Mapping[int, Mapping[str, Any]],
           kept: Dict[int, int], keep_previous: bool = False) -> None:
    """Write generation ``step`` for the members of ``payloads``, then remove the generation before.
    ``kept``: member -> the step of the file it holds now (updated here; the files of members that are not
    in ``payloads`` -- the finished ones -- stay).  ``keep_previous``: the generation before stays too and
    the one before that goes (ranks that exchange metrics at every boundary are at most one generation
    apart: the older of two is one that all of them have)."""
    for k, p in payloads.items():
        write(dirs[k], step, p)
    for k in payloads:  # only now: every member's new file exists
        old = kept.get(k)
        for s, (path, _) in _entries(dirs[k]).items():
            if s != step and old is not None and (s < old if keep_previous else s == old):
                try:
                    os.remove(path)
                except FileNotFoundError:
                    pass
        kept[k] = int(step)


def status(directory: Optional[str]) -> str:
    """``done`` / ``at step t`` / ``new``: what the name of a run's newest generation file says (no file is
    opened)."""
    entries = _entries(directory)
    if not entries:
        return "new"
    s = max(entries)
    return "done" if entries[s][1] else f"at step {s}"


# --------------------------------------------------------------------------- #
# configs
# --------------------------------------------------------------------------- #
def is_path_field(name: str) -> bool:
    return name in PATH_FIELDS or name.endswith(PATH_ENDINGS)


def config_dict(config) -> Dict[str, Any]:
    return dict(asdict(config)) if is_dataclass(config) else dict(config)


def config_differences(saved: Mapping[str, Any], current: Mapping[str, Any]) -> List[str]:
    """The fields in which two configs differ, paths aside."""
    return sorted(k for k in set(saved) | set(current)
                  if not is_path_field(k) and (k not in saved or k not in current or saved[k] != current[k]))


def saved_config(checkpoints_path: str) -> Optional[Dict[str, Any]]:
    """The ``config.yaml`` that ``checkpoint_dirs`` wrote there (None: there is none)."""
    path = os.path.join(checkpoints_path, "config.yaml")
    if not os.path.isfile(path):
        return None
    import yaml
    with open(path) as f:
        out = yaml.safe_load(f)
    return out if isinstance(out, dict) else None


def check_config(config) -> None:
    """What ``resume=True`` asks of a config before anything is written: a ``checkpoints_path``, and -- when a
    run was started there -- the config it was started with, paths aside.  ValueError otherwise."""
    if getattr(config, "checkpoints_path", None) is None:
        raise ValueError("resume=True needs config.checkpoints_path: the generations are kept in the run's "
                         "checkpoint directory")
    saved = saved_config(config.checkpoints_path)
    if saved is None:
        return
    diff = config_differences(saved, config_dict(config))
    if diff:
        raise ValueError(f"resume=True: the run in {config.checkpoints_path} was started with another config "
                         f"(differs in {', '.join(diff)}); a resumed run is the uninterrupted run only under "
                         "the same config")


def adopt_run_dir(config, seeds: Optional[Sequence[int]] = None, taken: Optional[set] = None) -> bool:
    """For the command lines, whose configs get a fresh random ``name`` (and with it a fresh directory) at
    every start: look beside ``config.checkpoints_path`` for the directory of an earlier start of the same
    config that holds a generation, and take its ``name`` and ``checkpoints_path``.  The same config: its
    ``config.yaml`` equals this config in EVERY field but those two -- the runs of one sweep may differ in a
    path alone (the pen sweeps: ``reward_model_path``), so no path is left aside here.  ``seeds``: only a
    directory whose newest generation is of one of these seeds (the ranks of one job share the config and
    differ in their seeds).  ``taken``: the directories given to other runs of this invocation; none is given
    twice, and the one taken here is added.  Of several the one that got furthest; True when one was taken."""
    cp = getattr(config, "checkpoints_path", None)
    if cp is None:
        return False
    base = os.path.dirname(os.path.normpath(cp))
    if not os.path.isdir(base):
        return False
    mine = {k: v for k, v in config_dict(config).items() if k not in ("name", "checkpoints_path")}
    best = None
    for entry in sorted(os.listdir(base)):
        d = os.path.join(base, entry)
        saved = saved_config(d) if os.path.isdir(d) else None
        if saved is None or (taken is not None and os.path.realpath(d) in taken) or \
                {k: v for k, v in saved.items() if k not in ("name", "checkpoints_path")} != mine:
            continue
        # the run's own files, or (K seeds) those of seed_<s>/ below
        where = [d] + [os.path.join(d, e) for e in sorted(os.listdir(d)) if os.path.isdir(os.path.join(d, e))]
        files = [(s, w) for w in where for s in steps_in(w)]
        if not files:
            continue
        reach, newest = max(files)
        if seeds is not None and (read(newest, reach) or {}).get("trainer", {}).get("seed") not in {int(x) for x in seeds}:
            continue
        if best is None or reach > best[0]:
            best = (reach, d, saved)
    if best is None:
        return False
    config.checkpoints_path = best[1]
    if "name" in best[2] and hasattr(config, "name"):
        config.name = best[2]["name"]
    if taken is not None:
        taken.add(os.path.realpath(best[1]))
    return True


def run_status(config) -> str:
    """``status`` of a config's run (``new`` without a ``checkpoints_path``)."""
    cp = getattr(config, "checkpoints_path", None)
    return "new" if cp is None else status(cp)
