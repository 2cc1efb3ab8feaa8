"""Sweep grids on one GPU: the runs of a W&B grid file, packed into seed groups.

The reference runs its pipeline (PIPELINE.md, Phase 2) as W&B grid sweeps: a file
``*_sweeps/sweep_*.yaml`` with ``method: grid`` and ``parameters: {name: {value | values}}`` plus a
``config_path`` naming the base YAML, and ``launch.sh`` starts ``AGENTS_PER_GPU`` agents per GPU, one
run each.  Here one process takes the whole grid:

``expand_sweep(file)``
    one ``TrainConfig`` per run of the grid.
``train_runs(configs)``
    every config trained as ``train(config)`` trains it, bit for bit, with runs of one shape stepped
    together as one ``SeedGroup`` (iqlpref_amd.multi): the group kernels read every hyperparameter
    (discount, tau, beta, iql_tau, dropout rate, learning rates, schedule length) from each member's
    own descriptor, so runs that differ in any of them -- not only in the seed -- share one launch
    sequence.
``python -m iqlpref_amd.sweep SWEEP.yaml [--list] [--only i,j] [--runs_per_gpu K] [--resume] [--field value]``
    the command line over both.  ``--resume``: every run goes on from its last evaluation boundary, bit for
    bit (``train_runs(resume=True)``); with ``--list`` it prints ``done`` / ``at step t`` / ``new`` per run.

Two flavours of sweep file.  A file whose ``program`` ends in ``custom_offline/iql.py`` (the six pen sweeps,
``mr_sweeps/sweep_pen_*_pref.yaml`` and ``pt_sweeps/sweep_pen_*_pt.yaml``) is a custom-flavour sweep: its
names are those of ``custom_offline.TrainConfig``, ``expand_sweep`` builds configs of that class through
``custom_offline.load_config``, and the command line trains them with ``custom_offline.train_runs`` (runs
that differ in the reward model, not the seed, as one seed group).  Every other ``program`` value, and none,
is an offline sweep as before.

The W&B service itself (agents, the sweep server, random / bayes search) stays out.
"""
import argparse
import importlib
import itertools
import os
import sys
from dataclasses import asdict, fields
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, _resume, _window_loop, custom_offline
from . import distributed as D
from ._offline_loop import checkpoint_dirs
from .iql import ImplicitQLearning, TrainConfig, load_config
from .multi import GROUP_MODES, SeedGroup, check_group_mode, resolve_group_mode

# top-level keys of a sweep file that only name or describe it (kept as labels, otherwise ignored)
LABEL_KEYS = ("program", "project", "name", "description", "metric", "command", "entity")
# the fields build_dataset reads besides the environment: runs equal in all of them share one relabel
RELABEL_FIELDS = ("reward_model_path", "query_length", "bnn_reward_model", "bnn_alpha", "bnn_n_samples",
                  "mr_ensemble", "mr_alpha", "mr_burn_in")
# a sweep file whose ``program`` ends in this runs the Minari custom-offline flavour (custom_offline.py)
CUSTOM_PROGRAM = "custom_offline/iql.py"
# observation / action sizes of the D4RL task families the reference's sweeps name (for --list
# without gym; training always reads them from the environment itself)
D4RL_DIMS = {"antmaze": (29, 8), "pen": (45, 24), "door": (39, 28), "hammer": (46, 26), "relocate": (39, 30),
             "halfcheetah": (17, 6), "hopper": (11, 3), "walker2d": (17, 6), "kitchen": (60, 9)}


# --------------------------------------------------------------------------- #
# sweep files -> configs
# --------------------------------------------------------------------------- #
def load_sweep(spec_or_path: Union[str, os.PathLike, Mapping]) -> Dict[str, Any]:
    """A sweep file's contents (a path is read as YAML; a mapping is taken as it is)."""
    if isinstance(spec_or_path, Mapping):
        return dict(spec_or_path)
    import yaml
    with open(spec_or_path) as f:
        spec = yaml.safe_load(f)
    if not isinstance(spec, dict):
        raise ValueError(f"{spec_or_path}: a sweep file is a mapping")
    return spec


def is_custom_sweep(spec: Mapping) -> bool:
    """Whether the sweep file runs ``algorithms/custom_offline/iql.py`` (told from its ``program`` key)."""
    return str(spec.get("program") or "").endswith(CUSTOM_PROGRAM)


def _flavour(spec: Mapping):
    """(TrainConfig class, load_config) of the flavour the sweep file runs."""
    if is_custom_sweep(spec):
        return custom_offline.TrainConfig, custom_offline.load_config
    return TrainConfig, load_config


def sweep_axes(spec: Mapping, known=None,
               what: str = "TrainConfig fields nor config_path") -> List[Tuple[str, List[Any]]]:
    """The grid's parameters in file order: [(name, [values...])].  Only ``method: grid`` with
    ``{value: x}`` / ``{values: [...]}`` entries; every name must be a field of the flavour's TrainConfig
    (``is_custom_sweep``) or ``config_path`` (all unknown names are reported together).  ``known``: another
    set of accepted names (``posthoc.expand_eval_sweep``: the fields of its EvalConfig), ``what`` names it."""
    method = spec.get("method")
    if method != "grid":
        raise ValueError(f"sweep method {method!r}: only 'grid' is supported (random / bayes search needs the "
                         "W&B sweep service)")
    extra = sorted(set(spec) - set(LABEL_KEYS) - {"method", "parameters"})
    if extra:
        raise ValueError(f"unsupported top-level sweep keys: {', '.join(extra)}")
    params = spec.get("parameters") or {}
    if not isinstance(params, Mapping):
        raise ValueError("'parameters' must map names to {value: x} or {values: [...]}")
    if known is None:
        known = {f.name for f in fields(_flavour(spec)[0])} | {"config_path"}
    axes, unknown = [], []
    for name, entry in params.items():
        if not isinstance(entry, Mapping) or len(entry) != 1 or next(iter(entry)) not in ("value", "values"):
            got = sorted(entry) if isinstance(entry, Mapping) else type(entry).__name__
            raise ValueError(f"parameter {name!r}: a grid entry is exactly {{value: x}} or {{values: [...]}}, "
                             f"got {got}")
        if "value" in entry:
            vals = [entry["value"]]
        else:
            vals = entry["values"]
            if not isinstance(vals, (list, tuple)) or not vals:
                raise ValueError(f"parameter {name!r}: 'values' must be a non-empty list")
            vals = list(vals)
        if name not in known:
            unknown.append(name)
        axes.append((name, vals))
    if unknown:
        raise ValueError(f"unknown sweep parameters (neither {what}): {', '.join(unknown)}")
    return axes


def expand_sweep(spec_or_path, *, config_root: str = ".", **overrides) -> List[TrainConfig]:
    """One TrainConfig per run of a W&B grid sweep (``custom_offline.TrainConfig`` for a custom-flavour
    file, ``is_custom_sweep``).

    Order: the cartesian product of the parameters in the order the file lists them, the LAST
    parameter varying fastest (``a: [1, 2]``, ``b: [x, y]`` -> (1, x), (1, y), (2, x), (2, y)).

    Each run loads its ``config_path`` (resolved against ``config_root``) with ``load_config``; the
    sweep's values override the base YAML and ``overrides`` (the command line's ``--field value``)
    override both, all coerced to the field types as load_config does.  With ``reward_model_root``
    every run reads ``{root}_{seed}`` (TrainConfig.__post_init__, as iql_eval.py does).  Every config
    carries ``sweep_label``: the varying parameters of its run, e.g. ``normalize_reward=3,seed=0``."""
    spec = load_sweep(spec_or_path)
    axes = sweep_axes(spec)
    config_cls, load = _flavour(spec)
    known = {f.name for f in fields(config_cls)} | {"config_path"}
    bad = [k for k in overrides if k not in known]
    if bad:
        raise ValueError(f"unknown overrides (not TrainConfig fields): {', '.join(bad)}")
    names = [n for n, _ in axes]
    varying = [n for n, vals in axes if len(vals) > 1 and n not in overrides]
    out = []
    for combo in itertools.product(*[vals for _, vals in axes]):
        run = dict(zip(names, combo))
        label = ",".join(f"{n}={run[n]}" for n in varying)
        run.update(overrides)
        cp = run.pop("config_path", None)
        path = None if cp is None else os.path.join(config_root, os.path.expanduser(str(cp)))
        cfg = load(path, **run)
        cfg.sweep_label = label  # (an attribute, not a field: config.yaml stays what train() writes)
        out.append(cfg)
    return out


# --------------------------------------------------------------------------- #
# host-side planning (no device work)
# --------------------------------------------------------------------------- #
def shape_key(config: TrainConfig, dims, precision: str = "bf16") -> tuple:
    """What runs of one SeedGroup must share (iqlhip_group_create's same_shape): state / action dims,
    batch size, policy kind, actor dropout on/off, critics, precision, device, width and number of the
    hidden layers.  ``dims`` = (S, A), or
    None when unknown (the env name stands in: runs of one env always share their dims)."""
    dims_key = tuple(int(d) for d in dims) if dims is not None else ("env", config.env)
    return (dims_key, int(config.batch_size), bool(config.iql_deterministic), bool(config.actor_dropout),
            int(config.n_critics), precision, str(config.device), int(config.hidden_dim), int(config.n_hidden))


def _check_runs_per_gpu(runs_per_gpu: int) -> int:
    k = int(runs_per_gpu)
    if not 1 <= k <= _lib.MAX_GROUP:
        raise ValueError(f"runs_per_gpu = {runs_per_gpu}: must be 1..{_lib.MAX_GROUP}")
    return k


def plan_batches(configs: Sequence, dims, runs_per_gpu: int = 8, precision: str = "bf16", *,
                 key: Optional[Callable[[Any, Any], tuple]] = None) -> List[List[int]]:
    """Launch batches as lists of config indices, in the order they run.  Runs of equal
    ``shape_key`` are taken greedily in config order into batches of at most ``runs_per_gpu``; a
    batch's position is that of its first run.  ``dims``: one (S, A) per config, or a mapping
    env name -> (S, A) (entries may be None, see ``shape_key``).  ``key(config, dims)``: the shape key
    of another flavour's configs (default: ``shape_key`` at ``precision``)."""
    k = _check_runs_per_gpu(runs_per_gpu)
    if key is None:
        key = lambda cfg, d: shape_key(cfg, d, precision)
    open_batch: Dict[tuple, List[int]] = {}
    batches: List[List[int]] = []
    for i, cfg in enumerate(configs):
        d = dims.get(cfg.env) if isinstance(dims, Mapping) else dims[i]
        shape = key(cfg, d)
        b = open_batch.get(shape)
        if b is None or len(b) >= k:
            b = open_batch[shape] = []
            batches.append(b)
        b.append(i)
    return batches


def rank_share(n_configs: int, rank: int, world_size: int) -> List[int]:
    """The configs rank ``rank`` of ``world_size`` trains: index = rank (mod world size)."""
    return list(range(int(rank), int(n_configs), max(int(world_size), 1)))


def check_runs(configs: Sequence, runs_per_gpu: int) -> None:
    """The checks train_runs makes before any device work."""
    _check_runs_per_gpu(runs_per_gpu)
    seen: Dict[str, int] = {}
    for i, cfg in enumerate(configs):
        if cfg.checkpoints_path is None:
            continue
        p = os.path.abspath(os.path.expanduser(cfg.checkpoints_path))
        if p in seen:
            raise ValueError(f"runs {seen[p]} and {i} share checkpoints_path {cfg.checkpoints_path!r}")
        seen[p] = i


def _rank_world() -> Tuple[int, int]:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def start_runs(configs: Sequence, runs_per_gpu: int, run_ids: Optional[Sequence[int]],
               resume: bool) -> Tuple[List[int], List[int]]:
    """What both ``train_runs`` do first, ahead of any device work: ``check_runs``, under ``resume`` every config's
    ``_resume.check_config``, the runs' names (default 0 .. n-1).  -> (run_ids, this rank's config indices)."""
    check_runs(configs, runs_per_gpu)
    if resume:
        for cfg in configs:
            _resume.check_config(cfg)
    n = len(configs)
    run_ids = list(range(n)) if run_ids is None else [int(r) for r in run_ids]
    if len(run_ids) != n:
        raise ValueError("run_ids: one entry per config")
    return run_ids, rank_share(n, *_rank_world())


class BatchCache:
    """key -> value, built on first need and dropped after the last launch batch whose runs use the key.
    ``batches``: lists of run indices in the order they run; ``key(i)``: the key of run i (kept as ``key_of[i]``)."""

    def __init__(self, batches: Sequence[Sequence[int]], key: Callable[[int], Any]):
        self.key_of, self._values = {i: key(i) for b in batches for i in b}, {}
        self._last_use = {self.key_of[i]: bi for bi, b in enumerate(batches) for i in b}

    def __contains__(self, key) -> bool:
        return key in self._values

    def get(self, i: int, build: Callable[[], Any]):
        """The value of run i's key; ``build()`` makes it if no earlier run has."""
        if self.key_of[i] not in self._values:
            self._values[self.key_of[i]] = build()
        return self._values[self.key_of[i]]

    def batch_done(self, bi: int) -> None:
        for key in [k for k in self._values if self._last_use[k] <= bi]:
            del self._values[key]


def _relabel_key(config: TrainConfig) -> tuple:
    return (config.env, str(config.device)) + tuple(getattr(config, f) for f in RELABEL_FIELDS)


# --------------------------------------------------------------------------- #
# training
# --------------------------------------------------------------------------- #
def _default_logger(configs: Sequence, mine: Sequence[int], run_ids: Sequence[int]):
    """One wandb run per process, the records of run i under ``run<i>/`` (with its own step axis:
    every launch batch starts again at step 0); without wandb the records are printed.  (The records of the
    custom flavour carry ``run`` and no ``seed``.)"""
    try:
        import wandb
    except ImportError:
        def show(d, step):
            who = f"run {d['run']}" + (f" seed {d['seed']}" if "seed" in d else "")
            print(f"[{who}] [{step}] " + " ".join(f"{n}={v:.5g}" for n, v in d.items() if n not in ("run", "seed")))
        return show
    first = configs[mine[0]]
    wandb.init(config={f"run{run_ids[i]}": asdict(configs[i]) for i in mine}, project=first.project,
               group=first.group, name=first.name)
    for i in mine:
        wandb.define_metric(f"run{run_ids[i]}/*", step_metric=f"run{run_ids[i]}/step")

    def log(d, step):
        r = d["run"]
        wandb.log({f"run{r}/step": step, **{f"run{r}/{n}": v for n, v in d.items() if n not in ("run", "seed")}})
    return log


def _resolve_envs(configs: Sequence[TrainConfig], mine: Sequence[int], env) -> Dict[str, Any]:
    """env name -> environment object for this rank's runs."""
    names = list(dict.fromkeys(configs[i].env for i in mine))
    if env is None:
        import gym
        return {n: gym.make(n) for n in names}
    if isinstance(env, Mapping):
        missing = [n for n in names if n not in env]
        if missing:
            raise ValueError(f"no environment given for {', '.join(missing)}")
        return {n: env[n] for n in names}
    if len(names) > 1:
        raise ValueError(f"one env object given for runs of {len(names)} environments ({', '.join(names)}); "
                         "pass env=None or a mapping env name -> env")
    return {n: env for n in names}


def train_runs(configs: Sequence[TrainConfig], env=None, dataset=None, *, runs_per_gpu: int = 8,
               logger: Optional[Callable[[Dict[str, float], int], None]] = None,
               evaluate: Union[None, Callable, Sequence[Callable]] = None, precision: str = "bf16",
               raw_dataset=None, host_prep: bool = False, vector_env: Optional[Callable] = None,
               group_mode: Optional[str] = None,
               run_ids: Optional[Sequence[int]] = None, resume: bool = False) -> List[ImplicitQLearning]:
    """Train every config exactly as ``train(config)`` would -- the same logged records (plus ``run``
    / ``seed`` entries), evaluation calls (own actor, own seed), checkpoint files (``config.yaml`` and
    ``checkpoint_{t}.pt`` under the run's own ``checkpoints_path``) and final parameters, target,
    Adam moments and ``total_it``, bit for bit -- with the runs packed into seed groups.

    Launch batches (``plan_batches``): runs of one shape key (dims, batch size, policy kind, dropout
    on/off, critics, precision, device, hidden_dim, n_hidden), at most ``runs_per_gpu`` (1..16) in config order; the
    batches run one after another, each as one ``SeedGroup`` of mode ``group_mode`` (None: the
    SeedGroup default; "general": one launch sequence for batches whose shape runs on the general
    layer-wise step, the default for the others).  Inside a batch everything else may differ: seed, reward normalisation,
    discount, tau, beta, iql_tau, learning rates, dropout rate, max_timesteps, log / eval
    frequencies, reward model, and the env when its dims match.  All runs of a batch start at step
    0; every library call runs to the next log / eval / end boundary of ANY active run; a finished
    run leaves the batch and the group is rebuilt over the others.

    ``env``: one environment for runs of one env name, a mapping env name -> environment, or None
    (one ``gym.make`` per name).  ``dataset`` / ``raw_dataset`` as in ``train()``, or a callable
    ``config -> dict`` (called once per distinct relabel key).  The dataset is relabelled once per
    distinct (env, reward-model fields) and one device buffer is built per distinct (relabel,
    normalize_reward, normalize); runs equal in those share it.  ``evaluate``: one callable
    ``(actor, step)`` or a list with one per config.  ``logger(record, step)``: default one wandb run
    per process with keys ``run<i>/``, or print.  ``run_ids``: the names of the runs in the records
    (default 0 .. n-1).

    ``resume`` (every config needs a ``checkpoints_path``, and the ``config.yaml`` there, if any, must have
    been written for the same config, paths aside; ValueError otherwise, before any device work): as in
    ``train()``, per launch batch.  At the end of every boundary at which a run of the batch evaluated or
    ended, every run active in it -- due or not -- writes ``resume_{t}.pt`` (trainer ``resume_state()``, its
    partly filled loss window, whether it has ended) at the batch's common step t under its own
    ``checkpoints_path``; the files of the generation before go once all are written, the file of an ended
    run stays.  A batch starts from its newest complete generation: ended runs are neither trained nor
    evaluated again (their trainers are loaded from their final state), the others go on as one regrouped
    batch, bit for bit the uninterrupted run.  A batch without a generation starts at step 0.  The step is
    one that all unfinished runs of the batch have: resume with the configs and ``runs_per_gpu`` of the first
    start -- runs that hold generations with no step in common are refused (ValueError) and keep their files.

    Under torchrun rank r trains the configs with index = r (mod world size), each at its own seed,
    with no collectives (each rank resumes its own runs).  Returns this rank's trainers in config order."""
    # the module, not the function the package exports under the same name (build_dataset is looked
    # up on it at call time: tests count its calls)
    T = importlib.import_module(".train", __package__)

    configs = list(configs)
    run_ids, mine = start_runs(configs, runs_per_gpu, run_ids, resume)
    if isinstance(evaluate, (list, tuple)) and len(evaluate) != len(configs):
        raise ValueError(f"evaluate: {len(evaluate)} callables for {len(configs)} configs")
    check_group_mode(group_mode)
    if not mine:
        return []
    envs = _resolve_envs(configs, mine, env)
    bound = D.local_device()  # under torchrun: this rank's GPU
    if bound is not None:
        for i in mine:
            configs[i].device = bound
    dims = {name: (e.observation_space.shape[0], e.action_space.shape[0]) for name, e in envs.items()}
    local = plan_batches([configs[i] for i in mine], [dims[configs[i].env] for i in mine], runs_per_gpu, precision)
    batches = [[mine[j] for j in b] for b in local]
    if logger is None:
        logger = _default_logger(configs, mine, run_ids)
    pick = lambda src, cfg: src(cfg) if callable(src) else src
    source = dataset if dataset is not None else raw_dataset

    # datasets and device buffers, built when a batch first needs them and dropped after their last batch
    rcfgs = {i: T.seed_configs(configs[i], [configs[i].seed])[0] for i in mine}
    datasets = BatchCache(batches, lambda i: _relabel_key(rcfgs[i]))
    buffers = BatchCache(batches, lambda i: (datasets.key_of[i], configs[i].normalize_reward,
                                             bool(configs[i].normalize), configs[i].buffer_size))

    def relabel(i):
        rc, src = rcfgs[i], pick(source, configs[i])
        return T.build_dataset(rc, envs[rc.env], src) if (rc.reward_model_path or dataset is None) else src

    def prepare(i):
        ds = datasets.get(i, lambda: relabel(i))
        if host_prep:  # the numpy path rewrites its dataset in place: every preparation gets a copy
            ds = {k: np.array(v) for k, v in ds.items()}
        return T._prepare_replay(configs[i], ds, *dims[configs[i].env], host_prep)

    trainers: Dict[int, ImplicitQLearning] = {}
    for bi, batch in enumerate(batches):
        bufs, evals = {}, {}
        for i in batch:
            cfg = configs[i]
            bufs[i], mean, std = buffers.get(i, lambda: prepare(i))
            e = envs[cfg.env]
            max_action = float(e.action_space.high[0])
            checkpoint_dirs(cfg, [cfg.seed], resume=resume)  # (one seed: the path itself, with its config.yaml)
            trainers[i] = T._build_trainer(cfg, cfg.seed, dims[cfg.env][0], dims[cfg.env][1], max_action, precision)
            evals[i] = (cfg, e, max_action, mean, std, cfg.seed)
        # one launch batch: its runs go in lock step to the next boundary of any of them, and at its end a run
        # leaves and the group is rebuilt over the rest.  The loop's member j is run members[j]
        members = [i for i in batch if int(configs[i].max_timesteps) > 0]
        cfgs, trs = [configs[i] for i in members], [trainers[i] for i in members]
        dirs = [c.checkpoints_path for c in cfgs]

        def make_group(active):
            group_trs = [trs[j] for j in active]
            return SeedGroup(group_trs, mode=resolve_group_mode(group_mode, group_trs, cfgs[active[0]].batch_size))

        def steps(group, active, t, n):
            return group.train_steps([bufs[members[j]] for j in active], n, cfgs[active[0]].batch_size,
                                     return_losses=True)

        _window_loop.run(
            _window_loop.restore(trs, dirs) if resume else _window_loop.State(len(members)), trs,
            [c.seed for c in cfgs], [c.max_timesteps for c in cfgs], [c.log_freq for c in cfgs],
            [c.eval_freq for c in cfgs], logger, dirs, make_group, steps,
            T.member_evaluator([evaluate[i] for i in members] if isinstance(evaluate, (list, tuple)) else evaluate,
                               vector_env, [evals[i] for i in members]),
            lambda rec, j: dict(rec, run=run_ids[members[j]], seed=cfgs[j].seed),
            goal_env=["antmaze" in c.env.lower() for c in cfgs], resume=resume)
        datasets.batch_done(bi)
        buffers.batch_done(bi)
    return [trainers[i] for i in mine]


# --------------------------------------------------------------------------- #
# command line
# --------------------------------------------------------------------------- #
def planned_mode(config: TrainConfig, group_mode: Optional[str]) -> str:
    """What ``--list`` prints for a run's batch: the SeedGroup mode ``group_mode`` resolves to for this
    shape, told from the config alone (no device; the library's own rule, without IQLHIP_FORCE_GENERAL)."""
    tuned = int(config.n_hidden) == 2 and int(config.hidden_dim) in (64, 128, 256)
    if group_mode is None or (group_mode == "general" and tuned):
        return "default"
    return group_mode


def _list_dims(env_name: str):
    fam = env_name.split("-")[0].lower()
    if fam in D4RL_DIMS:
        return D4RL_DIMS[fam]
    return None  # unknown family: batched by env name


def _list_dims_custom(dataset_id: str):
    """Dims of a Minari dataset id from the D4RL family inside it (``D4RL/pen/human-v2`` -> pen)."""
    for part in str(dataset_id).lower().replace("-", "/").split("/"):
        if part in D4RL_DIMS:
            return D4RL_DIMS[part]
    return None  # unknown family: batched by dataset id


def main(argv=None):
    """python -m iqlpref_amd.sweep SWEEP.yaml [--config_root DIR] [--runs_per_gpu K] [--only 0,3,5]
    [--list] [--resume] [--field value ...]"""
    from .train import parse_overrides
    ap = argparse.ArgumentParser(prog="python -m iqlpref_amd.sweep", allow_abbrev=False,
                                 description="train the runs of a W&B grid sweep file, packed into seed groups")
    ap.add_argument("sweep", help="sweep file (method: grid)")
    ap.add_argument("--config_root", default=".", help="directory the sweep's config_path is relative to")
    ap.add_argument("--runs_per_gpu", type=int, default=int(os.environ.get("AGENTS_PER_GPU", "8")),
                    help="runs stepped together as one seed group (default: $AGENTS_PER_GPU, else 8)")
    ap.add_argument("--only", default=None, help="comma-separated run indices to train")
    ap.add_argument("--list", action="store_true", help="print every run's index, label and launch batch; no GPU")
    ap.add_argument("--resume", action="store_true",
                    help="go on from the last evaluation boundary of an earlier start of each run under its "
                         "checkpoints_path (found by its config.yaml), bit for bit, and write resume generations; "
                         "with --list: print done / at step t / new per run")
    ap.add_argument("--group_mode", default=None, choices=list(GROUP_MODES),
                    help="SeedGroup mode of every launch batch (default: the SeedGroup default; 'general': one launch "
                         "sequence for batches on the general layer-wise step)")
    args, rest = ap.parse_known_args(argv)
    custom = is_custom_sweep(load_sweep(args.sweep))
    if custom and args.group_mode is not None:
        raise SystemExit(f"--group_mode: {args.sweep} is a custom-flavour sweep (program: ...{CUSTOM_PROGRAM}), whose "
                         "launch batches always run the SeedGroup default (fp32, 2 x 256 nets: there is no general "
                         "step to choose); drop the option")
    configs = expand_sweep(args.sweep, config_root=args.config_root, **parse_overrides(rest))
    ids = list(range(len(configs)))
    if args.only:
        ids = [int(s) for s in args.only.split(",") if s.strip()]
        bad = [i for i in ids if not 0 <= i < len(configs)]
        if bad:
            raise SystemExit(f"--only: no run {bad} (the sweep has {len(configs)})")
    chosen = [configs[i] for i in ids]
    if args.resume:  # (expanding the file gave every run a fresh random name and directory)
        taken = set()
        for cfg in chosen:
            _resume.adopt_run_dir(cfg, taken=taken)
    progress = (lambda i: "\t" + _resume.run_status(configs[i])) if args.resume else (lambda i: "")
    if custom:
        if args.list:
            batches = custom_offline.plan_batches(chosen, [_list_dims_custom(c.dataset_id) for c in chosen],
                                                  args.runs_per_gpu)
            where = {j: b for b, members in enumerate(batches) for j in members}
            for j, i in enumerate(ids):
                print(f"{i}\t{configs[i].sweep_label or '-'}\tbatch {where[j]}{progress(i)}")
            return
        custom_offline.train_runs(chosen, runs_per_gpu=args.runs_per_gpu, run_ids=ids, resume=args.resume)
        return
    if args.list:
        batches = plan_batches(chosen, [_list_dims(c.env) for c in chosen], args.runs_per_gpu)
        where = {j: b for b, members in enumerate(batches) for j in members}
        for j, i in enumerate(ids):
            mode = "" if args.group_mode is None else f"\tmode {planned_mode(configs[i], args.group_mode)}"
            print(f"{i}\t{configs[i].sweep_label or '-'}\tbatch {where[j]}{mode}{progress(i)}")
        return
    train_runs(chosen, runs_per_gpu=args.runs_per_gpu, run_ids=ids, group_mode=args.group_mode, resume=args.resume)


if __name__ == "__main__":
    main(sys.argv[1:])
