"""Post-hoc checkpoint evaluation: the second half of the reference's pen pipeline.

The reference's ``evaluation/minari/iql_eval.py``, ``iql_eval_median.py``, ``iql_stats.py`` and
``evaluation/d4rl/iql_eval_median.py`` load ``checkpoint["actor"]`` of one checkpoint, roll it out for
1,000 to 5,000 episodes (one batch-1 forward and one host wait per environment step) and append a row to a
CSV file; a W&B grid file lists about 200 checkpoints.  Here the M checkpoints of a file and R environments
per checkpoint advance in lock step: one ``iqlhip_mlp_set_forward`` launch per step for all M x R rows
(``MlpSet``, ``policy_actions_many``), with the numbers of the sequential program.

    python -m iqlpref_amd.posthoc FILE [--list] [--only i,j] [--lanes R] [--workers W]

Contract of ``evaluate_many``: the result equals the sequential program's whenever an episode depends only
on its seed and on the actions it receives.  gymnasium's ``reset(seed=)`` guarantees that; an environment
that reads a process-global generator is outside the contract."""
import argparse
import csv
import ctypes as C
import itertools
import functools
import os
import uuid
from dataclasses import dataclass, fields
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

# program: (dataset library, output kind)
PROGRAMS = {
    "evaluation/minari/iql_eval.py": ("minari", "mean"),
    "evaluation/minari/iql_eval_median.py": ("minari", "median"),
    "evaluation/minari/iql_stats.py": ("minari", "stats"),
    "evaluation/d4rl/iql_eval_median.py": ("d4rl", "median"),
}
SET_BYTES = 1 << 30  # one MlpSet holds at most this many bytes of weight images; more actors go in batches
MEAN_COLUMNS = ("dataset", "model_id", "checkpoint_id", "mean_score", "std_score", "normalized_mean_score",
                "normalized_std_score", "num_episodes")
MEDIAN_COLUMNS = ("dataset", "model_id", "checkpoint_id", "median_score", "num_episodes")


# --------------------------------------------------------------------------- #
# configs and grid files
# --------------------------------------------------------------------------- #
@dataclass
class EvalConfig:
    """The fields of the four programs' EvalConfig with their defaults.  ``dataset_id`` names the Minari
    dataset; the d4rl program calls the field ``env`` (a gym id), set it instead.  ``program`` (ours) says
    which of the four runs: it picks the seeding loop and the writer."""
    project: str = "IQL-eval"
    group: str = "IQL-eval"
    name: str = "eval"
    eval_csv: str = "~/iqlpref/task_reward_iql_results/pen_results.csv"
    actor_path: str = "~/iqlpref/human_pen_models/iql-D4RL/pen/human-v2-0f6ecda0/best_model.pt"
    iql_deterministic: bool = False
    actor_dropout: Optional[float] = 0.1
    dataset_id: str = "D4RL/pen/human-v2"
    env: Optional[str] = None
    normalize_state: bool = True
    eval_episodes: int = 1000
    eval_seed: int = 10
    program: str = "evaluation/minari/iql_eval.py"

    def __post_init__(self):
        if self.program not in PROGRAMS:
            raise ValueError(f"program {self.program!r} is none of {', '.join(PROGRAMS)}")
        self.name = f"{self.name}-{self.dataset}-{str(uuid.uuid4())[:8]}"

    @property
    def library(self) -> str:
        return PROGRAMS[self.program][0]

    @property
    def kind(self) -> str:
        return PROGRAMS[self.program][1]

    @property
    def dataset(self) -> str:
        """What the row's ``dataset`` column holds: ``env`` for the d4rl program, else ``dataset_id``."""
        return self.env if self.library == "d4rl" and self.env is not None else self.dataset_id


def _program_of(spec) -> str:
    program = str(spec.get("program") or "")
    for known in PROGRAMS:
        if program.endswith(known):
            return known
    raise ValueError(f"program {program!r} is none of the evaluation programs ({', '.join(PROGRAMS)}); "
                     "training grids go through sweep.expand_sweep")


def expand_eval_sweep(spec_or_path) -> List[EvalConfig]:
    """One EvalConfig per run of a W&B grid file whose ``program`` is one of the four evaluation programs
    (``sweep.expand_sweep`` refuses those).  ``sweep.sweep_axes``' rules: ``method: grid`` only,
    ``{value: x}`` / ``{values: [...]}`` entries, unknown names reported together; the runs are the product
    of the parameters in file order, the last one varying fastest."""
    from . import sweep
    from .iql import _coerce
    spec = sweep.load_sweep(spec_or_path)
    program = _program_of(spec)
    types = {f.name: f.type for f in fields(EvalConfig) if f.name != "program"}
    axes = sweep.sweep_axes(spec, known=set(types), what="EvalConfig fields")
    names = [n for n, _ in axes]
    out = []
    for combo in itertools.product(*[vals for _, vals in axes]):
        run = {n: _coerce(v, types[n]) for n, v in zip(names, combo)}
        out.append(EvalConfig(program=program, **run))
    return out


# --------------------------------------------------------------------------- #
# the grouped forward
# --------------------------------------------------------------------------- #
class MlpSet:
    """A frozen set of M ``MLP`` containers of one shape on the device (``iqlhip_mlp_set``): their weights are
    repacked once, ``forward`` is one launch for all of them.  A snapshot: later changes of the modules do not
    reach it.  Raises NotImplementedError for members wider than 256 (the caller then forwards them one by
    one) and ValueError for members of different shapes."""

    def __init__(self, nets: Sequence, device=None):
        import torch
        from . import _lib
        from .iql import mlp_desc
        self._lib = _lib.load()
        nets = list(nets)
        if not nets:
            raise ValueError("MlpSet needs at least one network")
        lin0 = nets[0].linears()
        self.device = _lib.require_gpu(lin0[0].weight.device if device is None else device)
        descs, keep = [], []
        for net in nets:
            lin = net.linears()
            # (a module in eval mode: no dropout, whatever the module's own mode is)
            d, k = mlp_desc([l.weight for l in lin], [l.bias for l in lin], w_in_out=False,
                            hidden_act=net._hidden_act, out_act=net._out_act)
            descs.append(d), keep.append(k)
        self.M, self.n_in, self.n_out = len(nets), int(descs[0].dims[0]), int(descs[0].dims[descs[0].n_layers])
        arr = (C.POINTER(_lib.MlpDesc) * self.M)(*[C.pointer(d) for d in descs])
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.iqlhip_mlp_set_create(arr, self.M, C.byref(handle), _lib.stream_ptr()))
        self._handle = handle

    def forward(self, x):
        """x [M, R, in] -> [M, R, out] (fp32, on the set's device)."""
        import torch
        from . import _lib
        if self._handle is None:
            raise RuntimeError("the set has been closed")
        x = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[0] != self.M or x.shape[2] != self.n_in:
            raise ValueError(f"x must be [{self.M}, R, {self.n_in}], got {tuple(x.shape)}")
        R = x.shape[1]
        out = torch.empty((self.M, R, self.n_out), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.iqlhip_mlp_set_forward(self._handle, _lib.ptr(x), R, self.n_in, _lib.ptr(out),
                                                        self.n_out, _lib.stream_ptr()))
        return out

    __call__ = forward

    def close(self):
        if getattr(self, "_handle", None) is not None:
            handle, self._handle = self._handle, None
            self._lib.iqlhip_mlp_set_destroy(handle)

    def __del__(self):
        self.close()


def policy_actions_many(actor_set: MlpSet, obs, max_action: float) -> np.ndarray:
    """Greedy actions of M actors for R observations each, obs [M, R, S] -> [M, R, A]: ``policy_actions``'
    expression on ONE grouped forward; row (m, r) carries the bits of ``policy_actions(actor_m, obs[m, r])``."""
    import torch
    states = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=actor_set.device)
    mean = actor_set.forward(states)
    return torch.clamp(max_action * mean, -max_action, max_action).cpu().numpy()


def set_batches(n_actors: int, image_floats: int) -> List[range]:
    """The actors of one shape in batches that fit one set: at most IQLHIP_MLP_SET_MAX members and SET_BYTES
    of weight images."""
    from . import _lib
    per = max(1, min(_lib.MLP_SET_MAX, SET_BYTES // max(1, 4 * image_floats)))
    return [range(i, min(i + per, n_actors)) for i in range(0, n_actors, per)]


def _image_floats(dims: Sequence[int]) -> int:
    up = [(d + 15) // 16 * 16 for d in dims]
    return sum(a * b + b for a, b in zip(up[:-1], up[1:]))


def load_actor(path: str, state_dim: int, action_dim: int, max_action: float, deterministic: bool, device,
               dropout: Optional[float] = None, strict: bool = True):
    """The policy stored under ``checkpoint["actor"]`` (the key contract of the training checkpoints), in eval
    mode.  ``hidden_dim`` and ``n_hidden`` are read from the tensor shapes, and whether the container has
    Dropout layers from the layer numbering of the keys (``dropout``: their p, which an evaluation never uses).
    ``strict=False`` is the d4rl program's ``load_state_dict(..., strict=False)``: a Gaussian checkpoint's
    ``log_std`` is ignored by a deterministic policy, a missing one stays at its initial zeros.  The file is
    read with ``weights_only=True`` (tensors and plain containers, which is all a training checkpoint holds):
    files this package did not write are never unpickled."""
    import torch
    from .iql import DeterministicPolicy, GaussianPolicy
    state = torch.load(os.path.expanduser(path), map_location=device, weights_only=True)["actor"]
    idx = sorted(int(k.split(".")[2]) for k in state if k.startswith("net.net.") and k.endswith(".weight"))
    if not idx:
        raise ValueError(f"{path}: checkpoint['actor'] holds no net.net.*.weight")
    first, last = state[f"net.net.{idx[0]}.weight"], state[f"net.net.{idx[-1]}.weight"]
    if first.shape[1] != state_dim or last.shape[0] != action_dim:
        raise ValueError(f"{path}: the actor maps {first.shape[1]} -> {last.shape[0]}, the environment has "
                         f"{state_dim} -> {action_dim}")
    n_hidden = len(idx) - 1
    has_dropout = n_hidden >= 1 and idx[1] - idx[0] == 3  # Linear, activation, Dropout
    p = (0.1 if dropout is None else dropout) if has_dropout else None
    cls = DeterministicPolicy if deterministic else GaussianPolicy
    actor = cls(state_dim, action_dim, max_action, hidden_dim=int(first.shape[0]), n_hidden=n_hidden,
                dropout=p).to(device)
    actor.load_state_dict(state, strict=strict)
    actor.eval()
    return actor


# --------------------------------------------------------------------------- #
# environments: in this process or in worker processes
# --------------------------------------------------------------------------- #
class _WorkerLanes:
    """``_env_worker.Lanes``' interface over ``workers`` processes; lane i lives in process i % workers.

    A worker is a fresh interpreter that runs ``_env_worker.py`` by path -- what multiprocessing's ``spawn``
    method starts, minus its re-import of the parent's main module, which under ``python -m
    iqlpref_amd.posthoc`` is this package: the worker imports nothing of the package, holds only the
    environments ``make_env`` builds, and inherits no state.  ``make_env`` is pickled here (a module-level
    function or a functools.partial of one; a lambda raises at once) and unpickled there under this process'
    ``sys.path``."""

    def __init__(self, make_env, n, workers, state_mean, state_std):
        import pickle
        import subprocess
        import sys
        from multiprocessing.connection import Listener
        from . import _env_worker
        try:
            factory = pickle.dumps(make_env)
        except Exception as e:
            raise TypeError(f"workers > 0 needs a picklable make_env (a module-level function or a "
                            f"functools.partial of one): {e}") from e
        self.W = max(1, min(int(workers), n))
        self.conns, self.procs = [], []
        key = os.urandom(32)
        try:
            with Listener(family="AF_UNIX", authkey=key) as listener:
                for w in range(self.W):
                    p = subprocess.Popen([sys.executable, os.path.abspath(_env_worker.__file__), listener.address],
                                         stdin=subprocess.PIPE)
                    self.procs.append(p)
                    p.stdin.write(key.hex().encode() + b"\n")
                    p.stdin.close()
                    self.conns.append(listener.accept())
            for w, c in enumerate(self.conns):
                c.send((list(sys.path), factory, len(range(w, n, self.W)), state_mean, state_std))
            for c in self.conns:
                self._answer(c)
        except BaseException:
            self.close()
            raise

    @staticmethod
    def _answer(conn):
        status, value = conn.recv()
        if status != "ok":
            raise RuntimeError(f"an environment worker failed:\n{value}")
        return value

    def _call(self, op, items):
        per = [[] for _ in range(self.W)]
        where = []
        for lane, v in items:
            w = lane % self.W
            where.append((w, len(per[w])))
            per[w].append((lane // self.W, v))
        busy = [w for w in range(self.W) if per[w]]
        for w in busy:
            self.conns[w].send((op, per[w]))
        got = {w: self._answer(self.conns[w]) for w in busy}
        return [got[w][i] if got[w] is not None else None for w, i in where]

    def seed(self, items):
        self._call("seed", items)

    def reset(self, items):
        return self._call("reset", items)

    def step(self, items):
        return self._call("step", items)

    def close(self):
        for c in self.conns:
            try:
                c.send(("close", None))
                c.close()
            except (OSError, EOFError):
                pass
        for p in self.procs:
            try:
                p.wait(timeout=10)
            except Exception:
                p.kill()
                p.wait()


# --------------------------------------------------------------------------- #
# the lock-step evaluation
# --------------------------------------------------------------------------- #
def _lock_step(lanes, M: int, R: int, num_episodes: int, seed: int, chain: bool, actions_fn) -> np.ndarray:
    """Lane m R + j is environment j of actor m.  Every pass: ONE ``actions_fn(obs [M, R, S]) -> [M, R, A]``,
    one step of every live lane, and a lane whose episode ended takes its actor's next unstarted episode."""
    returns = np.zeros((M, num_episodes), dtype=np.float64)
    episode = np.full((M, R), -1, dtype=np.int64)  # the episode a lane is running, -1: none
    next_ep = [0] * M
    total = [[0.0] * R for _ in range(M)]  # python floats: ``episode_reward += reward`` of the reference

    def start(cells):
        items = []
        for m, j in cells:
            i = next_ep[m]
            next_ep[m] += 1
            episode[m, j], total[m][j] = i, 0.0
            items.append((m * R + j, None if chain else seed + i))
        return lanes.reset(items)

    if chain:
        lanes.seed([(m * R, seed) for m in range(M)])
    first = [(m, j) for m in range(M) for j in range(R) if j < num_episodes]
    got = start(first)
    obs = None
    for (m, j), o in zip(first, got):
        o = np.asarray(o)
        if obs is None:
            obs = np.zeros((M, R) + o.shape, dtype=o.dtype)
        obs[m, j] = o
    live = list(first)
    while live:
        actions = actions_fn(obs)
        stepped = lanes.step([(m * R + j, actions[m, j]) for m, j in live])
        ended = []
        for (m, j), (o, reward, done) in zip(live, stepped):
            obs[m, j] = o
            total[m][j] += reward
            if done:
                returns[m, episode[m, j]] = total[m][j]
                episode[m, j] = -1
                ended.append((m, j))
        again, left = [], [num_episodes - n for n in next_ep]
        for m, j in ended:  # (several lanes of one actor may end in the same step)
            if left[m] > 0:
                left[m] -= 1
                again.append((m, j))
        for (m, j), o in zip(again, start(again)):
            obs[m, j] = o
        live = [c for c in live if episode[c] >= 0]  # a lane that ran out keeps its last observation
    return returns


def _solo_actions(actors, max_action, device):
    from .train import policy_actions

    def fn(obs):
        return np.stack([policy_actions(a, obs[m], max_action, device) for m, a in enumerate(actors)])
    return fn


def _actor_dims(actor) -> List[int]:
    return list(actor.net._dims)


def evaluate_many(make_env: Callable[[], Any], actors: Sequence, num_episodes: int, seed: int, *,
                  episode_seeding: str = "reset", lanes: Optional[int] = None, workers: int = 0,
                  state_mean=0.0, state_std=1.0, device="cuda", actions_fn=None) -> np.ndarray:
    """Returns [M, num_episodes] (float64) of M actors, episode i of every actor in column i.

    ``episode_seeding="reset"`` is the Minari programs' loop: episode i is ``env.reset(seed=seed + i)``, greedy
    actions until ``terminated or truncated``, the return accumulated step by step.  R = ``lanes``
    environments per actor (default min(16, num_episodes)) each take the actor's next unstarted episode when
    theirs ends.  ``"chain"`` is the d4rl program's loop: ``env.seed(seed)`` once per actor, then the episodes
    one after another on that environment; one lane per actor, the M actors side by side.

    Every lock step is ONE ``policy_actions_many`` call on an ``MlpSet`` of the actors (in batches of what one
    set holds); actors wider than the set's envelope (256) go through per-actor ``policy_actions``, with the
    same results.  Observations are normalised on the host by ``wrap_env``.  ``workers=0`` steps the
    environments in this process, ``workers=W`` in W freshly started interpreters that hold only
    environments and import nothing of this package (``_WorkerLanes``; ``make_env`` must then be picklable).  The actors are evaluated in eval mode and come back
    in the mode they had.  ``actions_fn`` (tests): obs [M, R, S] -> actions [M, R, A] in place of the device.

    Contract: the result equals the sequential program's whenever an episode depends only on its seed and
    the actions it receives.  ``reset(seed=)`` guarantees this in gymnasium; an environment that reads a
    process-global generator is outside the contract."""
    from . import _env_worker
    if episode_seeding not in ("reset", "chain"):
        raise ValueError("episode_seeding must be 'reset' or 'chain'")
    actors = list(actors)
    M, num_episodes = len(actors), int(num_episodes)
    if M < 1 or num_episodes < 1:
        raise ValueError("evaluate_many needs at least one actor and one episode")
    chain = episode_seeding == "chain"
    R = 1 if chain else max(1, min(int(lanes) if lanes is not None else 16, num_episodes))
    out = np.zeros((M, num_episodes), dtype=np.float64)
    if actions_fn is not None:
        batches = [(range(M), actions_fn)]
    else:
        batches = _device_batches(actors, device)
    modes = [getattr(a, "training", None) for a in actors]
    try:
        for a, mode in zip(actors, modes):
            if mode:
                a.eval()
        for members, fn in batches:
            n = len(members) * R
            env_lanes = (_WorkerLanes(make_env, n, workers, state_mean, state_std) if workers
                         else _env_worker.Lanes(make_env, n, state_mean, state_std))
            try:
                out[list(members)] = _lock_step(env_lanes, len(members), R, num_episodes, int(seed), chain,
                                                fn() if actions_fn is None else fn)
            finally:
                env_lanes.close()
    finally:
        for a, mode in zip(actors, modes):
            if mode:
                a.train()
    return out


def _device_batches(actors, device):
    """[(member indices, thunk -> actions_fn)]: sets of equal-shaped actors, per-actor calls for wide ones."""
    from . import _lib
    max_action = float(actors[0].max_action)
    if any(float(a.max_action) != max_action for a in actors):
        raise ValueError("the actors of one evaluation share max_action")
    groups: Dict[tuple, List[int]] = {}
    for i, a in enumerate(actors):
        groups.setdefault((tuple(_actor_dims(a)), a.net._hidden_act, a.net._out_act), []).append(i)
    out = []
    for (dims, _, _), idx in groups.items():
        if max(dims) > _lib.MLP_SET_MAX_WIDTH:
            out.append((idx, lambda idx=idx: _solo_actions([actors[i] for i in idx], max_action, device)))
            continue
        for part in set_batches(len(idx), _image_floats(dims)):
            ids = [idx[i] for i in part]

            def make(ids=ids):
                actor_set = MlpSet([actors[i].net for i in ids], device)
                return lambda obs: policy_actions_many(actor_set, obs, max_action)
            out.append((ids, make))
    return out


class _Borrowed:
    """The caller's environment as one lane: everything is the environment's, but it is not ours to close."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def close(self):
        pass


def evaluate(env, actor, num_episodes: int, seed: int, device) -> np.ndarray:
    """The Minari programs' ``evaluate`` (one actor on ``env``): ``evaluate_many`` with one actor, one lane."""
    return evaluate_many(lambda: _Borrowed(env), [actor], num_episodes, seed, lanes=1, device=device)[0]


# --------------------------------------------------------------------------- #
# the three outputs
# --------------------------------------------------------------------------- #
def path_ids(actor_path: str):
    """(model_id, checkpoint_id) as the programs parse them from ``.../<run>-<model_id>/<name>_<id>.pt``."""
    parts = os.path.expanduser(actor_path).split("/")
    return parts[-2].split("-")[-1], parts[-1].split(".")[0].split("_")[-1]


def _append_row(eval_csv: str, columns: Sequence[str], row: Dict[str, Any]) -> None:
    path = os.path.expanduser(eval_csv)
    fresh = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, "a", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        if fresh:
            w.writerow(columns)
        w.writerow(["" if row[c] is None else row[c] for c in columns])


def write_mean_row(eval_csv: str, dataset: str, actor_path: str, scores: np.ndarray,
                   normalized_score: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> Dict[str, Any]:
    """The row of ``iql_eval.py``: mean and ddof-1 std of the returns, and of ``normalized_score(scores) * 100``
    when the callable is given (else the two columns are empty)."""
    scores = np.asarray(scores, dtype=np.float64)
    model_id, checkpoint_id = path_ids(actor_path)
    mean_n = std_n = None
    if normalized_score is not None:
        n = np.asarray(normalized_score(scores)) * 100
        mean_n, std_n = float(n.mean()), float(n.std(ddof=1))
    row = {"dataset": dataset, "model_id": model_id, "checkpoint_id": checkpoint_id,
           "mean_score": float(scores.mean()), "std_score": float(scores.std(ddof=1)),
           "normalized_mean_score": mean_n, "normalized_std_score": std_n, "num_episodes": int(len(scores))}
    _append_row(eval_csv, MEAN_COLUMNS, row)
    return row


def write_median_row(eval_csv: str, dataset: str, actor_path: str, scores: np.ndarray) -> Dict[str, Any]:
    """The row of ``iql_eval_median.py``."""
    scores = np.asarray(scores, dtype=np.float64)
    model_id, checkpoint_id = path_ids(actor_path)
    row = {"dataset": dataset, "model_id": model_id, "checkpoint_id": checkpoint_id,
           "median_score": float(np.median(scores)), "num_episodes": int(len(scores))}
    _append_row(eval_csv, MEDIAN_COLUMNS, row)
    return row


def write_stats(eval_csv: str, scores: np.ndarray) -> None:
    """``iql_stats.py``: the raw returns, one per line (``np.savetxt``; the file is replaced)."""
    np.savetxt(os.path.expanduser(eval_csv), np.asarray(scores, dtype=np.float64), delimiter=",")


def write_result(config: EvalConfig, scores: np.ndarray, normalized_score=None):
    if config.kind == "mean":
        return write_mean_row(config.eval_csv, config.dataset, config.actor_path, scores, normalized_score)
    if config.kind == "median":
        return write_median_row(config.eval_csv, config.dataset, config.actor_path, scores)
    return write_stats(config.eval_csv, scores)


# --------------------------------------------------------------------------- #
# a whole grid file
# --------------------------------------------------------------------------- #
def group_key(config: EvalConfig) -> tuple:
    """Runs that may share one ``evaluate_many`` call (besides the actors' shapes, read from the checkpoints)."""
    return (config.library, config.dataset, bool(config.normalize_state), bool(config.iql_deterministic),
            int(config.eval_episodes), int(config.eval_seed))


def plan(configs: Sequence[EvalConfig]) -> List[List[int]]:
    """Indices of ``configs`` per group, groups in order of their first run."""
    groups: Dict[tuple, List[int]] = {}
    for i, c in enumerate(configs):
        groups.setdefault(group_key(c), []).append(i)
    return list(groups.values())


def make_minari_env(dataset_id: str):
    """A fresh environment of a Minari dataset on this machine (module-level: workers unpickle it by name and
    load the dataset themselves)."""
    import minari
    return minari.load_dataset(dataset_id).recover_environment()


def make_d4rl_env(env_name: str):
    import gym
    import d4rl  # noqa: F401 (registers the environments)
    return gym.make(env_name)


def _minari_source(dataset_id: str):
    """(make_env, observations, normalized_score) of a Minari dataset that is already on this machine
    (``minari.load_dataset`` reads local storage and raises when the dataset is not there; ``download_dataset``
    is never called)."""
    import minari
    dataset = minari.load_dataset(dataset_id)
    observations = np.concatenate([ep.observations[:-1].astype(np.float32) for ep in dataset])

    def normalized_score(scores):
        return minari.get_normalized_score(dataset, scores)
    return functools.partial(make_minari_env, dataset_id), observations, normalized_score


def _d4rl_source(env_name: str):
    """(make_env, observations, None) of a d4rl environment whose dataset file is already in d4rl's cache.
    ``env.get_dataset()`` without a path would fetch a missing file from the dataset's URL, so the cached
    file is looked up first and handed over, and a missing one raises FileNotFoundError."""
    import d4rl
    from d4rl.offline_env import filepath_from_url
    env = make_d4rl_env(env_name)
    try:
        url = getattr(env.unwrapped, "dataset_url", None)
        path = None if url is None else filepath_from_url(url)
        if path is None or not os.path.exists(path):
            raise FileNotFoundError(f"{env_name}: the dataset file {path!r} is not in d4rl's cache; this module "
                                    "never fetches (download it with d4rl itself first)")
        data = d4rl.qlearning_dataset(env, dataset=env.get_dataset(h5path=path))
    finally:
        env.close()
    return functools.partial(make_d4rl_env, env_name), data["observations"], None


def run(configs: Sequence[EvalConfig], make_env=None, dataset=None, *, lanes: Optional[int] = None,
        workers: int = 0, device="cuda", only: Optional[Sequence[int]] = None, normalized_score=None,
        log: Callable[[str], None] = print) -> List[np.ndarray]:
    """Evaluate every config and write its output; returns the returns per config (None for runs left out by
    ``only``).  The configs are grouped by (dataset, shape, policy kind) and each group goes through one
    ``evaluate_many``; the rows are written in file order, each as soon as every run before it in the file is
    done (a file that is one group: when the group ends), so a failure in a later group loses nothing finished.  ``make_env`` () -> a fresh environment and
    ``dataset`` (a mapping with "observations") replace the lookup by name: without them a Minari dataset is
    loaded with ``minari.load_dataset`` / ``recover_environment()`` and a d4rl one with gym + d4rl (imported
    here).  Nothing is downloaded: a Minari dataset or a d4rl dataset file that is not on this machine raises.  State statistics (``compute_mean_std``, eps 1e-3) are computed once per
    dataset when a run normalises."""
    from .iql import compute_mean_std
    configs = list(configs)
    chosen = set(range(len(configs)) if only is None else only)
    scores: List[Optional[np.ndarray]] = [None] * len(configs)
    sources: Dict[tuple, tuple] = {}
    stats: Dict[tuple, tuple] = {}
    written = 0

    def flush():  # every finished run that no unfinished chosen run precedes
        nonlocal written
        while written < len(configs) and (written not in chosen or scores[written] is not None):
            c = configs[written]
            if scores[written] is not None:
                write_result(c, scores[written], sources[(c.library, c.dataset)][2])
            written += 1

    for members in plan(configs):
        members = [i for i in members if i in chosen]
        if not members:
            continue
        c0 = configs[members[0]]
        src = (c0.library, c0.dataset)
        if src not in sources:
            if make_env is not None:
                sources[src] = (make_env, None if dataset is None else np.asarray(dataset["observations"]),
                                normalized_score)
            else:
                sources[src] = _d4rl_source(c0.dataset) if c0.library == "d4rl" else _minari_source(c0.dataset)
        mk, observations, _ = sources[src]
        mean, std = 0.0, 1.0
        if c0.normalize_state:
            if observations is None:
                raise ValueError("normalize_state needs the dataset's observations (pass dataset=)")
            if src not in stats:
                stats[src] = compute_mean_std(observations, eps=1e-3)
            mean, std = stats[src]
        probe = mk()
        state_dim, action_dim = probe.observation_space.shape[0], probe.action_space.shape[0]
        max_action = float(probe.action_space.high[0])
        close = getattr(probe, "close", None)
        if close is not None:
            close()
        actors = [load_actor(configs[i].actor_path, state_dim, action_dim, max_action, c0.iql_deterministic, device,
                             dropout=configs[i].actor_dropout, strict=c0.library != "d4rl") for i in members]
        log(f"group {c0.dataset} ({len(members)} checkpoints, {c0.eval_episodes} episodes)")
        got = evaluate_many(mk, actors, c0.eval_episodes, c0.eval_seed,
                            episode_seeding="chain" if c0.library == "d4rl" else "reset", lanes=lanes,
                            workers=workers, state_mean=mean, state_std=std, device=device)
        for i, row in zip(members, got):
            scores[i] = row
        flush()
    return scores


def describe(configs: Sequence[EvalConfig], lanes: Optional[int] = None) -> str:
    """The plan as ``--list`` prints it: runs, groups and set batches (at the default 2 x 256 shape a batch is
    bounded by IQLHIP_MLP_SET_MAX; the actual shapes are read from the checkpoints when the run starts)."""
    from . import _lib
    lines = [f"{len(configs)} runs"]
    for g, members in enumerate(plan(configs)):
        c = configs[members[0]]
        R = 1 if c.library == "d4rl" else max(1, min(lanes if lanes is not None else 16, c.eval_episodes))
        batches = -(-len(members) // _lib.MLP_SET_MAX)
        lines.append(f"group {g}: {c.program} {c.dataset} {'deterministic' if c.iql_deterministic else 'gaussian'} "
                     f"{len(members)} checkpoints x {c.eval_episodes} episodes, seed {c.eval_seed}, "
                     f"{R} lanes each, {batches} set batch{'es' if batches != 1 else ''} -> {c.eval_csv}")
        for i in members:
            lines.append(f"  run {i}: {configs[i].actor_path}")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m iqlpref_amd.posthoc",
                                 description="Evaluate the checkpoints of a W&B evaluation grid file in lock step.")
    ap.add_argument("sweep", help="grid file whose program is one of the evaluation programs")
    ap.add_argument("--list", action="store_true", help="print the plan (runs, groups, batches); no device work")
    ap.add_argument("--only", default=None, help="comma-separated run indices")
    ap.add_argument("--lanes", type=int, default=None, help="environments per checkpoint (default 16)")
    ap.add_argument("--workers", type=int, default=None, help="environment processes (default min(16, lanes))")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    configs = expand_eval_sweep(args.sweep)
    only = None if args.only is None else [int(t) for t in args.only.split(",") if t != ""]
    if only is not None and any(not 0 <= i < len(configs) for i in only):
        raise SystemExit(f"--only: run indices are 0..{len(configs) - 1}")
    if args.list:
        print(describe(configs, args.lanes))
        return 0
    lanes = 16 if args.lanes is None else args.lanes
    workers = min(16, lanes) if args.workers is None else args.workers
    run(configs, lanes=lanes, workers=workers, device=args.device, only=only)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
