"""``algorithms/offline/any_percent_bc.py`` ("dbc"): the D4RL any-percent behaviour-cloning baseline -- keep the
``frac`` of the trajectories of a D4RL transition dataset with the greatest discounted return, clone their actions
with one ``Actor`` under ``F.mse_loss`` and plain Adam.  The baseline of the antmaze / halfcheetah tables beside
``iqlpref_amd.train``.

The step is ``minari_bc``'s kernel pair (csrc/bc_step.hip, ``iqlhip_bc_*``: fp32, the 256-256 actor,
``state_dim`` <= 128, ``action_dim`` <= 32, 1..16 members).  What this flavour adds is the selection: dbc:206-239
walks every transition of a ~1M-row dataset in Python and then fancy-indexes the five arrays.  Here
``select_best_trajectories`` cuts the dataset into trajectories and sums their returns on the device
(``iqlhip_prep_trajectory_returns``), ranks the few thousand returns on the host with the reference's own numpy
expression, and copies the chosen trajectories, best first, with one ``iqlhip_prep_gather_trajectories`` per array.
What is kept from dbc, because it decides what a run computes:

* a trajectory ends at a row with ``done == 1.0`` or after ``max_episode_steps`` rows; a trailing run that reaches
  neither is dropped (dbc:217-226);
* ``cur_return += reward_scale * reward`` (dbc:218) runs in the dtype of the stored rewards: on float32 rewards
  numpy 2 rounds the Python float ``reward_scale`` to float32, multiplies in float32 and adds in float32, while
  ``reward_scale *= discount`` (dbc:220) stays Python double arithmetic -- so the factor of row k is
  ``float32(s_k)``, ``s_0 = 1.0``, ``s_{k+1} = s_k * discount``, never ``discount ** k``
  (``return_scale_table``).  The device walker adds the same products in the same order with every product and
  sum rounded on its own: returns are bit-identical.  float64 rewards follow numpy's float64 arithmetic, on the
  host (``keep_best_trajectories``);
* the ranking is ``np.argsort(returns, axis=0)[::-1]`` (dbc:228), an UNSTABLE sort: among equal returns (antmaze
  has them by the thousand) the order is whatever numpy's sort kernel on this host gives.  It runs on the host, on
  the returns the device hands back, as that very expression -- there is no device sort;
  ``max(1, int(frac * n_traj))`` trajectories are kept (dbc:229);
* the rows lie in the order of the chosen trajectories, best first (dbc:231-239): that decides which row an index
  names; the state statistics are those of the selected rows with ``eps=1e-3`` (dbc:324-325);
* indices come from ``np.random.randint(0, min(size, pointer), size=B)`` on numpy's global generator (dbc:148),
  drawn on the host or by ``custom_offline.NumpyIndexStream``;
* one ``{"actor_loss"}`` record per step at ``step=total_it`` (one-based, dbc:386), at ``(t + 1) % eval_freq == 0``
  an evaluation with the old gym API -- ``env.seed(seed)`` once, then chained episodes (dbc:186-203) --, a
  ``d4rl_normalized_score = env.get_normalized_score(mean) * 100`` record, and ``checkpoint_{t}.pt`` with the
  ZERO-based ``t`` (dbc:407-416); ``BC.state_dict`` has dbc's three keys (dbc:300-305).

Two quirks of dbc's ``train()`` are kept on purpose:

* it calls ``keep_best_trajectories(dataset, config.frac, config.discount)`` (dbc:322) and never passes
  ``config.max_traj_len``: the cut is always 1000 rows, whatever the config says;
* ``config.discount`` reaches ``BC`` (dbc:363) and is unused there.
"""
import ctypes as C
import os
import uuid
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _d4rl, _lib, _offline_loop, minari_bc
from . import custom_offline as _co
from ._d4rl import eval_actor  # noqa: F401  (dbc:186-203: greedy actions from ``actor.act``)
from ._lib import check, ptr, stream_ptr
from .iql import load_config_for, compute_mean_std, normalize_states, set_seed  # noqa: F401  (dbc:68-75, 162-172)
from .minari_bc import Actor, check_envelope, stepper  # (dbc:242-263 is minari_bc.Actor)
from .train import wrap_env  # noqa: F401  (dbc:78-97)

TensorBatch = List[torch.Tensor]
MAX_TRAJ_LEN = 1 << 20  # iqlhip_prep_trajectory_returns: the longest cut
ARRAYS = ("observations", "actions", "next_observations", "rewards", "terminals")  # dbc:235-239


@dataclass
class TrainConfig:
    """dbc:21-60, same fields and defaults."""
    project: str = "CORL"
    group: str = "BC-D4RL"
    name: str = "BC"
    env: str = "halfcheetah-medium-expert-v2"
    max_timesteps: int = int(1e6)
    batch_size: int = 256
    buffer_size: int = 2_000_000
    frac: float = 0.1
    max_traj_len: int = 1000  # (never read by train(): dbc:322)
    normalize: bool = True
    discount: float = 0.99
    eval_freq: int = int(5e3)
    n_episodes: int = 10
    checkpoints_path: Optional[str] = None
    load_model: str = ""
    seed: int = 0
    device: str = "cuda"

    def __post_init__(self):
        self.name = f"{self.name}-{self.env}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)


def load_config(config_path: Optional[str] = None, **overrides) -> TrainConfig:
    """The pyrallis ``--config_path`` behaviour (dbc:313) with ``iql.load_config``'s rules."""
    return load_config_for(TrainConfig, "offline_bc.TrainConfig", config_path, **overrides)


# --------------------------------------------------------------------------- #
# selection (dbc:206-239)
# --------------------------------------------------------------------------- #
def return_scale_table(discount: float, max_len: int, dtype=np.float32) -> np.ndarray:
    """``table[k]`` = the factor dbc:218 multiplies the k-th reward of a trajectory by, in ``dtype``:
    ``reward_scale`` is a Python float that starts at 1.0 and is multiplied by ``discount`` once per row
    (dbc:216, 220), and numpy rounds it to the rewards' dtype at each use."""
    table = np.empty(int(max_len), dtype=dtype)
    s = 1.0
    for k in range(int(max_len)):
        table[k] = s
        s *= discount
    return table


def _done_flags(terminals) -> np.ndarray:
    return np.asarray(terminals).reshape(-1) == 1.0  # dbc:221 `done == 1.0`


def trajectory_bounds(done: np.ndarray, max_len: int) -> Tuple[np.ndarray, np.ndarray]:
    """(starts, lengths), int64, of the complete trajectories in dataset order (dbc:217-226): a run of rows up to
    and including a done row is cut into pieces of ``max_len`` rows, its last piece taking what is left; the
    rows behind the last done row give whole pieces only."""
    done = np.asarray(done, bool).reshape(-1)
    n, M = done.shape[0], int(max_len)
    ends = np.flatnonzero(done)
    seg_start = np.concatenate(([0], ends + 1)).astype(np.int64)
    seg_len = np.concatenate((ends + 1, [n])).astype(np.int64) - seg_start
    pieces = -(-seg_len // M)
    pieces[-1] = seg_len[-1] // M  # the trailing run ends on no done row
    n_traj = int(pieces.sum())
    seg = np.repeat(np.arange(len(pieces)), pieces)
    within = np.arange(n_traj, dtype=np.int64) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    starts = seg_start[seg] + within * M
    lengths = np.minimum(M, seg_start[seg] + seg_len[seg] - starts)
    return starts, lengths


def trajectory_returns(rewards: np.ndarray, starts: np.ndarray, lengths: np.ndarray, discount: float) -> np.ndarray:
    """The ``returns`` list of dbc:213-223 as an array of the rewards' dtype, bit-equal to the loop for float32
    and float64 rewards: row k of every trajectory is added at pass k, so each trajectory sees its own products
    in row order (other dtypes: the loop itself)."""
    rewards = np.asarray(rewards).reshape(-1)
    if rewards.dtype not in (np.float32, np.float64):
        out = []
        for s, L in zip(starts.tolist(), lengths.tolist()):
            cur, scale = 0, 1.0
            for r in rewards[s:s + L]:
                cur += scale * r
                scale *= discount
            out.append(cur)
        return np.asarray(out)
    n_traj = len(starts)
    if n_traj == 0:
        return np.zeros(0, rewards.dtype)
    table = return_scale_table(discount, int(lengths.max()), rewards.dtype)
    by_len = np.argsort(-lengths, kind="stable")  # longest first: the trajectories with a row k are a prefix
    s_sorted, neg_len = starts[by_len], -lengths[by_len]
    cur = np.zeros(n_traj, rewards.dtype)
    for k in range(int(lengths.max())):
        live = int(np.searchsorted(neg_len, -k, side="left"))  # trajectories with length > k
        cur[:live] += table[k] * rewards[s_sorted[:live] + k]
    out = np.empty_like(cur)
    out[by_len] = cur
    return out


def rank_trajectories(returns: np.ndarray, frac: float) -> np.ndarray:
    """dbc:228-229 as written: the numbers of the kept trajectories, best first.  ``np.argsort`` is numpy's
    default unstable sort: the order among equal returns is this host's."""
    sort_ord = np.argsort(returns, axis=0)[::-1].reshape(-1)
    return sort_ord[: max(1, int(frac * len(sort_ord)))]


def keep_best_trajectories(dataset: Dict[str, np.ndarray], frac: float, discount: float,
                           max_episode_steps: int = 1000):
    """dbc:206-239 on the host, in place, without the loop over the rows; bit-equal to it (``trajectory_returns``).
    A dataset without a complete trajectory raises IndexError, as the reference's empty ``order`` does."""
    rewards = np.asarray(dataset["rewards"])
    starts, lengths = trajectory_bounds(_done_flags(dataset["terminals"]), max_episode_steps)
    if len(starts) == 0:
        raise IndexError("arrays used as indices must be of integer (or boolean) type: the dataset holds no "
                         "complete trajectory")
    top = rank_trajectories(trajectory_returns(rewards, starts, lengths, discount), frac)
    L = lengths[top]
    order = np.repeat(starts[top] - (np.cumsum(L) - L), L) + np.arange(int(L.sum()), dtype=np.int64)
    for k in ARRAYS:
        dataset[k] = dataset[k][order]


def device_trajectory_returns(rewards: torch.Tensor, done: torch.Tensor, discount: float, max_episode_steps: int):
    """``iqlhip_prep_trajectory_returns``: (starts int64 [n_traj], lengths int64 [n_traj], returns float32
    [n_traj]) device tensors for contiguous device ``rewards`` float32 [n] and ``done`` uint8 [n].  ValueError
    when no trajectory is complete (nothing is written then)."""
    lib = _lib.load()
    dev = _lib.require_gpu(rewards.device)
    if rewards.dtype != torch.float32 or done.dtype != torch.uint8 or rewards.dim() != 1 or done.shape != rewards.shape:
        raise ValueError("rewards float32 [n] and done uint8 [n]")
    n, M = rewards.shape[0], int(max_episode_steps)
    if n < 1 or M < 1:
        raise ValueError("n and max_episode_steps must be >= 1")
    if M > MAX_TRAJ_LEN:
        raise NotImplementedError(f"max_episode_steps {M} is beyond {MAX_TRAJ_LEN}")
    rewards, done = rewards.contiguous(), done.contiguous()
    scale = torch.from_numpy(return_scale_table(discount, min(M, n))).to(dev)  # (a trajectory has at most n rows)
    starts = torch.empty(n, dtype=torch.int64, device=dev)
    lengths = torch.empty(n, dtype=torch.int64, device=dev)
    returns = torch.empty(n, dtype=torch.float32, device=dev)
    count = C.c_int64(0)
    with torch.cuda.device(dev):
        check(lib.iqlhip_prep_trajectory_returns(ptr(rewards), ptr(done), n, M, ptr(scale), ptr(starts), ptr(lengths),
                                                 ptr(returns), C.byref(count), stream_ptr()))
    k = count.value
    return starts[:k], lengths[:k], returns[:k]


def gather_trajectories(src: torch.Tensor, starts: torch.Tensor, lengths: torch.Tensor, chosen: torch.Tensor,
                        offsets: torch.Tensor, total_rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``iqlhip_prep_gather_trajectories``: the rows of the trajectories ``chosen`` (int64 device [m]) of ``src``
    (float32 device [n] or [n, width]) in that order, ``offsets`` = the exclusive prefix sum of their lengths.
    ``out``: where to write (its first ``total_rows`` rows), default a fresh tensor of exactly that many rows."""
    lib = _lib.load()
    dev = _lib.require_gpu(src.device)
    if src.dtype != torch.float32 or src.dim() not in (1, 2) or not src.is_contiguous():
        raise ValueError("src must be a contiguous float32 device tensor [n] or [n, width]")
    n, width = src.shape[0], (1 if src.dim() == 1 else src.shape[1])
    shape = (total_rows,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] < total_rows or out.shape[1:] != src.shape[1:]:
        raise ValueError("out must be a contiguous float32 tensor of at least total_rows rows of src's width")
    with torch.cuda.device(dev):
        check(lib.iqlhip_prep_gather_trajectories(ptr(src), n, width, ptr(starts), ptr(lengths), starts.shape[0],
                                                  ptr(chosen), ptr(offsets), chosen.shape[0], int(total_rows), ptr(out),
                                                  stream_ptr()))
    return out


def select_best_trajectories(observations, actions, next_observations, rewards, terminals, frac: float,
                             discount: float, max_episode_steps: int = 1000, *, device="cuda"):
    """dbc:206-239 on the device.  The five arrays are numpy arrays or tensors, on the host or the device;
    ``rewards`` must be float32 (TypeError otherwise: float64 rewards sum in float64, ``keep_best_trajectories``).
    Returns ``(selected, chosen)``: ``selected`` maps the five names to float32 device tensors holding exactly the
    rows of the kept trajectories, best first (terminals as 0.0 / 1.0, what the buffer stores); ``chosen`` is the
    int64 numpy array of their numbers in dataset order.  One host wait for the trajectory count, one copy of the
    returns to the host for the ranking (``rank_trajectories``), no other.  ValueError when the dataset holds no
    complete trajectory."""
    rew_dtype = rewards.dtype if torch.is_tensor(rewards) else np.asarray(rewards).dtype
    if rew_dtype not in (torch.float32, np.float32):
        raise TypeError(f"select_best_trajectories takes float32 rewards, not {rew_dtype}")
    dev = _lib.require_gpu(device)
    up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
    rew, term = up(rewards).reshape(-1).contiguous(), up(terminals).reshape(-1)
    done = (term == 1.0).to(torch.uint8)
    starts, lengths, returns = device_trajectory_returns(rew, done, discount, max_episode_steps)
    chosen = np.ascontiguousarray(rank_trajectories(returns.cpu().numpy(), frac)).astype(np.int64)
    chosen_d = torch.from_numpy(chosen).to(dev)
    L = lengths[chosen_d]
    ends = torch.cumsum(L, 0)
    offsets, total = (ends - L).contiguous(), int(ends[-1].item())
    f32 = lambda t: t.to(torch.float32).contiguous()
    sources = dict(zip(ARRAYS, (f32(up(observations)), f32(up(actions)), f32(up(next_observations)), rew, f32(term))))
    return {k: gather_trajectories(v, starts, lengths, chosen_d, offsets, total) for k, v in sources.items()}, chosen


# --------------------------------------------------------------------------- #
# buffer, trainer (dbc:100-159, 266-310; the evaluation, dbc:186-203, is ``_d4rl.eval_actor``)
# --------------------------------------------------------------------------- #
class ReplayBuffer(_co.ReplayBuffer):
    """dbc:100-159 on the packed device rows: ``load_d4rl_dataset`` (its two ``ValueError``s, dbc:129-136),
    ``sample`` on ``np.random.randint(0, min(size, pointer), size=B)`` of numpy's global generator (dbc:148);
    ``add_transition`` raises ``NotImplementedError`` (dbc:156-159)."""


class BC(minari_bc.BC):
    """dbc:266-310 on ``minari_bc.BC``'s kernels and arenas: the reference's constructor -- ``discount`` is kept
    and, as there, never used -- and its three-key state dict."""

    def __init__(self, max_action, actor: nn.Module, actor_optimizer: torch.optim.Optimizer, discount: float = 0.99,
                 device: str = "cpu", *, keep_grads: bool = False):
        super().__init__(max_action, actor, actor_optimizer, device, keep_grads=keep_grads)
        self.discount = discount

    def state_dict(self) -> Dict[str, Any]:
        return dict(minari_bc.BC.state_dict(self), total_it=self.total_it)

    def load_state_dict(self, state_dict: Dict[str, Any]):
        """dbc:307-310.  The kernels count Adam's steps and the trainer's iterations as one number, which they
        are in every file dbc's or this ``train()`` writes; a file in which they differ is a ValueError."""
        minari_bc.BC.load_state_dict(self, state_dict)  # (total_it := the optimiser's step count)
        if int(state_dict["total_it"]) != self.total_it:
            raise ValueError(f"total_it {state_dict['total_it']} is not the optimiser's step count {self.total_it}")


# --------------------------------------------------------------------------- #
# train (dbc:313-416)
# --------------------------------------------------------------------------- #
def _build_trainer(seed: int, state_dim: int, action_dim: int, max_action: float, discount: float, device: str) -> BC:
    """dbc:356-372 for one seed: the net is built right after ``torch.manual_seed(seed)`` on the CPU generator,
    then moved to the device."""
    torch.manual_seed(seed)
    actor = Actor(state_dim, action_dim, max_action).to(device)
    return BC(max_action=max_action, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
              discount=discount, device=device)


def _load_selected(config: TrainConfig, dataset: Dict[str, np.ndarray], state_dim: int, action_dim: int, device: str):
    """dbc:322-342: selection, state statistics of the selected rows, normalised rows in the buffer.  float32
    rewards: on the device (``select_best_trajectories``; the statistics are numpy's, of the selected
    observations copied back, and the z-scoring is fused into the buffer load), ``dataset`` is left as it is.
    Any other reward dtype: the host restatement, which rewrites ``dataset`` as the reference does.  Returns
    (replay buffer, state_mean, state_std)."""
    replay_buffer = ReplayBuffer(state_dim, action_dim, config.buffer_size, device)
    rewards = dataset["rewards"]
    if (rewards.dtype if torch.is_tensor(rewards) else np.asarray(rewards).dtype) in (torch.float32, np.float32):
        sel, _ = select_best_trajectories(*[dataset[k] for k in ARRAYS], config.frac, config.discount, device=device)
        mean_d = std_d = None
        state_mean, state_std = 0, 1
        if config.normalize:
            state_mean, state_std = compute_mean_std(sel["observations"].cpu().numpy(), eps=1e-3)
            mean_d, std_d = torch.from_numpy(state_mean).to(device), torch.from_numpy(state_std).to(device)
        replay_buffer.load_device_arrays(sel["observations"], sel["actions"], sel["rewards"], sel["next_observations"],
                                         sel["terminals"], mean_d, std_d)
        return replay_buffer, state_mean, state_std
    keep_best_trajectories(dataset, config.frac, config.discount)
    if config.normalize:
        state_mean, state_std = compute_mean_std(dataset["observations"], eps=1e-3)
    else:
        state_mean, state_std = 0, 1
    dataset["observations"] = normalize_states(dataset["observations"], state_mean, state_std)
    dataset["next_observations"] = normalize_states(dataset["next_observations"], state_mean, state_std)
    replay_buffer.load_d4rl_dataset(dataset)
    return replay_buffer, state_mean, state_std


class _Records(_offline_loop.Records):
    """dbc:386, 413-416: every record at ``step=trainer.total_it``, one-based and continuing a loaded model's count
    (``first_it``); an evaluation logs ``d4rl_normalized_score``, the score of the mean return x 100, nothing else."""
    loss_names = ("actor_loss",)

    def __init__(self, env, first_it: int):
        self.env, self.step_offset = env, first_it + 1

    def evaluated(self, k, trainer, step, returns, log):
        log({"d4rl_normalized_score": np.asarray(self.env.get_normalized_score(returns.mean())).mean() * 100})


def train(config: TrainConfig, dataset=None, env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None, seeds_per_gpu: int = 1,
          sampler: str = "device", device: Optional[str] = None, chunk: int = 2000):
    """dbc:313-416 on the HIP step and the device selection.

    ``dataset``: a D4RL transition dict (``observations``, ``actions``, ``next_observations``, ``rewards``,
    ``terminals``); None: ``d4rl.qlearning_dataset(env)``.  ``env``: a gym < 0.26 environment with
    ``get_normalized_score``; None: ``gym.make(config.env)`` (gym and d4rl are imported only then).  ``logger``,
    ``sampler``, ``device`` and ``chunk`` as in ``custom_offline.train``; ``device`` defaults to the rank's GPU,
    else ``config.device``.

    The two quirks of dbc's ``train()`` hold here too: the selection is always cut at 1000 rows
    (``config.max_traj_len`` is never passed on, dbc:322), and ``config.discount`` reaches ``BC`` where nothing
    reads it (it does decide the returns of the selection).

    ``seeds_per_gpu`` = K > 1: seed k is ``rank_seed(seed, K) + k`` with its own net (built right after
    ``torch.manual_seed(seed)``), its own ``np.random.RandomState(seed)`` index stream, its own evaluation seed,
    checkpoints under ``seed_<seed>/`` and a ``seed`` entry in its records; all K share the buffer and step as one
    ``BCGroup``.  Every seed is bit-identical to the run it is alone.  ``load_model`` is for one seed.
    Returns the trainer (K = 1) or the list of K trainers."""
    _offline_loop.check_sampler(sampler)
    seeds = _offline_loop.group_seeds(config.seed, seeds_per_gpu)
    K = len(seeds)
    if K > 1 and config.load_model != "":
        raise ValueError("load_model continues one run: seeds_per_gpu must be 1")
    device = _d4rl.default_device(config, device)
    env = _d4rl.default_env(config.env, env, dataset)
    dataset = _d4rl.default_dataset(env, dataset)
    state_dim = env.observation_space.shape[0]
    action_dim = env.action_space.shape[0]

    check_envelope(state_dim, action_dim)  # (before anything is uploaded: nothing is launched for a refused shape)

    replay_buffer, state_mean, state_std = _load_selected(config, dataset, state_dim, action_dim, device)
    env = wrap_env(env, state_mean=state_mean, state_std=state_std)

    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)
    max_action = float(env.action_space.high[0])
    set_seed(seeds[0], env)  # dbc:353-354
    print("---------------------------------------")
    print(f"Training BC, Env: {config.env}, Seed: {seeds[0] if K == 1 else seeds}")
    print("---------------------------------------")
    trainers = [_build_trainer(s, state_dim, action_dim, max_action, config.discount, device) for s in seeds]
    if config.load_model != "":
        trainers[0].load_state_dict(torch.load(Path(config.load_model)))
    gens, stream = _co._index_sources(seeds, sampler, device)
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    _offline_loop.run(
        trainers, seeds, lambda active: stepper(trainers), int(config.max_timesteps), int(config.eval_freq), chunk,
        logger, ckpt_dirs, _co._steps(stream, trainers, [replay_buffer] * K, gens, config.batch_size),
        lambda k, trainer, step: eval_actor(env, trainer.actor, device, config.n_episodes, seeds[k]),
        _Records(env, trainers[0].total_it))
    return trainers if K > 1 else trainers[0]


def main(argv=None):
    """``python -m iqlpref_amd.offline_bc --config_path file.yaml --field value ...`` (dbc:313 pyrallis.wrap)."""
    _d4rl.cli("iqlpref_amd.offline_bc", load_config, train, argv)


if __name__ == "__main__":
    main()
