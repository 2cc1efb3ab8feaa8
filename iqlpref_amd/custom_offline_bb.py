"""The ``algorithms/custom_offline/iql_bb.py`` flavour of the path (config
``configs/custom_offline/iql/bb.yaml``).  "bref:" = that file.

Differences from ``custom_offline`` (``iql.py``) and how they map onto the same kernels:

* batches are not drawn row by row: ``RandomBatchSampler`` (bref:208-238) draws ONE
  ``torch.randperm(N // B)`` when it is built, and every epoch of ``ceil(N / B)`` steps walks the
  same permutation -- batch i is the contiguous rows ``[perm[i] B, (perm[i] + 1) B)``, and the
  ``N % B`` rows left over are one SHORT batch at the end of each epoch (``drop_last=False``).
  ``BlockEpochSampler`` holds the permutation; ``iqlhip_block_epoch_indices`` writes the indices
  and the valid-row count of every step on the device, and ``iqlhip_train_steps_valid`` forms the
  batch means of a short step over its valid rows only (csrc/np_sampler.hip, csrc/iql_step.hip);
* the Q target is ``r + attn_mask * gamma * V(s')`` (bref:473): the buffer stores
  ``done = 1 - attn_mask``, exact for masks in {0, 1} (anything else is refused);
* states are z-scored on all columns but the last four, eps 1e-3 (bref:145-149), in float64 on the
  host as ``IQL_H5Dataset.__getitem__`` does, then rounded to float32 once;
* ``act()`` clamps per dimension to ``[min_actions, max_actions]`` without scaling (bref:344-350);
  the maximum speed is the 99th percentile of ``actions[:, 0]``, the angle range +-180;
* the Polyak form, no autocast, the cosine actor schedule and the checkpoint keys are those of
  ``custom_offline``, whose ``_build_trainer`` builds the trainer; the train / evaluate / checkpoint loop is
  ``_offline_loop.run``, as for the other custom flavours.

``bb_run_eval_IQL`` is the evaluation of bref:675-867: a numpy simulator of a point agent that steers
to a goal among drifting obstacles, rewarded by the preference model over a rolling context.  It makes
the same ``default_rng(seed)`` calls in the same order with the same float arithmetic, so that equal
actions give equal states and returns.
``_device_eval`` is the same evaluation with the step loop on the GPU (csrc/bb_sim.hip): the host draws the
set-up and the drift table, a rollout takes the episode to its end, and one ``window_values`` call per episode
gives the rewards.  Its rollouts: ``bb_run_eval_device`` (``train(eval_on="device")``) alternates the actor's
forward and one simulator step on one stream; ``bb_run_eval_fused`` (``train(eval_on="fused")``) runs the whole
step loop, the forward included, in ONE launch (``k_bb_episodes``), and ``bb_run_eval_fused_group`` the episodes
of K actors as K work-groups of that launch, with the bits of ``bb_run_eval_device``.

``train(seeds_per_gpu=K)`` steps K seeds side by side on one GPU as one ``SeedGroup``: each seed walks its
own block permutation (``BlockEpochSamplerGroup`` writes the K index arrays and the one shared count array
with one launch of ``iqlhip_block_epoch_indices_group``), and ``iqlhip_group_train_steps_valid`` forms the
short step of every member over its valid rows.  Every seed is bit-identical to ``train()`` of that seed
alone.

Not built: the Orbax reward-model reader (``load_PT``); HDF5 is read only when ``h5py`` is there.
Sweeps and bf16 are not offered for this flavour.
"""
import ctypes as C
import os
import time
import uuid
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _offline_loop
from . import custom_offline as _co
from . import distributed as D
from ._lib import check, ptr, stream_ptr
from .custom_offline import ImplicitQLearning as _CustomIQL
from .custom_offline import ReplayBuffer
from .iql import DeterministicPolicy as _DeterministicPolicy
from .iql import GaussianPolicy as _GaussianPolicy
from .iql import set_seed
from .multi import stepper
from .relabel import RewardPT

DATASET_KEYS = ("states", "actions", "rewards", "n_rewards", "next_states", "attn_mask")


@dataclass
class TrainConfig:
    """bref:43-81, same fields and defaults."""
    project: str = "IQL-pref"
    group: str = "IQL-BB"
    name: str = "iql"
    gamma: float = 0.99
    tau: float = 0.005
    beta: float = 3.0
    iql_tau: float = 0.7
    iql_deterministic: bool = False
    vf_lr: float = 3e-4
    qf_lr: float = 3e-4
    actor_lr: float = 3e-4
    actor_dropout: Optional[float] = None
    dataset_id: str = "bbway1"
    dataset_path: str = "~/iqlpref/t0012/reward_data_1/bbway1_t0012.hdf5"
    reward_model_path: str = "~/iqlpref/t0012/pt_rewards_1/best_model.ckpt"
    move_stats_path: str = "~/iqlpref/t0012/cache/p_stats.npy"
    update_steps: int = int(1e6)
    batch_size: int = 256
    normalize_state: bool = False
    normalize_reward: bool = False
    eval_every: int = int(5e3)
    eval_episodes: int = 10
    train_seed: int = 0
    eval_seed: int = 0
    checkpoints_path: Optional[str] = None

    def __post_init__(self):
        self.name = f"{self.name}-{self.dataset_id}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)


def load_stats(load_file):
    """bref:84-86."""
    return tuple(np.load(os.path.expanduser(load_file), fix_imports=False))


# --------------------------------------------------------------------------- #
# dataset (bref:120-205)
# --------------------------------------------------------------------------- #
def _h5py():
    try:
        import h5py
    except ImportError:
        raise ImportError("custom_offline_bb: reading a dataset from an HDF5 path needs h5py, which is not "
                          "installed; pass the arrays instead (a mapping with the keys "
                          f"{', '.join(DATASET_KEYS)})") from None
    return h5py


class BBDataset:
    """``IQL_H5Dataset`` (bref:120-205) over arrays held in memory.

    ``source``: a mapping with ``states`` [N, S], ``actions`` [N, A], ``rewards``, ``n_rewards`` [N] or
    [N, 1], ``next_states`` [N, S], ``attn_mask`` [N] or [N, 1], or the path of an HDF5 file with these
    datasets (needs h5py).  The statistics are the reference's numpy calls on the arrays as stored:
    the 99th percentile of ``actions[:, 0]``, and -- ``normalized_states`` -- mean and std + eps of every
    state column but the last four, which keep mean 0 and std 1."""

    def __init__(self, source, normalized_states: bool = True, normalized_rewards: bool = True,
                 reward_adjustment: float = 0.0, eps: float = 1e-3, device: str = "cpu"):
        if isinstance(source, (str, os.PathLike)):
            h5py = _h5py()
            with h5py.File(os.path.expanduser(os.fspath(source)), "r") as f:
                source = {k: f[k][...] for k in DATASET_KEYS}
        if not isinstance(source, Mapping):
            raise TypeError("BBDataset takes a mapping of arrays or an HDF5 path")
        missing = [k for k in DATASET_KEYS if k not in source]
        if missing:
            raise KeyError(f"BBDataset: missing arrays {missing}")
        self._data = {k: np.asarray(source[k]) for k in DATASET_KEYS}
        states, actions = self._data["states"], self._data["actions"]
        if states.ndim != 2 or actions.ndim != 2 or states.shape[1] < 5:
            raise ValueError("states must be [N, S] with S > 4 and actions [N, A]")
        n = states.shape[0]
        for k in DATASET_KEYS:
            if self._data[k].shape[0] != n:
                raise ValueError(f"BBDataset: {k} has {self._data[k].shape[0]} rows, states {n}")
        mask = self._data["attn_mask"]
        if not np.all((mask == 0) | (mask == 1)):
            raise ValueError("attn_mask must hold only 0 and 1: the buffer stores done = 1 - attn_mask, and the "
                             "target r + attn_mask * gamma * V(s') is reproduced exactly only for these")
        self.normalized_rewards = normalized_rewards
        self.reward_adjustment = reward_adjustment
        self._device = device
        self._sts_shape, self._acts_shape = states.shape, actions.shape
        self._max_speed = np.percentile(actions[:, 0], 99)
        self._min_speed, self._max_angle, self._min_angle = 0.0, 180.0, -180.0
        self._state_mean = np.zeros(states.shape[1])
        self._state_std = np.ones(states.shape[1])
        if normalized_states:
            self._state_mean[:-4] = states[:, :-4].mean(0)
            self._state_std[:-4] = states[:, :-4].std(0) + eps

    def __len__(self):
        return self._sts_shape[0]

    def shapes(self):
        return self._sts_shape, self._acts_shape

    def max_actions(self):
        return torch.tensor([self._max_speed, self._max_angle], device=self._device)

    def min_actions(self):
        return torch.tensor([self._min_speed, self._min_angle], device=self._device)

    def state_mean(self):
        return self._state_mean

    def state_std(self):
        return self._state_std

    def transitions(self) -> Dict[str, np.ndarray]:
        """All N transitions as ``__getitem__`` (bref:162-187) hands them out, float32, under the keys
        ``ReplayBuffer.load_dataset`` takes; ``terminals`` = 1 - attn_mask."""
        d = self._data
        f32 = lambda x: np.asarray(x).astype(np.float32)
        rewards = d["n_rewards"] if self.normalized_rewards else d["rewards"]
        n = len(self)
        return {"observations": f32((d["states"] - self._state_mean) / self._state_std),
                "actions": f32(d["actions"]),
                "rewards": f32(rewards + self.reward_adjustment).reshape(n),
                "next_observations": f32((d["next_states"] - self._state_mean) / self._state_std),
                "terminals": 1.0 - f32(d["attn_mask"]).reshape(n)}


# --------------------------------------------------------------------------- #
# block-shuffled epochs (bref:208-267)
# --------------------------------------------------------------------------- #
class BlockEpochSampler:
    """``fast_loader`` (bref:241-267): the ``n_rows // batch_size`` whole blocks in ONE permuted order,
    drawn at construction with ``torch.randperm`` on the CPU ``generator`` (None: torch's global one, as
    the reference) or handed in as ``perm``; then the ``n_rows % batch_size`` rows left over.  Step t of
    training uses slot ``t % len(self)``."""

    def __init__(self, n_rows: int, batch_size: int, generator: Optional[torch.Generator] = None, perm=None):
        self.n_rows, self.batch_size = int(n_rows), int(batch_size)
        if self.n_rows < 1 or self.batch_size < 1:
            raise ValueError("n_rows and batch_size must be >= 1")
        self.n_blocks = self.n_rows // self.batch_size
        self.tail = self.n_rows - self.n_blocks * self.batch_size
        if perm is None:
            perm = torch.randperm(self.n_blocks, generator=generator)
        perm = torch.as_tensor(np.asarray(perm)).to(torch.int64).cpu().reshape(-1)
        if perm.numel() != self.n_blocks or sorted(perm.tolist()) != list(range(self.n_blocks)):
            raise ValueError(f"perm must be a permutation of 0..{self.n_blocks - 1}")
        self.perm = perm
        self._dev_perm = None

    def __len__(self):
        """Steps per epoch: ceil(n_rows / batch_size)."""
        return self.n_blocks + (1 if self.tail else 0)

    def host_indices(self, t0: int, n_steps: int) -> Tuple[np.ndarray, np.ndarray]:
        """(int64 [n_steps, batch_size], int32 [n_steps]): the rows of steps t0 .. t0 + n_steps - 1 and how
        many of them count; the entries of a short batch beyond its count repeat the last row."""
        B, perm = self.batch_size, self.perm.numpy()
        idx = np.empty((n_steps, B), np.int64)
        valid = np.empty(n_steps, np.int32)
        j = np.arange(B, dtype=np.int64)
        for i in range(n_steps):
            slot = (t0 + i) % len(self)
            if slot < self.n_blocks:
                idx[i], valid[i] = perm[slot] * B + j, B
            else:
                idx[i], valid[i] = np.minimum(self.n_blocks * B + j, self.n_rows - 1), self.tail
        return idx, valid

    def device_indices(self, t0: int, n_steps: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """The same two arrays written on the device by one launch of ``iqlhip_block_epoch_indices`` on
        the current stream: nothing waits for the host."""
        lib = _lib.load()
        dev = _lib.require_gpu(device)
        if self._dev_perm is None or self._dev_perm.device != dev:
            self._dev_perm = self.perm.to(dev)
        idx = torch.empty((n_steps, self.batch_size), dtype=torch.int64, device=dev)
        valid = torch.empty(n_steps, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib.iqlhip_block_epoch_indices(ptr(self._dev_perm) if self.n_blocks else None, self.n_rows,
                                                 self.batch_size, int(t0), int(n_steps), ptr(idx), ptr(valid),
                                                 stream_ptr()))
        return idx, valid


class BlockEpochSamplerGroup:
    """The samplers of the K members of a seed group: 1..``MAX_GROUP`` ``BlockEpochSampler`` of equal
    ``n_rows`` and ``batch_size``, each with its own permutation.  All members walk epochs of the same
    length, so the short slot falls on the same step for all of them and one count array serves the group."""

    def __init__(self, samplers: Sequence[BlockEpochSampler]):
        self.samplers = list(samplers)
        if not 1 <= len(self.samplers) <= _lib.MAX_GROUP:
            raise ValueError(f"a sampler group holds 1..{_lib.MAX_GROUP} samplers (got {len(self.samplers)})")
        self.n_rows, self.batch_size = self.samplers[0].n_rows, self.samplers[0].batch_size
        for k, sm in enumerate(self.samplers):
            if (sm.n_rows, sm.batch_size) != (self.n_rows, self.batch_size):
                raise ValueError(f"sampler {k} walks {sm.n_rows} rows in batches of {sm.batch_size}, sampler 0 "
                                 f"{self.n_rows} in batches of {self.batch_size}: a group shares one epoch shape")
        self._dev_perms = None

    @classmethod
    def draw(cls, n_rows: int, batch_size: int, n_members: int, perm=None) -> "BlockEpochSamplerGroup":
        """``perm=None``: ``n_members`` permutations drawn in member order from torch's global generator
        (what as many reference processes would each draw when they build their loader); else a sequence of
        ``n_members`` permutations."""
        K = int(n_members)
        if perm is None:
            return cls([BlockEpochSampler(n_rows, batch_size) for _ in range(K)])
        perms = list(perm)
        if len(perms) != K or any(np.ndim(p) != 1 for p in perms):
            raise ValueError(f"perm must be a sequence of {K} block permutations, one per seed")
        return cls([BlockEpochSampler(n_rows, batch_size, perm=p) for p in perms])

    def __len__(self):
        return len(self.samplers)

    def device_indices(self, t0: int, n_steps: int, device) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """(K int64 [n_steps, batch_size] tensors, one int32 [n_steps] count tensor): what
        ``BlockEpochSampler.device_indices`` gives for every member, from ONE launch of
        ``iqlhip_block_epoch_indices_group`` on the current stream (one member: from its own launch)."""
        lib = _lib.load()
        dev = _lib.require_gpu(device)
        K = len(self.samplers)
        if K == 1:  # (the one-sampler launch)
            idx, valid = self.samplers[0].device_indices(t0, n_steps, device)
            return [idx], valid
        if self._dev_perms is None or self._dev_perms.device != dev:
            self._dev_perms = torch.stack([sm.perm for sm in self.samplers]).to(dev)  # [K, n_blocks]
        area = torch.empty((K, n_steps, self.batch_size), dtype=torch.int64, device=dev)
        valid = torch.empty(n_steps, dtype=torch.int32, device=dev)
        whole = self.samplers[0].n_blocks > 0
        perms = (C.c_void_p * K)(*[self._dev_perms[k].data_ptr() if whole else None for k in range(K)])
        outs = (C.c_void_p * K)(*[area[k].data_ptr() for k in range(K)])
        with torch.cuda.device(dev):
            check(lib.iqlhip_block_epoch_indices_group(perms, self.n_rows, self.batch_size, int(t0), int(n_steps),
                                                       outs, ptr(valid), K, stream_ptr()))
        return [area[k] for k in range(K)], valid


# --------------------------------------------------------------------------- #
# policies and trainer (bref:318-552)
# --------------------------------------------------------------------------- #
def _clamped_act(policy, action: torch.Tensor) -> np.ndarray:
    lo = torch.as_tensor(policy.min_actions, device=action.device)
    hi = torch.as_tensor(policy.max_actions, device=action.device)
    return torch.clamp(action, lo, hi).cpu().data.numpy().flatten()


class GaussianPolicy(_GaussianPolicy):
    """bref:318-350: no action scaling; ``act`` clamps to [min_actions, max_actions] per dimension."""

    def __init__(self, state_dim: int, act_dim: int, max_actions: torch.Tensor, min_actions: torch.Tensor,
                 hidden_dim: int = 256, n_hidden: int = 2, dropout: Optional[float] = None):
        super().__init__(state_dim, act_dim, 1.0, hidden_dim, n_hidden, dropout)
        self.max_actions, self.min_actions = max_actions, min_actions

    @torch.inference_mode()
    def act(self, state: np.ndarray, device: str = "cpu"):
        state = torch.tensor(state.reshape(1, -1), device=device, dtype=torch.float32)
        dist = self(state)
        return _clamped_act(self, dist.mean if not self.training else dist.sample())


class DeterministicPolicy(_DeterministicPolicy):
    """bref:353-384."""

    def __init__(self, state_dim: int, act_dim: int, max_actions: torch.Tensor, min_actions: torch.Tensor,
                 hidden_dim: int = 256, n_hidden: int = 2, dropout: Optional[float] = None):
        super().__init__(state_dim, act_dim, 1.0, hidden_dim, n_hidden, dropout)
        self.max_actions, self.min_actions = max_actions, min_actions

    @torch.inference_mode()
    def act(self, state: np.ndarray, device: str = "cpu"):
        state = torch.tensor(state.reshape(1, -1), device=device, dtype=torch.float32)
        return _clamped_act(self, self(state))


class ImplicitQLearning(_CustomIQL):
    """bref:416-552 on the fused step: the constructor of the reference, the arithmetic of
    ``custom_offline.ImplicitQLearning`` (the attn_mask of bref:473 lives in the buffer as 1 - done)."""

    def __init__(self, max_actions, min_actions, actor, actor_optimizer, actor_lr_scheduler, q_network, q_optimizer,
                 v_network, v_optimizer, iql_tau: float = 0.7, beta: float = 3.0, gamma: float = 0.99,
                 tau: float = 0.005, device: str = "cpu", *, seed: Optional[int] = None, keep_grads: bool = False):
        super().__init__(1.0, actor, actor_optimizer, actor_lr_scheduler, q_network, q_optimizer, v_network,
                         v_optimizer, iql_tau=iql_tau, beta=beta, gamma=gamma, tau=tau, device=device, seed=seed,
                         keep_grads=keep_grads)
        self.max_actions, self.min_actions = max_actions, min_actions

    def train_epoch_steps(self, replay_buffer: ReplayBuffer, sampler: BlockEpochSampler, t0: int, n_steps: int, *,
                          graph_unroll: Optional[int] = None):
        """Steps t0 .. t0 + n_steps - 1 of the epoch walk (bref:966-970) in one library call: the indices
        and valid-row counts come from the device generator, nothing waits for the host.  Returns the
        [n_steps, 3] device loss tensor."""
        if sampler.n_rows != replay_buffer.index_bound():
            raise ValueError(f"the sampler walks {sampler.n_rows} rows, the buffer holds {replay_buffer.index_bound()}")
        idx, valid = sampler.device_indices(t0, n_steps, self._dev)
        return self.train_steps(replay_buffer, n_steps, sampler.batch_size, indices=idx, n_valid=valid,
                                graph_unroll=graph_unroll)


# --------------------------------------------------------------------------- #
# evaluation (bref:577-867): the simulator
# --------------------------------------------------------------------------- #
_RAD = np.pi / 180.0
ARENA_RADIUS = 50.0
AGENT_RADIUS, GOAL_RADIUS = 0.3, 1.0
STATE_TAIL = 4  # level, ai, attempt, day: the columns the normalisation leaves alone


def _cos_deg(deg):
    c = np.cos(deg * _RAD)
    c = np.where(np.isclose(deg, 90), 0.0, c)
    return np.where(np.isclose(deg, 270), 0.0, c) * 1


def _sin_deg(deg):
    s = np.sin(deg * _RAD)
    s = np.where(np.isclose(deg, 360), 0.0, s)
    return np.where(np.isclose(deg, 180), 0.0, s) * 1


def _disc_point(radius, n, rng):
    """Uniform in a disc: the radius draw(s) first, then the angle draw(s)."""
    rad = radius * np.sqrt(rng.random(n))
    ang = rng.random(n) * 2 * np.pi
    return rad * np.cos(ang), rad * np.sin(ang)


def _segment_hits_goal(ax, ay, bx, by, gx, gy):
    """Does the agent (radius 0.3) moving from a to b touch the goal disc (radius 1)?  The point of the
    segment closest to the goal is tested; all scalars."""
    px, py, dx, dy = gx - ax, gy - ay, bx - ax, by - ay
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.asarray(px * dx + py * dy) / np.asarray((dx ** 2) + (dy ** 2))
    u = np.where(np.isnan(u), 0.0, u)
    u = np.where(u < 0, 0.0, u)
    u = np.where(u > 1, 1.0, u)
    cx, cy = ax + dx * u, ay + dy * u
    d2 = ((cx - gx) ** 2) + ((cy - gy) ** 2)
    lim = (AGENT_RADIUS + GOAL_RADIUS) ** 2
    return bool(np.any((d2 < lim) | np.isclose(d2, lim)))


def _observe(goal, px, py, ox, oy, oang, tail, n_near):
    """[x, y, (x, y, heading) of the n_near nearest obstacles, goal x, y, level, ai, attempt, day]."""
    dist = np.sqrt(((ox - px) ** 2) + ((oy - py) ** 2)) * 1
    near = np.argpartition(dist, np.arange(n_near))[:n_near]
    s = [px, py]
    for k in near:
        s += [ox[k], oy[k], oang[k]]
    s += [goal[0], goal[1]]
    s += [v * 1.0 for v in tail]
    return np.asarray(s)


def _episode_setup(rng, days):
    """The draws that open an episode (bref:690-741), in the reference's order: level, ai, attempt, day,
    the obstacles' disc points and headings, a start more than 1 away from obstacle 0, a goal about 30
    away inside the arena.  Returns (n_obs, ox, oy, oang, px, py, goal, tail)."""
    level = rng.choice([9, 10, 11])
    n_obs = {9: 50, 10: 100}.get(int(level), 150)
    ai = rng.choice([1, 2, 3, 4])
    attempt = rng.choice(4)
    day = rng.choice(days)
    ox, oy = _disc_point(ARENA_RADIUS, n_obs, rng)
    oang = rng.uniform(0.0, 360.0, n_obs)
    while True:  # a start more than 1 away from obstacle 0
        sx, sy = _disc_point(ARENA_RADIUS, None, rng)
        if np.all(((sx - ox[0]) ** 2) + ((sy - oy[0]) ** 2) > 1):
            break
    px, py = float(sx), float(sy)
    while True:  # a goal about 30 away, inside the arena
        heading = rng.uniform(0.0, 360.0)
        reach = rng.normal(30)
        goal = (float(px + reach * _cos_deg(heading)), float(py + reach * _sin_deg(heading)))
        if ((goal[0] ** 2) + (goal[1] ** 2)) <= ARENA_RADIUS ** 2:
            break
    return n_obs, ox, oy, oang, px, py, goal, (level, ai, attempt, day)


def bb_run_eval_IQL(actor, num_episodes, r_model, move_stats, state_mean=0, state_std=1, max_horizon=500,
                    n_min_obstacles=6, days=181, context_length=100, seed=4, device="cpu"):
    """bref:675-867.  ``num_episodes`` episodes of a point agent in a disc of radius 50: 50 / 100 / 150
    obstacles (level 9 / 10 / 11) drift along their headings by ``normal(move_stats[2], move_stats[3])``
    per step and re-enter mirrored when they leave; the agent moves by (speed, heading) =
    ``actor.act(normalised state)``; the episode ends when its path touches the goal or after
    ``max_horizon`` steps.  The reward of a step is ``r_model(states, actions, timesteps, mask,
    training=False)[0]["value"][:, 0, -1]`` over the last ``context_length`` steps; the return is their
    sum.  Obstacles do not stop the agent (the reference computes those collisions and drops them).
    Every draw comes from ``np.random.default_rng(seed)`` in the reference's order.  The actor is handed
    back in train mode."""
    actor.eval()
    returns = []
    rng = np.random.default_rng(seed)
    for _ in range(num_episodes):
        n_obs, ox, oy, oang, px, py, goal, tail = _episode_setup(rng, days)
        s = _observe(goal, px, py, ox, oy, oang, tail, n_min_obstacles).reshape(1, 1, -1)
        a = np.zeros((1, 0, 2))
        t = np.zeros((1, 1), dtype=np.int32)
        episode_return = 0.0
        for _ in range(max_horizon):
            action = actor.act((s[-1, -1] - state_mean) / state_std, device)
            a = np.concatenate([a, action.reshape(1, 1, -1)], axis=1)[:, -context_length:, :]
            reward, _ = r_model(s, a, t, np.ones((1, t.shape[1]), dtype=np.float32), training=False)
            reward = reward["value"][:, 0, -1]
            qx, qy = px, py
            px = float(px + (action[0] * _cos_deg(action[1])))
            py = float(py + (action[0] * _sin_deg(action[1])))
            drift = rng.normal(move_stats[2], move_stats[3], n_obs)
            nx, ny = ox + (drift * _cos_deg(oang)), oy + (drift * _sin_deg(oang))
            out = np.sqrt((nx ** 2) + (ny ** 2)) > ARENA_RADIUS
            ox, oy = np.where(out, -ox, nx), np.where(out, -oy, ny)
            reached = _segment_hits_goal(qx, qy, px, py, goal[0], goal[1])
            s = np.concatenate([s, _observe(goal, px, py, ox, oy, oang, tail, n_min_obstacles).reshape(1, 1, -1)],
                               axis=1)[:, -context_length:, :]
            t = np.concatenate([t, (t[-1][-1] + 1).reshape(1, -1)], axis=1)[:, -context_length:]
            episode_return += reward
            if reached:
                break
        returns.append(episode_return)
    actor.train()
    return np.asarray(returns)


class RewardPTContext:
    """A ``RewardPT`` behind the call shape of the reference's reward model (bref:786-793):
    ``r(states [1, L, S], actions [1, L, A], timesteps [1, L], mask, training=False)`` ->
    ``({"value": [1, 1, 1]}, None)``, the value of the LAST token of the context -- the one entry
    ``bb_run_eval_IQL`` reads -- from one ``window_values`` call with the true timesteps."""

    def __init__(self, model: RewardPT, context_length: int = 100):
        if not isinstance(model, RewardPT):
            raise TypeError("RewardPTContext wraps an iqlpref_amd RewardPT")
        self.model, self.context_length = model, int(context_length)

    def __call__(self, states, actions, timesteps, attn_mask=None, training=False):
        dev = next(self.model.parameters()).device
        L = states.shape[1]
        if actions.shape[1] != L or timesteps.shape[1] != L or L > self.context_length:
            raise ValueError("states, actions and timesteps must share one length <= context_length")
        up = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(dev)
        v = self.model.window_values(up(states[0], torch.float32), up(actions[0], torch.float32),
                                     up([0], torch.int64), up([L], torch.int32), self.context_length,
                                     win_t0=up([int(timesteps[0, 0])], torch.int32))
        return {"value": v.cpu().numpy().astype(np.float64).reshape(1, 1, 1)}, None


# --------------------------------------------------------------------------- #
# the device state of the same evaluation and the launches that advance it (csrc/bb_sim.hip)
# --------------------------------------------------------------------------- #
class DeviceEpisode:
    """The device state of one simulated episode and the launches that advance it: ``load`` uploads a
    set-up and its drift table, ``reset`` writes observation row 0, ``step`` is one ``iqlhip_bb_sim_step``
    and ``rollout`` n times (actor forward, step) in one library call; ``poll`` is the one place that waits
    for the device.  The buffers are allocated once and serve every episode of an evaluation.

    ``injected``: an fp32 [max_horizon, 2] table of raw actor outputs that step t reads in place of the
    forward's output row (tests)."""

    def __init__(self, n_near: int, max_horizon: int, state_mean, state_std, min_actions, max_actions, device,
                 n_obs_max: int = 150, injected=None):
        self.lib = _lib.load()
        self.dev = _lib.require_gpu(device)
        self.n_near, self.H = int(n_near), int(max_horizon)
        self.S, self.A = 2 + 3 * self.n_near + 2 + STATE_TAIL, 2
        S, H, dev = self.S, self.H, self.dev
        f64 = lambda x: torch.from_numpy(np.array(np.broadcast_to(np.asarray(x, np.float64), (S,)))).to(dev)
        lim = lambda x: torch.as_tensor(x).detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        self.mean, self.std = f64(state_mean), f64(state_std)
        self.lo, self.hi = lim(min_actions), lim(max_actions)
        if self.lo.numel() != 2 or self.hi.numel() != 2:
            raise ValueError("min_actions and max_actions hold (speed, heading)")
        self.n_obs_max = int(n_obs_max)
        self.state = torch.zeros(8 + 3 * self.n_obs_max, dtype=torch.float64, device=dev)
        self.drift = torch.zeros(H * self.n_obs_max, dtype=torch.float64, device=dev)
        self.ctl = torch.zeros(2, dtype=torch.int32, device=dev)
        self.obs_hist = torch.zeros((H + 1, S), dtype=torch.float32, device=dev)
        self.act_hist = torch.zeros((H, 2), dtype=torch.float32, device=dev)
        self.record = torch.zeros((H + 1, S), dtype=torch.float64, device=dev)
        self.actor_in = torch.zeros(S, dtype=torch.float32, device=dev)
        self.actor_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.injected = None
        if injected is not None:
            self.injected = torch.as_tensor(np.ascontiguousarray(injected, dtype=np.float32)).to(dev)
            if self.injected.shape != (self.H, 2):
                raise ValueError(f"injected actions must be [{self.H}, 2]")
        self.n_obs = 0
        self.sim = None

    def _struct(self, n_obs: int) -> "_lib.BbSim":
        b = _lib.BbSim()
        b.n_obs, b.n_near, b.state_dim, b.action_dim, b.max_horizon = n_obs, self.n_near, self.S, self.A, self.H
        b.actor_out_stride = 0 if self.injected is None else 2
        out = self.actor_out if self.injected is None else self.injected
        for name, t in (("state", self.state), ("drift", self.drift), ("ctl", self.ctl), ("obs_hist", self.obs_hist),
                        ("act_hist", self.act_hist), ("record", self.record), ("actor_in", self.actor_in),
                        ("actor_out", out), ("state_mean", self.mean), ("state_std", self.std),
                        ("min_actions", self.lo), ("max_actions", self.hi)):
            setattr(b, name, t.data_ptr())
        return b

    def load(self, ox, oy, oang, px, py, goal, tail, drift):
        """One upload of the set-up and one of the [max_horizon, n_obs] drift table, on the current stream."""
        n_obs = int(len(ox))
        if n_obs > self.n_obs_max:
            raise ValueError(f"{n_obs} obstacles, the buffers hold {self.n_obs_max}")
        drift = np.ascontiguousarray(drift, dtype=np.float64)
        if drift.shape != (self.H, n_obs):
            raise ValueError(f"the drift table must be [{self.H}, {n_obs}]")
        host = np.concatenate([[px, py, goal[0], goal[1]], [float(v) for v in tail], ox, oy, oang]).astype(np.float64)
        self.state[:host.size].copy_(torch.from_numpy(host), non_blocking=False)
        self.drift[:drift.size].copy_(torch.from_numpy(drift.reshape(-1)), non_blocking=False)
        self.n_obs, self.sim = n_obs, self._struct(n_obs)

    def reset(self):
        with torch.cuda.device(self.dev):
            check(self.lib.iqlhip_bb_sim_reset(C.byref(self.sim), stream_ptr()))

    def step(self):
        with torch.cuda.device(self.dev):
            check(self.lib.iqlhip_bb_sim_step(C.byref(self.sim), stream_ptr()))

    def rollout(self, actor_desc, n_steps: int):
        with torch.cuda.device(self.dev):
            check(self.lib.iqlhip_bb_sim_rollout(C.byref(self.sim), C.byref(actor_desc), int(n_steps), stream_ptr()))

    def poll(self) -> Tuple[int, bool]:
        """(steps taken, done): waits for everything queued."""
        t, done = self.ctl.cpu().tolist()
        return int(t), bool(done)


def _actor_desc(actor):
    """The ``iqlhip_mlp_desc`` of a policy's net on its live fp32 weights, eval mode (no dropout), and
    the tensors it points into."""
    net = getattr(actor, "net", None)
    if not isinstance(actor, (GaussianPolicy, DeterministicPolicy)) or not hasattr(net, "linears"):
        raise TypeError("bb_run_eval_device rolls out a custom_offline_bb GaussianPolicy or DeterministicPolicy; "
                        "bb_run_eval_IQL takes any object with act()")
    d = _lib.MlpDesc()
    lin = net.linears()
    d.n_layers = len(lin)
    keep = []
    for i, l in enumerate(lin):
        w = l.weight.detach().to(torch.float32).contiguous()
        b = l.bias.detach().to(torch.float32).contiguous()
        keep += [w, b]
        d.dims[i], d.dims[i + 1] = w.shape[1], w.shape[0]
        d.weights[i], d.biases[i] = w.data_ptr(), b.data_ptr()
    d.w_in_out, d.hidden_act, d.out_act = 0, net._hidden_act, net._out_act
    return d, keep


def _rewind_drift(rng, saved_state, move_stats, length: int, n_obs: int):
    """Leave ``rng`` where ``length`` per-step draws of ``n_obs`` normals from ``saved_state`` leave it."""
    rng.bit_generator.state = saved_state
    if length:
        rng.normal(move_stats[2], move_stats[3], (length, n_obs))


# --------------------------------------------------------------------------- #
# K episodes as the work-groups of one launch (k_bb_episodes)
# --------------------------------------------------------------------------- #
class FusedEpisodes:
    """K ``DeviceEpisode`` buffer sets run as the K work-groups of one ``iqlhip_bb_sim_episodes`` call.  Their
    control words are the rows of ONE [K, 2] tensor, so that ``poll`` is one device-to-host copy; the scratch of
    the call (argument blocks and weight images) is allocated once and grows only when an actor does."""

    def __init__(self, episodes: Sequence[DeviceEpisode]):
        self.episodes = list(episodes)
        K = len(self.episodes)
        if not 1 <= K <= _lib.MAX_GROUP:
            raise ValueError(f"1..{_lib.MAX_GROUP} episodes run side by side, got {K}")
        self.lib, self.dev = self.episodes[0].lib, self.episodes[0].dev
        if any(ep.dev != self.dev for ep in self.episodes):
            raise ValueError("the episodes of one launch live on one device")
        self.ctl = torch.zeros((K, 2), dtype=torch.int32, device=self.dev)
        for k, ep in enumerate(self.episodes):
            ep.ctl = self.ctl[k]  # (load() builds the struct from it)
        self.scratch = None

    def run(self, actor_descs: Sequence[Optional["_lib.MlpDesc"]]):
        """Queue every loaded episode from its reset to its end; ``actor_descs[k]`` may be None for an episode
        with an injected table."""
        K = len(self.episodes)
        if len(actor_descs) != K:
            raise ValueError(f"{K} episodes, {len(actor_descs)} actors")
        sims = (_lib.BbSim * K)(*[ep.sim for ep in self.episodes])
        actors = (C.POINTER(_lib.MlpDesc) * K)(*[C.pointer(d) if d is not None else C.POINTER(_lib.MlpDesc)()
                                                 for d in actor_descs])
        need = C.c_size_t(0)
        check(self.lib.iqlhip_bb_sim_episodes_scratch_bytes(actors, K, C.byref(need)))
        if self.scratch is None or self.scratch.numel() < need.value:
            self.scratch = torch.empty(need.value, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            check(self.lib.iqlhip_bb_sim_episodes(sims, actors, K, ptr(self.scratch), self.scratch.numel(),
                                                  stream_ptr()))

    def poll(self) -> List[Tuple[int, bool]]:
        """[(length, done)] of the K episodes: waits for everything queued, one copy."""
        return [(int(t), bool(d)) for t, d in self.ctl.cpu().tolist()]


def _fused_actor_descs(actors):
    """The descriptors of ``actors`` after the library has checked them against the fused forward's envelope
    (widths <= 256, relu / tanh, eval mode) -- a host-side check, nothing is launched."""
    pairs = [_actor_desc(a) for a in actors]
    K = len(pairs)
    arr = (C.POINTER(_lib.MlpDesc) * K)(*[C.pointer(d) for d, _ in pairs])
    need = C.c_size_t(0)
    check(_lib.load().iqlhip_bb_sim_episodes_scratch_bytes(arr, K, C.byref(need)))
    return pairs


# --------------------------------------------------------------------------- #
# the device evaluations: one procedure, two rollouts
# --------------------------------------------------------------------------- #
def _launch_pair_rollout(eps, chunk: int):
    """A reset launch, then ``chunk`` (forward, step) pairs per library call and one host wait per chunk, until the
    episode is done or ``max_horizon`` steps are queued."""
    ep, = eps

    def run(descs):
        ep.reset()
        queued, length, done = 0, 0, False
        while queued < ep.H and not done:
            n = min(chunk, ep.H - queued)
            ep.rollout(descs[0], n)
            queued += n
            length, done = ep.poll()
        return [length]
    return run


def _fused_rollout(eps):
    """One library call and one copy of the [K, 2] control words per episode index, whatever K is."""
    fused = FusedEpisodes(eps)

    def run(descs):
        fused.run(descs)
        return [length for length, _ in fused.poll()]
    return run


def _device_eval(caller, describe, rollout, actors, seeds, num_episodes, r_model, move_stats, state_mean, state_std,
                 max_horizon, n_min_obstacles, days, context_length, device, records, record):
    """``bb_run_eval_IQL`` for K actors, ``actors[k]`` on ``default_rng(seeds[k])``, in lock step over the episode
    index with the step loop on the device; returns the K float64 [num_episodes, 1] arrays of returns.

    Per episode every member draws its set-up and the whole [max_horizon, n_obs] drift table from its own generator
    and uploads them; the rollout runs; every generator is put where the numpy loop leaves it (the saved state plus
    ``length`` rows of drift).  All rewards of an episode come from ONE ``RewardPT.window_values`` call over the
    device histories: window t covers steps ``max(0, t + 1 - context_length) .. t`` with their true timesteps, what
    the numpy loop hands to ``RewardPTContext`` step by step; the return is their float64 sum in step order.

    ``describe(actors)``: the K (descriptor, tensors) pairs, past the rollout's envelope check.  ``rollout(eps)``,
    called with the K ``DeviceEpisode`` before any is loaded: the ``run(descs)`` that takes the loaded episodes from
    their reset to their ends and returns the K lengths.  ``records[k]``: None or the dict for member k's
    ``episodes``; ``record``: the caller's, for its ``timing`` dict."""
    timing = record.get("timing") if isinstance(record, dict) else None
    if isinstance(r_model, RewardPT):
        r_model = RewardPTContext(r_model, context_length)
    if not isinstance(r_model, RewardPTContext):
        raise TypeError(f"{caller} takes a RewardPTContext or a RewardPT: its rewards are one window_values "
                        "call over device histories; bb_run_eval_IQL is the path for any other callable")
    H, cl, K = int(max_horizon), int(context_length), len(actors)
    if H < 1:
        raise ValueError("max_horizon must be >= 1")
    if min(H, cl) > r_model.context_length:
        raise ValueError("states, actions and timesteps must share one length <= context_length")
    if len(seeds) != K:
        raise ValueError(f"{K} actors, {len(seeds)} seeds")
    pairs = describe(actors)
    descs = [d for d, _ in pairs]
    pt_dev = next(r_model.model.parameters()).device
    for a in actors:
        a.eval()
    rngs = [np.random.default_rng(s) for s in seeds]
    eps = [DeviceEpisode(n_min_obstacles, H, state_mean, state_std, a.min_actions, a.max_actions, device)
           for a in actors]
    run = rollout(eps)
    steps = np.arange(H)
    starts = np.maximum(0, steps + 1 - cl)
    win_start = torch.from_numpy(starts.astype(np.int64)).to(pt_dev)
    win_len = torch.from_numpy((steps + 1 - starts).astype(np.int32)).to(pt_dev)
    win_t0 = torch.from_numpy(starts.astype(np.int32)).to(pt_dev)
    returns = [[] for _ in range(K)]

    def mark(phase, t0):
        if timing is None:
            return t0
        torch.cuda.synchronize(eps[0].dev)
        now = time.perf_counter()
        timing[phase] = timing.get(phase, 0.0) + (now - t0 if t0 is not None else 0.0)
        return now

    for _ in range(num_episodes):
        t0 = mark("other", None)
        drawn = []
        for rng, ep in zip(rngs, eps):
            n_obs, ox, oy, oang, px, py, goal, tail = _episode_setup(rng, days)
            saved = rng.bit_generator.state
            drift = rng.normal(move_stats[2], move_stats[3], (H, n_obs))
            ep.load(ox, oy, oang, px, py, goal, tail, drift)
            drawn.append((saved, n_obs))
        t0 = mark("setup", t0)
        lengths = run(descs)
        for rng, (saved, n_obs), length in zip(rngs, drawn, lengths):
            _rewind_drift(rng, saved, move_stats, length, n_obs)
        t0 = mark("steps", t0)
        for k, (ep, length) in enumerate(zip(eps, lengths)):
            values = np.zeros(0)
            if length:
                v = r_model.model.window_values(ep.obs_hist.to(pt_dev), ep.act_hist.to(pt_dev), win_start[:length],
                                                win_len[:length], r_model.context_length, win_t0=win_t0[:length])
                values = v.cpu().numpy().astype(np.float64)
            episode_return = np.zeros(1)
            for x in values:  # (0.0 + r_0 + r_1 + ..., the order of the numpy loop)
                episode_return = episode_return + x
            returns[k].append(episode_return)
            if isinstance(records[k], dict):
                records[k].setdefault("episodes", []).append(
                    {"states": ep.record[:length + 1].cpu().numpy(), "actions": ep.act_hist[:length].cpu().numpy(),
                     "rewards": values, "length": length})
        t0 = mark("reward", t0)
    for a in actors:
        a.train()
    return [np.asarray(r) for r in returns]


def bb_run_eval_device(actor, num_episodes, r_model, move_stats, state_mean=0, state_std=1, max_horizon=500,
                       n_min_obstacles=6, days=181, context_length=100, seed=4, device="cuda:0", chunk=64,
                       record=None):
    """``bb_run_eval_IQL`` with the step loop on the device: the same episodes, the same generator calls,
    the same float arithmetic, the same float64 array of returns (``_device_eval`` is the procedure).

    Per step the host queues the actor's forward (``iqlhip_mlp_forward`` on the live weights, the kernel
    ``actor.act`` reaches) and one ``k_bb_step``, ``chunk`` steps per library call, and reads the done flag once
    per chunk -- the only waits of the rollout.  Steps queued behind the goal write nothing.

    ``r_model``: a ``RewardPTContext`` or a ``RewardPT`` (wrapped with ``context_length``).  ``record``: a
    dict that receives ``record["episodes"]``, per episode ``states`` (float64 [length + 1, S], every
    observation), ``actions`` (float32 [length, 2]), ``rewards`` (float64 [length]) and ``length``; a
    ``record["timing"]`` dict, when present, receives the seconds spent in set-up and upload (``setup``),
    the step loop (``steps``) and the reward call (``reward``), each closed by a device synchronisation.  The
    actor is handed back in train mode."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    return _device_eval("bb_run_eval_device", lambda actors: [_actor_desc(a) for a in actors],
                        lambda eps: _launch_pair_rollout(eps, chunk), [actor], [seed], num_episodes, r_model,
                        move_stats, state_mean, state_std, max_horizon, n_min_obstacles, days, context_length,
                        device, [record], record)[0]


def bb_run_eval_fused(actor, num_episodes, r_model, move_stats, state_mean=0, state_std=1, max_horizon=500,
                      n_min_obstacles=6, days=181, context_length=100, seed=4, device="cuda:0", record=None):
    """``bb_run_eval_device`` with ONE launch per episode: the contract, the arguments (but ``chunk``), the
    ``record`` entries and the ``record["timing"]`` phases of that function, and its bits -- returns, states,
    actions, lengths and the generator's final state.

    Per episode: one set-up draw, one drift table, one upload, one ``iqlhip_bb_sim_episodes`` call (the weights
    are repacked once, then ``k_bb_episodes`` runs reset, forwards and steps to the end of the episode in one
    work-group), one host wait, one ``window_values`` call.  The fused forward takes actors of widths <= 256 with
    relu or tanh hidden layers; others are refused (``NotImplementedError``) before anything is launched, and
    ``bb_run_eval_device`` takes them."""
    return _device_eval("bb_run_eval_fused", _fused_actor_descs, _fused_rollout, [actor], [seed], num_episodes,
                        r_model, move_stats, state_mean, state_std, max_horizon, n_min_obstacles, days,
                        context_length, device, [record], record)[0]


def bb_run_eval_fused_group(actors, num_episodes, r_model, move_stats, state_mean=0, state_std=1, max_horizon=500,
                            n_min_obstacles=6, days=181, context_length=100, seeds=(4,), device="cuda:0",
                            record=None):
    """K evaluations side by side: ``actors[k]`` on ``default_rng(seeds[k])``.  Returns the list of the K return
    arrays, each bit-equal to ``bb_run_eval_fused`` of that member alone.

    The members run in lock step over the episode index (``_device_eval``): for episode e ONE library call runs the
    K episodes as K work-groups of one launch, ONE copy reads the K (length, done) pairs, every generator is rewound
    by its own member's length.  A member whose episode ends early leaves its generator elsewhere than the others,
    so the later set-ups differ between members -- as in K separate evaluations.

    ``record``: a dict that receives ``record["members"]``, K dicts with the ``episodes`` list of
    ``bb_run_eval_fused``, and whose ``record["timing"]``, when present, receives the phases of all members."""
    actors, seeds = list(actors), list(seeds)
    members = [{} if isinstance(record, dict) else None for _ in actors]
    if isinstance(record, dict):
        record["members"] = members
    return _device_eval("bb_run_eval_fused_group", _fused_actor_descs, _fused_rollout, actors, seeds, num_episodes,
                        r_model, move_stats, state_mean, state_std, max_horizon, n_min_obstacles, days,
                        context_length, device, members, record)


# --------------------------------------------------------------------------- #
# train (bref:870-1027)
# --------------------------------------------------------------------------- #
group_seeds = _offline_loop.group_seeds


def train(config: TrainConfig, dataset=None, reward_model=None, move_stats=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None, perm=None, seeds_per_gpu: int = 1,
          device: Optional[str] = None, chunk: int = 2000, eval_on: str = "host"):
    """bref:870-1027 on the fused HIP step.

    ``dataset``: a ``BBDataset``, a mapping of arrays or an HDF5 path (None: ``config.dataset_path``);
    mappings and paths are wrapped with ``config.normalize_state`` / ``normalize_reward`` as bref:892-897.
    ``reward_model``: a callable with the reference's call shape (``RewardPTContext``); the Orbax checkpoint
    at ``reward_model_path`` cannot be read here.  ``move_stats``: the four movement statistics (None:
    ``load_stats(config.move_stats_path)``).  ``logger(record, step)``: one call per ``wandb.log`` of bref
    (default: wandb when importable, else print).  ``perm``: the block permutation (None: drawn with
    ``torch.randperm`` on torch's global generator BEFORE the training seed is set, where the reference
    builds its loader).  There is no ``resume`` for this flavour for that reason: the permutations of a second
    start would be others (``_offline_loop.run(resume=...)`` is not passed).

    The steps are queued in chunks of at most ``chunk`` that end on evaluation boundaries; the indices of
    a chunk are written on the device, and its losses come back to the host once, after the next chunk has
    been queued.  Returns the trainer.

    ``eval_on``: "host" evaluates with ``bb_run_eval_IQL`` (the numpy simulator, any reward callable),
    "device" with ``bb_run_eval_device`` (the step loop on the GPU; ``reward_model`` must then be a
    ``RewardPTContext`` or a ``RewardPT``, which is checked before the first step), "fused" with
    ``bb_run_eval_fused`` (one launch per episode; the same bits as "device"; the reward model as for "device",
    actors of widths <= 256, both checked before the first step).  With ``seeds_per_gpu`` = K > 1, "fused"
    evaluates the K members side by side (``bb_run_eval_fused_group``): the first member's evaluation of a step
    runs the K rollouts in one launch per episode index, the others are handed their arrays.

    ``seeds_per_gpu`` = K > 1: seed k is ``rank_seed(train_seed, K) + k``, with its own nets (built right after
    ``torch.manual_seed(seed)``), its own block permutation (``perm``: a sequence of K permutations; None: K
    draws in member order from torch's global generator, before any seed is set), its own evaluations
    (``seed = eval_seed + step``, as K separate runs), best score and checkpoints under ``seed_<seed>/``, and a
    ``seed`` entry in its logger records; all K share one buffer and step as one ``SeedGroup`` with the indices
    of one K-way launch.  Every seed is bit-identical to ``train()`` of that seed alone with its permutation.
    Returns the list of K trainers."""
    if eval_on not in ("host", "device", "fused"):
        raise ValueError(f"eval_on must be 'host', 'device' or 'fused', got {eval_on!r}")
    K = int(seeds_per_gpu)
    seeds = group_seeds(config.train_seed, K)
    if K == 1:
        seeds = [config.train_seed]  # (one seed per GPU: every rank trains train_seed, as before)
    if device is None:
        device = D.local_device() or "cuda:0"
    if reward_model is None:
        _co._reward_model_missing("custom_offline_bb.train", config, "a callable with the reference's call shape "
                                  "(RewardPTContext wraps a RewardPT)", "load_PT")
    if eval_on in ("device", "fused") and not isinstance(reward_model, (RewardPT, RewardPTContext)):
        raise TypeError(f"train(eval_on='{eval_on}') needs a RewardPTContext or a RewardPT as reward_model: the device "
                        "rollout takes its rewards from one window_values call; eval_on='host' (bb_run_eval_IQL) "
                        "takes any callable")
    if move_stats is None:
        move_stats = load_stats(config.move_stats_path)
    if dataset is None:
        dataset = os.path.expanduser(config.dataset_path)
    if not isinstance(dataset, BBDataset):
        dataset = BBDataset(dataset, normalized_states=config.normalize_state,
                            normalized_rewards=config.normalize_reward, device=device)
    # bref:899-902: the loader is built, and its permutation drawn, before set_seed (one seed takes one ``perm``)
    samplers = BlockEpochSamplerGroup.draw(len(dataset), config.batch_size, K,
                                           [perm] if K == 1 and perm is not None else perm)
    state_shape, action_shape = dataset.shapes()
    state_dim, action_dim = state_shape[1], action_shape[1]
    limits = (dataset.max_actions().to(device), dataset.min_actions().to(device))
    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)

    # with K == 1 set_seed has just called torch.manual_seed(train_seed) and nothing has drawn since, so
    # _build_trainer's own torch.manual_seed(seed) leaves the generator where it is
    set_seed(seeds[0])  # np, random, torch, PYTHONHASHSEED
    trainers = [_co._build_trainer(config, s, state_dim, action_dim, limits, device,
                                   (GaussianPolicy, DeterministicPolicy), ImplicitQLearning) for s in seeds]
    if eval_on == "fused":
        _fused_actor_descs([t.actor for t in trainers])  # (the envelope, before the first step)
    replay_buffer = ReplayBuffer(state_dim, action_dim, len(dataset), device)
    replay_buffer.load_dataset(dataset.transitions())
    if samplers.n_rows != replay_buffer.index_bound():
        raise ValueError(f"the samplers walk {samplers.n_rows} rows, the buffer holds {replay_buffer.index_bound()}")
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    def steps(group, active, t, n):  # (always all K seeds: they end together)
        idx, valid = samplers.device_indices(t, n, device)
        return group.train_steps(replay_buffer, n, config.batch_size, indices=idx, n_valid=valid, return_losses=True)

    group_eval = {"step": None, "returns": None}

    def evaluate(k, trainer, step):  # (the four bb_run_eval_* are the module's globals at call time)
        kw = dict(num_episodes=config.eval_episodes, r_model=reward_model, move_stats=move_stats,
                  state_mean=dataset.state_mean(), state_std=dataset.state_std(), device=device)
        if eval_on == "fused" and K > 1:
            # the weights of no member change between the K calls of an evaluation step (the group has been
            # synchronized and queues nothing until all have been evaluated)
            if group_eval["step"] != step:
                group_eval["returns"] = bb_run_eval_fused_group(actors=[t.actor for t in trainers],
                                                                seeds=[config.eval_seed + step] * K, **kw)
                group_eval["step"] = step
            return group_eval["returns"][k]
        run_eval = {"device": bb_run_eval_device, "fused": bb_run_eval_fused}.get(eval_on, bb_run_eval_IQL)
        return run_eval(actor=trainer.actor, seed=config.eval_seed + step, **kw)

    _offline_loop.run(trainers, seeds, lambda active: stepper(trainers), int(config.update_steps),
                      int(config.eval_every), chunk, logger, ckpt_dirs, steps, evaluate,
                      _offline_loop.BestModelRecords(ckpt_dirs))
    return trainers if K > 1 else trainers[0]
