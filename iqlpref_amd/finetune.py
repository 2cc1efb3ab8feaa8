"""The ``algorithms/finetune/iql.py`` flavour of the path: offline pretraining, then online fine-tuning on a
replay buffer that grows on the device.  "fref:" = that file.

``offline_iterations`` steps are the chunked ``train_steps`` loop of the offline flavours, with numpy's index
stream drawn on the device.  Each of the ``online_iterations`` ticks after them is a plain host loop around
the same training step, with one small kernel for each thing the tick adds (csrc/online.hip):

1. ``ImplicitQLearning.explore_action``: the actor's forward and the noise / scale / clamp of fref:681-693;
2. ``env.step`` on the host;
3. ``ReplayBuffer.add_transition``: one packed row written at the ring pointer (fref:164-180);
4. ``train_steps(n_steps=1)`` on indices that ``GrowingIndexStream`` drew ahead for a whole chunk of ticks:
   the bound of tick j is known in advance, ``min(size + j + 1, buffer_size)`` (fref:156, 180).

What differs from ``offline/iql.py`` and how it maps onto the same kernels: no autocast (``precision="fp32"``),
the Polyak update written as ``(1 - tau) t + tau s`` (fref:71-73, ``polyak_form=1``), ``sample`` on numpy's
global generator over ``_size`` (fref:156), ``actor_dropout`` a float with 0.0 for none (fref:45, 314), and a
cosine schedule that keeps stepping past ``T_max = offline_iterations`` (fref:448, 513): the rate climbs again
as ``(1 + cos(pi t / T_max)) / 2`` does, on the host's bookkeeping and in the kernels alike.

``train(seeds_per_gpu=K)`` runs K such seeds side by side on one GPU.  The host waits once per tick whatever K
is, so the act (``explore_actions``), the append (``add_transitions``) and the gradient step (``SeedGroup``) of
all members go out as one launch sequence each; member k is bit for bit the run ``config.seed = seed_k`` is alone.

gym, d4rl and wandb are imported only when ``train()`` is not handed what they would provide.
"""
import contextlib
import ctypes as C
import math
import os
import uuid
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _d4rl, _lib, _offline_loop
from . import distributed as D
from ._lib import check, ptr, stream_ptr
from .custom_offline import NP_STATE_WORDS, NumpyIndexStream, pack_np_state, unpack_np_state
from .iql import DeterministicPolicy, GaussianPolicy, TwinQ, ValueFunction, compute_mean_std, normalize_states, set_seed
from .iql import ImplicitQLearning as _OfflineIQL
from .iql import ReplayBuffer as _OfflineReplayBuffer
from .iql import _buffer_generation
from .multi import stepper
from .train import wrap_env  # noqa: F401  (fref:86-105)

ENVS_WITH_GOAL = ("antmaze", "pen", "door", "hammer", "relocate")  # fref:28


@dataclass
class TrainConfig:
    """fref:31-68, same fields and defaults."""
    device: str = "cuda"
    env: str = "antmaze-umaze-v2"
    seed: int = 0
    eval_seed: int = 0
    eval_freq: int = int(5e4)
    n_episodes: int = 100
    offline_iterations: int = int(1e6)
    online_iterations: int = int(1e6)
    checkpoints_path: Optional[str] = None
    load_model: str = ""
    actor_dropout: float = 0.0
    buffer_size: int = 2_000_000
    batch_size: int = 256
    discount: float = 0.99
    tau: float = 0.005
    beta: float = 3.0
    iql_tau: float = 0.7
    expl_noise: float = 0.03
    noise_clip: float = 0.5
    iql_deterministic: bool = False
    normalize: bool = True
    normalize_reward: bool = False
    vf_lr: float = 3e-4
    qf_lr: float = 3e-4
    actor_lr: float = 3e-4
    project: str = "CORL"
    group: str = "IQL-D4RL"
    name: str = "IQL"

    def __post_init__(self):
        self.name = f"{self.name}-{self.env}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)


# --------------------------------------------------------------------------- #
# host helpers of the reference module
# --------------------------------------------------------------------------- #
LOCOMOTION = ("halfcheetah", "hopper", "walker2d")  # the environments whose rewards are scaled by the return range


def is_goal_reached(reward: float, info: Dict) -> bool:
    """fref:212-215: the environment's own ``goal_achieved`` flag where it reports one, else a positive reward."""
    return info["goal_achieved"] if "goal_achieved" in info else reward > 0


def modify_reward(dataset: Dict, env_name: str, max_episode_steps: int = 1000) -> Dict:
    """fref:259-271: rescales ``dataset["rewards"]`` in place (locomotion: by ``max_episode_steps`` over the range
    of the episode returns, taken with the project's vectorised ``relabel.return_reward_range``; antmaze: minus
    one) and returns the ``reward_mod_dict`` that ``modify_reward_online`` takes as keywords."""
    if any(tag in env_name for tag in LOCOMOTION):
        from .relabel import return_reward_range
        lo, hi, _ = return_reward_range(dataset, max_episode_steps)
        dataset["rewards"] /= hi - lo
        dataset["rewards"] *= max_episode_steps
        return {"max_ret": hi, "min_ret": lo, "max_episode_steps": max_episode_steps}
    if "antmaze" in env_name:
        dataset["rewards"] -= 1.0
    return {}


def modify_reward_online(reward: float, env_name: str, **reward_mod) -> float:
    """fref:274-280: one environment reward through what ``modify_reward`` did to the dataset's; ``reward_mod`` is
    the dict it returned.  The division and the multiplication stay two operations, as on the dataset."""
    if any(tag in env_name for tag in LOCOMOTION):
        scaled = reward / (reward_mod["max_ret"] - reward_mod["min_ret"])
        return scaled * reward_mod["max_episode_steps"]
    return reward - 1.0 if "antmaze" in env_name else reward


def eval_actor(env, actor, device: str, n_episodes: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """fref:218-241: ``n_episodes`` sequential episodes of a gym < 0.26 environment, greedy actions from
    ``actor.act`` (one exact-fp32 forward on the GPU per step).  Returns (episode returns, success rate);
    the actor is handed back in train mode."""
    env.seed(seed)
    actor.eval()
    episode_rewards, successes = [], []
    try:
        for _ in range(n_episodes):
            state, done = env.reset(), False
            episode_reward = 0.0
            goal_achieved = False
            while not done:
                action = actor.act(np.asarray(state), device)
                state, reward, done, env_infos = env.step(action)
                episode_reward += reward
                if not goal_achieved:
                    goal_achieved = is_goal_reached(reward, env_infos)
            successes.append(float(goal_achieved))
            episode_rewards.append(episode_reward)
    finally:
        actor.train()
    return np.asarray(episode_rewards), np.mean(successes)


# --------------------------------------------------------------------------- #
# replay buffer (fref:108-181)
# --------------------------------------------------------------------------- #
def ring_advance(pointer: int, size: int, n: int, buffer_size: int) -> Tuple[int, int]:
    """fref:179-180, n times: (``_pointer``, ``_size``) after ``n`` transitions went into the ring."""
    return (pointer + n) % buffer_size, min(size + n, buffer_size)


class ReplayBuffer(_OfflineReplayBuffer):
    """The offline buffer with a ring that takes new transitions.  All ``buffer_size`` packed rows are
    allocated up front (the offline buffer allocates only what it loads); ``sample`` draws from ``_size`` on
    numpy's global generator (fref:156); ``load_d4rl_dataset`` leaves ``_pointer`` at the dataset's length
    (fref:151)."""

    def __init__(self, state_dim: int, action_dim: int, buffer_size: int, device: str = "cpu"):
        if int(buffer_size) < 1:
            raise ValueError("buffer_size must be >= 1")
        super().__init__(state_dim, action_dim, int(buffer_size), device)
        W = 2 * state_dim + action_dim + 2  # one transition in the staging order s | a | r | s' | d
        self._stage_host = torch.zeros(W, dtype=torch.float32).pin_memory()
        self._stage_dev = torch.zeros(W, dtype=torch.float32, device=self._dev)
        self._stage_free: Optional[torch.cuda.Event] = None

    def _alloc(self, n):
        if getattr(self, "_rows", None) is not None and self._rows.shape[0] == self._buffer_size:
            return  # (load_device_arrays asks for its n rows: the ring is there already, zeros beyond them)
        try:
            super()._alloc(self._buffer_size)
        except torch.cuda.OutOfMemoryError as e:
            gib = self._buffer_size * self._stride * 4 / 2**30
            raise MemoryError(f"finetune.ReplayBuffer: buffer_size = {self._buffer_size} rows of {self._stride} floats "
                              f"({gib:.1f} GiB) do not fit on {self._dev}; pass a smaller buffer_size ({e})") from None

    def view(self) -> _lib.ReplayView:
        key = (self._rows.data_ptr(), self._size, self._generation)
        if getattr(self, "_view_key", None) != key:
            self._view = _lib.ReplayView(ptr(self._rows), self._size, self._stride, self._state_dim, self._action_dim,
                                         self._generation)
            self._view_key = key
        return self._view

    def index_bound(self) -> int:
        """The ``hi`` of fref:156."""
        return self._size

    def sample(self, batch_size: int, indices=None):
        if indices is None:
            indices = torch.from_numpy(np.random.randint(0, self._size, size=batch_size)).to(self._dev)
        return super().sample(batch_size, indices)

    def append_device(self, obs: torch.Tensor, act: torch.Tensor, rew: torch.Tensor, nxt: torch.Tensor,
                      done: torch.Tensor):
        """``n`` transitions that already live on the device (fp32 [n, S], [n, A], [n], [n, S], [n]) in one
        ``iqlhip_replay_append`` launch: row ``(_pointer + i) % buffer_size`` receives transition i."""
        n, S, A = int(obs.shape[0]), self._state_dim, self._action_dim
        f = lambda t, shape: t.to(device=self._dev, dtype=torch.float32).reshape(shape).contiguous()
        obs, act, nxt, rew, done = f(obs, (n, S)), f(act, (n, A)), f(nxt, (n, S)), f(rew, (n,)), f(done, (n,))
        if n > self._buffer_size:
            raise ValueError(f"{n} transitions do not fit a replay buffer of {self._buffer_size} rows")
        with _appending([self], n), torch.cuda.device(self._dev):
            check(self._lib.iqlhip_replay_append(ptr(self._rows), self._stride, S, A, self._buffer_size, self._pointer, n,
                                                 ptr(obs), ptr(act), ptr(rew), ptr(nxt), ptr(done), stream_ptr()))
        for t in (obs, act, rew, nxt, done):
            t.record_stream(torch.cuda.current_stream(self._dev))

    def add_transition(self, state: np.ndarray, action: np.ndarray, reward: float, next_state: np.ndarray, done: bool):
        """fref:164-180: one pinned staging block, one copy, one launch; nothing waits on the host except for
        the previous call's copy out of the same block."""
        S, A = self._state_dim, self._action_dim
        with _appending([self], 1):
            if self._stage_free is not None:
                self._stage_free.synchronize()
            _stage(self._stage_host.numpy()[None], S, A, state, action, reward, next_state, done)
            d = self._stage_dev
            with torch.cuda.device(self._dev):
                d.copy_(self._stage_host, non_blocking=True)
                if self._stage_free is None:
                    self._stage_free = torch.cuda.Event()
                self._stage_free.record()
                base, sz = d.data_ptr(), 4
                at = lambda off: C.c_void_p(base + off * sz)
                check(self._lib.iqlhip_replay_append(ptr(self._rows), self._stride, S, A, self._buffer_size, self._pointer,
                                                     1, at(0), at(S), at(S + A), at(S + A + 1), at(2 * S + A + 1),
                                                     stream_ptr()))


def _stage(h: np.ndarray, S: int, A: int, states, actions, rewards, next_states, dones):
    """K transitions into the [K, W] staging block ``h`` in the order s | a | r | s' | d (five assignments
    whatever K is: the block is filled column-wise)."""
    K = h.shape[0]
    h[:, :S] = np.asarray(states, dtype=np.float32).reshape(K, S)
    h[:, S:S + A] = np.asarray(actions, dtype=np.float32).reshape(K, A)
    h[:, S + A] = np.asarray(rewards, dtype=np.float32).reshape(K)
    h[:, S + A + 1:2 * S + A + 1] = np.asarray(next_states, dtype=np.float32).reshape(K, S)
    h[:, 2 * S + A + 1] = np.asarray(dones, dtype=np.float32).reshape(K)


@contextlib.contextmanager
def _appending(bufs: Sequence[ReplayBuffer], n: int):
    """Around the launch that writes ``n`` rows at every ring's pointer: all rings are checked before anything is
    written, and pointer, size and generation advance only when the body raised nothing."""
    for b in bufs:
        if b._pointer >= b._buffer_size:  # (a dataset that filled the buffer: fref:173 indexes past the end)
            raise IndexError(f"index {b._pointer} is out of bounds for a replay buffer of {b._buffer_size} rows")
    yield
    for b in bufs:
        b._pointer, b._size = ring_advance(b._pointer, b._size, n, b._buffer_size)
        _buffer_generation[0] += 1
        b._generation = _buffer_generation[0]  # the rows changed: no prefetched batch survives


def add_transitions(buffers: Sequence[ReplayBuffer], states, actions, rewards, next_states, dones):
    """``buffers[k].add_transition(states[k], actions[k], rewards[k], next_states[k], dones[k])`` for K rings of
    one geometry on one device: one pinned [K, W] staging block, one copy and ONE
    ``iqlhip_replay_append_group`` launch; nothing waits on the host except for the previous call's copy out
    of the same block.  Every ring is checked as ``add_transition`` checks it before anything is written."""
    bufs = list(buffers)
    K = len(bufs)
    if not 1 <= K <= _lib.MAX_GROUP:
        raise ValueError(f"add_transitions takes 1..{_lib.MAX_GROUP} replay buffers (got {K})")
    b0 = bufs[0]
    S, A = b0._state_dim, b0._action_dim
    if any(len(x) != K for x in (states, actions, rewards, next_states, dones)):
        raise ValueError(f"add_transitions: one state, action, reward, next state and done flag per buffer ({K})")
    if len({id(b) for b in bufs}) != K:
        raise ValueError("a replay buffer may appear only once")
    for b in bufs:
        if (b._state_dim, b._action_dim, b._stride, b._dev) != (S, A, b0._stride, b0._dev):
            raise ValueError("add_transitions: all replay buffers must have one state_dim, action_dim and device")
    with _appending(bufs, 1):
        stage = getattr(b0, "_group_stage", None)
        if stage is None or stage[0].shape[0] != K:
            stage = b0._group_stage = (torch.zeros((K, 2 * S + A + 2), dtype=torch.float32).pin_memory(),
                                       torch.zeros((K, 2 * S + A + 2), dtype=torch.float32, device=b0._dev),
                                       torch.cuda.Event())
        host, dev, free = stage
        free.synchronize()  # (an event never recorded is complete)
        _stage(host.numpy(), S, A, states, actions, rewards, next_states, dones)
        with torch.cuda.device(b0._dev):
            dev.copy_(host, non_blocking=True)
            free.record()
            check(b0._lib.iqlhip_replay_append_group((C.c_void_p * K)(*[b._rows.data_ptr() for b in bufs]), b0._stride, S,
                                                     A, (C.c_int64 * K)(*[b._buffer_size for b in bufs]),
                                                     (C.c_int64 * K)(*[b._pointer for b in bufs]), K, ptr(dev),
                                                     stream_ptr()))


# --------------------------------------------------------------------------- #
# numpy's index stream over a growing buffer
# --------------------------------------------------------------------------- #
def bound_schedule(hi0: int, cap: int, n_steps: int, growth: int = 1) -> np.ndarray:
    """``hi_t = min(hi0 + t * growth, cap)`` for t < n_steps: the bounds ``iqlhip_np_randint_growing`` draws
    under.  For the online ticks that follow a buffer of ``size`` rows: ``hi0 = min(size + 1, buffer_size)``."""
    return np.minimum(int(hi0) + np.arange(int(n_steps), dtype=np.int64) * int(growth), int(cap))


class GrowingIndexStream:
    """``np.random.randint(0, hi_t, size=B)`` for ``n_steps`` consecutive steps with the bounds of
    ``bound_schedule``, for K generators at once, in ONE launch of ``iqlhip_np_randint_growing``; every
    generator (an ``np.random.RandomState``, or None for numpy's global one) is left where the host calls
    would have left it.  Synchronous: the online tick waits for its action every step anyway."""

    def __init__(self, device):
        self._lib = _lib.load()
        self._dev = _lib.require_gpu(device)
        G = _lib.MAX_GROUP
        self._state = torch.empty((G, NP_STATE_WORDS), dtype=torch.int32, device=self._dev)
        self._host = torch.empty((G, NP_STATE_WORDS), dtype=torch.int32).pin_memory()

    def draw(self, hi0, cap, n_steps: int, batch_size: int, growth: int = 1,
             generators: Optional[Sequence] = None):
        gens = [None] if generators is None else list(generators)
        K = len(gens)
        his = [int(hi0)] * K if np.ndim(hi0) == 0 else [int(h) for h in hi0]
        caps = [int(cap)] * K if np.ndim(cap) == 0 else [int(c) for c in cap]
        n, B = int(n_steps), int(batch_size)
        if not 1 <= K <= _lib.MAX_GROUP or len(his) != K or len(caps) != K:
            raise ValueError(f"1..{_lib.MAX_GROUP} generators, one hi0 and one cap per generator")
        if n < 1 or B < 1 or growth not in (0, 1):
            raise ValueError("n_steps and batch_size must be >= 1, growth 0 or 1")
        if any(h < 1 for h in his) or any(c < h for c, h in zip(caps, his)):
            raise ValueError(f"every stream needs 1 <= hi0 <= cap (got hi0 = {his}, cap = {caps})")
        before = []
        for k, g in enumerate(gens):
            st = (np.random if g is None else g).get_state(legacy=True)
            self._host[k].numpy().view(np.uint32)[:] = pack_np_state(st)
            before.append(st)
        area = torch.empty((K, n, B), dtype=torch.int64, device=self._dev)
        outs = (C.c_void_p * K)(*[area[k].data_ptr() for k in range(K)])
        with torch.cuda.device(self._dev):
            self._state[:K].copy_(self._host[:K], non_blocking=True)
            check(self._lib.iqlhip_np_randint_growing(ptr(self._state), (C.c_int64 * K)(*his), (C.c_int64 * K)(*caps),
                                                      int(growth), K, B, n, outs, stream_ptr()))
            self._host[:K].copy_(self._state[:K], non_blocking=True)
            torch.cuda.current_stream(self._dev).synchronize()
        for k, g in enumerate(gens):
            (np.random if g is None else g).set_state(unpack_np_state(self._host[k].numpy(), before[k]))
        return [area[k] for k in range(K)]


# --------------------------------------------------------------------------- #
# trainer (fref:423-563)
# --------------------------------------------------------------------------- #
def cosine_rate(base_lr: float, t: int, t_max: int, eta_min: float = 0.0) -> float:
    """The actor's rate for its step number ``t`` (0-based) in closed form, what ``CosineAnnealingLR``'s recursion
    follows for every t -- past ``T_max`` too, where it climbs again (period 2 ``T_max``).  The trainer's host
    bookkeeping and the kernels' in-step rate evaluate this expression in float64."""
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * t / t_max)) / 2


def _act_args(dev, S: int, A: int, states, eps, rows: Optional[int] = None):
    """``states`` [rows, S] and ``eps`` [rows, A] | None (arrays or tensors) as contiguous float32 tensors on
    ``dev``; ``rows`` None takes as many as ``states`` has, at least one."""
    # (host arrays are rounded to float32 on the host: one copy up, no cast kernel behind it)
    up = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    s = up(states).to(device=dev, dtype=torch.float32).reshape(-1, S).contiguous()
    if s.shape[0] < 1 or rows not in (None, s.shape[0]):
        raise ValueError(f"states must have shape (rows, {S}) with rows {rows or '>= 1'}, got {tuple(s.shape)}")
    if eps is not None:
        eps = up(eps).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(eps.shape) != (s.shape[0], A):
            raise ValueError(f"eps must have shape {(s.shape[0], A)} (rows, A), got {tuple(eps.shape)}")
    return s, eps


class ImplicitQLearning(_OfflineIQL):
    """fref:423-563 on the same kernels: no autocast, convex Polyak form, ``max_steps`` the cosine ``T_max``
    (``train()`` passes ``offline_iterations``; the online steps run past it)."""

    def __init__(self, max_action, actor, actor_optimizer, q_network, q_optimizer, v_network, v_optimizer,
                 iql_tau: float = 0.7, beta: float = 3.0, max_steps: int = 1000000, discount: float = 0.99,
                 tau: float = 0.005, device: str = "cpu", *, seed: Optional[int] = None, keep_grads: bool = False,
                 precision: str = "fp32"):
        super().__init__(max_action, actor, actor_optimizer, q_network, q_optimizer, v_network, v_optimizer,
                         iql_tau=iql_tau, beta=beta, max_steps=max_steps, discount=discount, tau=tau, device=device,
                         precision=precision, seed=seed, keep_grads=keep_grads, polyak_form=1)
        self._explore_calls = 0

    def explore_action(self, states, eps=None, *, expl_noise: float = 0.03, noise_clip: float = 0.5,
                       batch_size: Optional[int] = None) -> torch.Tensor:
        """fref:681-693 for ``states`` [rows, S] (array or tensor): the actor's forward on the live weights,
        then ``mean + std * eps`` (Gaussian) or ``out + clamp(expl_noise * eps, +-noise_clip)`` (deterministic),
        scaled by ``max_action`` and clamped to it.  ``eps`` [rows, A]: the standard normals to use; None
        draws them on the device from the trainer's Philox key.  Returns a float32 device tensor [rows, A]."""
        if self._precision != _lib.PREC_FP32:
            raise NotImplementedError("explore_action needs a precision='fp32' trainer (the fine-tune flavour runs "
                                      "without autocast)")
        s, eps = _act_args(self._dev, self._state_dim, self._action_dim, states, eps)
        rows = s.shape[0]
        self._ensure_handle(batch_size or self._handle_batch or 32)
        out = torch.empty((rows, self._action_dim), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_explore_action(self._handle, ptr(s), rows, ptr(eps), float(expl_noise),
                                                  float(noise_clip), float(self.max_action),
                                                  self._explore_calls & 0xFFFFFFFF, ptr(out), stream_ptr()))
        self._explore_calls += 1
        return out

    def state_dict(self):
        """The reference's keys and ``explore_calls``: the number that keys the next exploring call's noise and
        dropout masks, so that a resumed run does not draw the blocks of its first ticks again."""
        sd = super().state_dict()
        sd["explore_calls"] = self._explore_calls
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        self._explore_calls = int(sd.pop("explore_calls", 0))  # (a checkpoint of the reference has none)
        super().load_state_dict(sd)


def explore_actions(trainers: Sequence[ImplicitQLearning], states, eps=None, *, expl_noise: float, noise_clip: float,
                    batch_size: Optional[int] = None) -> torch.Tensor:
    """``trainers[k].explore_action(states[k:k + 1], eps[k:k + 1])`` for K trainers (1..``_lib.MAX_GROUP``, one
    device, one state_dim / action_dim / max_action; depth, width, policy kind, dropout and seed each member's
    own) in ONE ``iqlhip_explore_action_group`` launch: row k of the float32 device tensor [K, A] that comes
    back has the bits the member's own call would give.  ``states`` [K, S], ``eps`` None or [K, A].  Every
    trainer's call number advances by one."""
    trs = list(trainers)
    K = len(trs)
    if not 1 <= K <= _lib.MAX_GROUP:
        raise ValueError(f"explore_actions takes 1..{_lib.MAX_GROUP} trainers (got {K})")
    t0 = trs[0]
    for t in trs:
        if t._precision != _lib.PREC_FP32:
            raise NotImplementedError("explore_actions needs precision='fp32' trainers (the fine-tune flavour runs "
                                      "without autocast)")
    for t in trs:
        if (t._state_dim, t._action_dim, t._dev, float(t.max_action)) != \
                (t0._state_dim, t0._action_dim, t0._dev, float(t0.max_action)):
            raise ValueError("explore_actions: all trainers must have one state_dim, action_dim, max_action and device")
    S, A = t0._state_dim, t0._action_dim
    s, eps = _act_args(t0._dev, S, A, states, eps, rows=K)
    for t in trs:
        t._ensure_handle(batch_size or t._handle_batch or 32)
    out = torch.empty((K, A), dtype=torch.float32, device=t0._dev)
    with torch.cuda.device(t0._dev):
        check(t0._lib.iqlhip_explore_action_group((C.c_void_p * K)(*[t._handle.value for t in trs]), K, ptr(s), S, ptr(eps),
                                                  float(expl_noise), float(noise_clip), float(t0.max_action),
                                                  (C.c_uint32 * K)(*[t._explore_calls & 0xFFFFFFFF for t in trs]),
                                                  ptr(out), stream_ptr()))
    for t in trs:
        t._explore_calls += 1
    return out


# --------------------------------------------------------------------------- #
# train (fref:566-767)
# --------------------------------------------------------------------------- #
def _gym_and_d4rl():
    try:
        import d4rl
        import gym
    except ImportError:
        raise ImportError("finetune.train: env=None / dataset=None build them with gym and d4rl, which are not "
                          "installed; pass env=, eval_env= and dataset=") from None
    return gym, d4rl


def _member_envs(env, K: int, what: str):
    """``env`` / ``eval_env`` as it was given -- for one seed the environment itself, for K > 1 a callable
    ``k -> env`` or K environments -- as a callable ``k -> env``; None stays None."""
    if env is None or (K > 1 and callable(env)):
        return env
    if K == 1:
        return lambda k: env
    if not isinstance(env, (list, tuple)) or len(env) != K:
        n = len(env) if isinstance(env, (list, tuple)) else 1
        raise ValueError(f"finetune.train(seeds_per_gpu={K}): {what} must be {K} environments or a callable "
                         f"k -> env (got {n})")
    return list(env).__getitem__


def train(config: TrainConfig, env=None, eval_env=None, dataset: Optional[Dict[str, np.ndarray]] = None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None,
          normalized_score: Optional[Callable[[float], float]] = None, device: Optional[str] = None,
          chunk: int = 2000, online_chunk: int = 256,
          exploration_noise: Optional[Callable[[int], Union[np.ndarray, torch.Tensor]]] = None,
          on_start: Optional[Callable] = None, seeds_per_gpu: int = 1):
    """fref:566-767 on the HIP path.

    ``env`` / ``eval_env``: gym < 0.26 environments (``seed``, ``reset() -> obs``, ``step(a) -> (obs, r, done,
    info)``, ``_max_episode_steps``, spaces); None builds ``gym.make(config.env)``.  ``dataset``: the d4rl
    transition dict (None: ``d4rl.qlearning_dataset(env)``); its rewards are rescaled in place with
    ``normalize_reward``, as fref does.  ``logger(record, step)``: one call per ``wandb.log`` of fref (default:
    wandb when importable, else print).  ``normalized_score(score)``: default ``eval_env.get_normalized_score``.

    Offline steps run in chunks of at most ``chunk`` that end on evaluation boundaries, their indices drawn
    by ``NumpyIndexStream``.  The indices of the online ticks are drawn ``online_chunk`` ticks ahead by
    ``GrowingIndexStream``: numpy's global generator then runs ahead of the environment by up to that many
    draws, which only an environment that itself reads numpy's global generator could notice
    (``online_chunk=1`` keeps fref's interleaving).  Losses come back to the host once per chunk.
    ``exploration_noise(tick)``: the standard normals [A] of online tick ``tick`` (parity runs); None draws
    them on the device.  ``on_start(trainer, replay_buffer)`` is called before the first step.
    Returns the trainer.

    ``seeds_per_gpu`` = K > 1 (up to ``_lib.MAX_GROUP``): K runs side by side on one GPU, run k what this
    function does alone under ``config.seed = rank_seed(config.seed, K) + k`` -- bit for bit, as long as no
    environment reads numpy's global generator (member k draws its indices from its own
    ``np.random.RandomState(seed_k)``).  ``env`` / ``eval_env``: sequences of K environments or a callable
    ``k -> env``.  The loop is the same one over K members; only what a tick launches differs: it acts for all
    members in one launch (``explore_actions``), steps the K environments on the host, appends in one launch
    (``add_transitions``) and takes one ``SeedGroup`` step, where one seed calls its trainer's and its ring's
    own methods.  Records carry a ``seed`` entry, checkpoints go under ``seed_<s>/``, ``exploration_noise(tick)``
    returns [K, A], ``on_start(trainers, replay_buffers)`` gets the lists, and the list of trainers is returned.

    There is no ``resume`` here (``train`` / ``sweep.train_runs`` / ``custom_offline`` have one): the replay ring
    grows on the device, and going on bit for bit would need a snapshot of it and of the index stream drawn ahead."""
    K = int(seeds_per_gpu)
    if not 1 <= K <= _lib.MAX_GROUP:
        raise ValueError(f"seeds_per_gpu must be in 1..{_lib.MAX_GROUP}")
    env, eval_env = _member_envs(env, K, "env"), _member_envs(eval_env, K, "eval_env")
    device = _d4rl.default_device(config, device)
    if env is None or eval_env is None or dataset is None:
        gym, d4rl = _gym_and_d4rl()
        env = (lambda k: gym.make(config.env)) if env is None else env
        eval_env = (lambda k: gym.make(config.env)) if eval_env is None else eval_env
    ks = range(K)
    envs, eval_envs = [env(k) for k in ks], [eval_env(k) for k in ks]
    if dataset is None:
        dataset = d4rl.qlearning_dataset(envs[0])
    normalized = [e.get_normalized_score for e in eval_envs] if normalized_score is None else [normalized_score] * K
    is_env_with_goal = config.env.startswith(ENVS_WITH_GOAL)
    max_steps = envs[0]._max_episode_steps
    state_dim = envs[0].observation_space.shape[0]
    action_dim = envs[0].action_space.shape[0]
    n_off, n_on, B = int(config.offline_iterations), int(config.online_iterations), int(config.batch_size)

    # ---- dataset and normalisation once, one ring per member (fref:578-603) ----
    reward_mod_dict = {}
    if config.normalize_reward:
        reward_mod_dict = modify_reward(dataset, config.env)
    if config.normalize:
        state_mean, state_std = compute_mean_std(dataset["observations"], eps=1e-3)
    else:
        state_mean, state_std = 0, 1
    dataset["observations"] = normalize_states(dataset["observations"], state_mean, state_std)
    dataset["next_observations"] = normalize_states(dataset["next_observations"], state_mean, state_std)
    envs = [wrap_env(e, state_mean=state_mean, state_std=state_std) for e in envs]
    eval_envs = [wrap_env(e, state_mean=state_mean, state_std=state_std) for e in eval_envs]
    # one seed keeps config.seed as it is (under torchrun too: no rank offset)
    seeds = [config.seed] if K == 1 else [D.rank_seed(config.seed, K) + k for k in ks]
    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)
    tagged = _offline_loop.tag(seeds)
    up = lambda name: torch.tensor(dataset[name], dtype=torch.float32, device=device)
    arrays = [up(n) for n in ("observations", "actions", "rewards", "next_observations", "terminals")]
    buffers = []
    for k in ks:
        try:
            buffers.append(ReplayBuffer(state_dim, action_dim, config.buffer_size, device))
            buffers[k].load_device_arrays(*arrays)
        except MemoryError as e:
            if K == 1:
                raise
            raise MemoryError(f"finetune.train(seeds_per_gpu={K}): the ring of member {k} of {K}: {e}") from None
    del arrays
    max_action = float(envs[0].action_space.high[0])

    # ---- seeds and nets, member by member as a run of its own sets them up (fref:613-660) ----
    dropout = config.actor_dropout if config.actor_dropout and config.actor_dropout > 0.0 else None  # fref:314
    policy = DeterministicPolicy if config.iql_deterministic else GaussianPolicy
    trainers = []
    for k, seed in enumerate(seeds):
        set_seed(seed, envs[k])
        eval_envs[k].seed(config.eval_seed)
        eval_envs[k].action_space.seed(config.eval_seed)
        q_network = TwinQ(state_dim, action_dim).to(device)
        v_network = ValueFunction(state_dim).to(device)
        actor = policy(state_dim, action_dim, max_action, dropout=dropout).to(device)
        v_optimizer = torch.optim.Adam(v_network.parameters(), lr=config.vf_lr)
        q_optimizer = torch.optim.Adam(q_network.parameters(), lr=config.qf_lr)
        actor_optimizer = torch.optim.Adam(actor.parameters(), lr=config.actor_lr)
        print("---------------------------------------")
        print(f"Training IQL, Env: {config.env}, Seed: {seed}")
        print("---------------------------------------")
        trainers.append(ImplicitQLearning(max_action=max_action, actor=actor, actor_optimizer=actor_optimizer,
                                          q_network=q_network, q_optimizer=q_optimizer, v_network=v_network,
                                          v_optimizer=v_optimizer, discount=config.discount, tau=config.tau,
                                          device=device, beta=config.beta, iql_tau=config.iql_tau, max_steps=n_off,
                                          seed=seed))
        if config.load_model != "":
            trainers[k].load_state_dict(torch.load(config.load_model))
    if logger is None:
        logger = _offline_loop.default_logger(config, K)
    if on_start is not None:
        on_start(*((trainers[0], buffers[0]) if K == 1 else (trainers, buffers)))

    # ---- what a tick launches: one seed stays on its trainer's and its ring's own calls (the group kernels
    # cost more per member), K > 1 send each part out once for all members ----
    act_kw = dict(expl_noise=config.expl_noise, noise_clip=config.noise_clip, batch_size=B)
    if K == 1:
        gens, mode = None, None  # (numpy's global generator, as set_seed left it)
        act = lambda states, eps: trainers[0].explore_action(states, eps, **act_kw).cpu().numpy()
        append = lambda s, a, r, s2, d: buffers[0].add_transition(s[0], a[0], r[0], s2[0], d[0])
    else:
        # what np.random.seed(seed_k) leaves numpy's global generator in, one generator per member
        gens = [np.random.RandomState(seed) for seed in seeds]
        # ONE launch sequence per step for all members (the two-stream split pays per call, and a tick is one step)
        mode = "general" if trainers[0].step_kind(B) == "general" else "group"
        act = lambda states, eps: explore_actions(trainers, states, eps, **act_kw).cpu().numpy()
        append = lambda *transitions: add_transitions(buffers, *transitions)
    group = stepper(trainers, mode=mode)
    step = lambda n, indices: group.train_steps(buffers, n, B, indices=indices, return_losses=True)

    train_successes = [[] for _ in ks]
    pending = []  # (first t, [K] device losses [n, 3], [K] lists of the online records of those steps, or None)

    def flush():
        for t0, losses, extras in pending:
            for k, arr in enumerate(l.cpu().numpy() for l in losses):
                for i, (v, q, a) in enumerate(arr.tolist()):
                    t = t0 + i
                    rec = {"value_loss": v, "q_loss": q, "actor_loss": a}
                    rec["offline_iter" if t < n_off else "online_iter"] = t if t < n_off else t - n_off
                    if extras is not None:
                        rec.update(extras[k][i])
                    logger(tagged(rec, k), t + 1)  # (step = trainer.total_it after the step, fref:734)
        pending.clear()

    def evaluate(t):
        """fref:736-767 after step t, member after member."""
        flush()
        group.synchronize()
        print(f"Time steps: {t + 1}")
        for k, seed in enumerate(seeds):
            eval_scores, success_rate = eval_actor(eval_envs[k], trainers[k].actor, device=device,
                                                   n_episodes=config.n_episodes, seed=seed)
            eval_score = eval_scores.mean()
            eval_log = {}
            if t >= n_off and is_env_with_goal:
                # (of the TRAINING episodes, as fref:751)
                eval_log["eval/regret"] = np.mean(1 - np.array(train_successes[k]))
                eval_log["eval/success_rate"] = success_rate
            normalized_eval_score = normalized[k](eval_score) * 100.0
            eval_log["eval/d4rl_normalized_score"] = normalized_eval_score
            print("---------------------------------------")
            print(f"{'Evaluation' if K == 1 else f'Seed {seed}: evaluation'} over {config.n_episodes} episodes: "
                  f"{eval_score:.3f} , D4RL score: {normalized_eval_score:.3f}")
            print("---------------------------------------")
            if ckpt_dirs[k] is not None:
                torch.save(trainers[k].state_dict(), os.path.join(ckpt_dirs[k], f"checkpoint_{t}.pt"))
            logger(tagged(eval_log, k), t + 1)

    every = int(config.eval_freq)
    states = [e.reset() for e in envs]
    episode_return, episode_step, goal_achieved = [0] * K, [0] * K, [False] * K

    # ---- offline pretraining: the chunked loop of the offline flavours ----
    print("Offline pretraining")
    offline_stream = NumpyIndexStream(device) if n_off > 0 else None
    t = 0
    while t < n_off:
        nxt = min(n_off, t + int(chunk), (t // every + 1) * every)
        losses = step(nxt - t, offline_stream.draw(buffers[0].index_bound(), nxt - t, B, gens))
        flush()
        pending.append((t, losses, None))
        t = nxt
        if t % every == 0:
            evaluate(t - 1)

    # ---- online tuning: act, step the environments, append, one gradient step ----
    if n_on > 0:
        print("Online tuning")
    online_stream = GrowingIndexStream(device) if n_on > 0 else None
    chunk_idx, chunk_t0 = None, 0
    for t in range(n_off, n_off + n_on):
        tick = t - n_off
        if chunk_idx is None or tick - chunk_t0 >= chunk_idx[0].shape[0]:
            flush()
            n = min(max(1, int(online_chunk)), n_on - tick)
            hi0 = [min(b.index_bound() + 1, int(config.buffer_size)) for b in buffers]
            chunk_idx, chunk_t0 = online_stream.draw(hi0, int(config.buffer_size), n, B, generators=gens), tick
        eps = None if exploration_noise is None else \
            torch.as_tensor(np.asarray(exploration_noise(tick))).reshape(K, action_dim)
        actions = act(np.asarray(states).reshape(K, -1), eps)
        online_logs, rewards, next_states, real_dones, after = [], [], [], [], []
        for k in ks:
            online_log = {}
            episode_step[k] += 1
            next_state, reward, done, env_infos = envs[k].step(actions[k])
            if not goal_achieved[k]:
                goal_achieved[k] = is_goal_reached(reward, env_infos)
            episode_return[k] += reward
            real_dones.append(bool(done and episode_step[k] < max_steps))  # (a timeout is no terminal)
            if config.normalize_reward:
                reward = modify_reward_online(reward, config.env, **reward_mod_dict)
            rewards.append(reward), next_states.append(next_state)
            if done:
                next_state = envs[k].reset()  # (the appended s' stays the one the step returned)
                if is_env_with_goal:
                    train_successes[k].append(goal_achieved[k])
                    online_log["train/regret"] = np.mean(1 - np.array(train_successes[k]))
                    online_log["train/is_success"] = float(goal_achieved[k])
                online_log["train/episode_return"] = episode_return[k]
                online_log["train/d4rl_normalized_episode_return"] = normalized[k](episode_return[k]) * 100.0
                online_log["train/episode_length"] = episode_step[k]
                episode_return[k], episode_step[k], goal_achieved[k] = 0, 0, False
            online_logs.append([online_log])
            after.append(next_state)
        append(states, actions, rewards, next_states, real_dones)
        states = after
        j = tick - chunk_t0
        pending.append((t, step(1, [c[j:j + 1] for c in chunk_idx]), online_logs))
        if (t + 1) % every == 0:
            evaluate(t)
    flush()
    group.synchronize()
    group.close()
    return trainers[0] if K == 1 else trainers
