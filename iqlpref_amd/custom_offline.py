"""The ``algorithms/custom_offline/iql.py`` flavour of the path -- what the
pen sweeps run (pt_sweeps/sweep_pen_human_pt.yaml:2).  "cref:" = that file.

Differences from ``algorithms/offline/iql.py`` and how they map onto the same kernels:

* dataset = Minari episodes; the preference-transformer relabel is PER EPISODE with the TRUE
  timesteps (cref:158-225): one forward over the first ``query_length`` steps of an episode gives
  the reward of each of them, every later step gets the last value of its rolling window.  Causal
  attention makes position i of that first forward equal to the last-token value of the prefix
  window [0, i], so the whole relabel is ONE ``iqlhip_pt_relabel`` call over windows
  (start, len, t0) = (ep + max(0, i - QL + 1), min(i + 1, QL), max(0, i + 1 - QL));
* ``query_length == 1``: a Markovian reward MLP (reward_models/q_mlp.py) over (s, a);
* ``ReplayBuffer.sample`` draws indices with numpy's global RNG (cref:277-284) -- reproduced
  exactly, either on the host with the same call (then uploaded) or on the device by
  ``NumpyIndexStream`` (csrc/np_sampler.hip: numpy's legacy ``randint`` bit for bit, the advanced
  state written back into the generator);
* no autocast (``precision="fp32"``), Polyak update written as (1 - tau) t + tau s (cref:85-87,
  ``polyak_form=1``), checkpoint key ``actor_lr_scheduler`` and no ``total_it`` (cref:546-556);
* ``modify_reward``: only the locomotion range scaling and antmaze's -1 (cref:145-155).

``train()`` is cref:597-749 with the absent services (minari, the Orbax reward-model readers,
wandb) injectable, and ``seeds_per_gpu`` seeds side by side on one GPU.  Its setup (``_train``) is shared
with ``custom_offline_br``; the train / evaluate / checkpoint loop itself is ``_offline_loop.run``, which
the BB flavour runs too.

Not built (stated): the Orbax / flax-nnx checkpoint readers ``load_PT`` / ``load_QMLP``
(reward_models/pref_transformer.py:280-327, q_mlp.py:100-168) need orbax + jax, which are absent;
``RewardPT.load_flax_params`` / ``QMLP.load_flax_params`` take the parameter pytree as numpy
arrays instead.  PT numerics stay "parity unpinned" (no runnable reference, no fixtures).
"""
import ctypes as C
import uuid
import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _offline_loop
from . import distributed as D
from ._lib import check, ptr
from .iql import DeterministicPolicy, GaussianPolicy, TwinQ, ValueFunction, compute_mean_std, normalize_states, set_seed
from .iql import ImplicitQLearning as _OfflineIQL
from .iql import ReplayBuffer as _OfflineReplayBuffer
from .iql import mlp_forward_f32
from .relabel import RewardPT

ACTIVATIONS = ("cos", "tanh", "relu", "softplus", "sin", "leaky_relu", "swish", "none")  # q_mlp.py:121-130


@dataclass
class TrainConfig:
    """cref:44-78, same fields and defaults."""
    project: str = "IQL-pref"
    group: str = "IQL-Minari-pref"
    name: str = "iql-p"
    gamma: float = 0.99
    tau: float = 0.005
    beta: float = 3.0
    iql_tau: float = 0.7
    iql_deterministic: bool = False
    vf_lr: float = 3e-4
    qf_lr: float = 3e-4
    actor_lr: float = 3e-4
    actor_dropout: Optional[float] = None
    dataset_id: str = "D4RL/pen/human-v2"
    reward_model_path: str = "~/iqlpref/pen_labels/mr_pen/best_model.ckpt"
    query_length: int = 1
    update_steps: int = int(1e6)
    buffer_size: int = 2_000_000
    batch_size: int = 256
    normalize_state: bool = True
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


# --------------------------------------------------------------------------- #
# reward models
# --------------------------------------------------------------------------- #
class QMLP(nn.Module):
    """reward_models/q_mlp.py:16-98: Linear layers over concat(s, a) (flax kernels are [in, out]),
    ``activations`` between them, ``activation_final`` on the scalar output."""

    def __init__(self, state_dim: int, action_dim: int, hidden_dims: Sequence[int] = (256, 256),
                 activations: str = "relu", activation_final: str = "none"):
        super().__init__()
        if activations not in ACTIVATIONS or activation_final not in ACTIVATIONS:
            raise ValueError(f"activations must be among {ACTIVATIONS}")
        dims = [state_dim + action_dim, *hidden_dims, 1]
        self.kernels = nn.ParameterList([nn.Parameter(torch.zeros(i, o)) for i, o in zip(dims[:-1], dims[1:])])
        self.biases = nn.ParameterList([nn.Parameter(torch.zeros(o)) for o in dims[1:]])
        self.activations, self.activation_final = activations, activation_final

    def load_flax_params(self, layers: Sequence[Dict[str, np.ndarray]]):
        """``layers``: [{"kernel": [in,out], "bias": [out]}, ...] in layer order (nnx.Linear)."""
        with torch.no_grad():
            for k, b, l in zip(self.kernels, self.biases, layers):
                k.copy_(torch.as_tensor(np.asarray(l["kernel"], np.float32)))
                b.copy_(torch.as_tensor(np.asarray(l["bias"], np.float32)))
        return self

    def forward(self, observations, actions) -> torch.Tensor:
        dev = self.kernels[0].device
        x = torch.cat([torch.as_tensor(observations, dtype=torch.float32, device=dev),
                       torch.as_tensor(actions, dtype=torch.float32, device=dev)], dim=-1)
        y = mlp_forward_f32(list(self.kernels), list(self.biases), x, w_in_out=True,
                            hidden_act=ACTIVATIONS.index(self.activations) + _lib.ACT_FLAX_BASE,
                            out_act=ACTIVATIONS.index(self.activation_final) + _lib.ACT_FLAX_BASE)
        return y.squeeze(-1)


def load_pt_flax_params(model: RewardPT, params: Dict[str, Any]) -> RewardPT:
    """Copy a flax-nnx PT parameter tree (reward_models/pref_transformer.py:170-209; numpy arrays,
    ``kernel`` [in, out], ``scale`` for LayerNorm weights, ``embedding`` for nnx.Embed) into the
    torch-layout container.  Keys: state_linear, action_linear, timestep_embed,
    stacked_layer_norm, gpt.layers.<i>.{layer_norm_0, attention.{in_linear,out_linear},
    layer_norm_1, mlp.{in_linear,out_linear}}, gpt.layer_norm, pref_linear."""
    sd = {}

    def walk(prefix, node):
        for k, v in node.items():
            name = f"{prefix}.{k}" if prefix else str(k)
            if isinstance(v, dict):
                walk(name, v)
            else:
                a = np.asarray(v, np.float32)
                if k == "kernel":
                    sd[prefix + ".weight"] = torch.from_numpy(np.ascontiguousarray(a.T))
                elif k in ("scale", "embedding"):
                    sd[prefix + ".weight"] = torch.from_numpy(a)
                elif k == "bias":
                    sd[prefix + ".bias"] = torch.from_numpy(a)
    walk("", params)
    missing = model.load_state_dict(sd, strict=False)
    bad = [k for k in missing.missing_keys if not k.endswith("causal_bias")]
    if bad or missing.unexpected_keys:
        raise KeyError(f"flax parameter tree does not match: missing {bad}, unexpected {missing.unexpected_keys}")
    return model


# --------------------------------------------------------------------------- #
# dataset (cref:158-225)
# --------------------------------------------------------------------------- #
def _concat_episodes(dataset: Iterable) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, List[int]]:
    """Episodes (Minari ``EpisodeData`` or dicts) -> the per-step arrays (observations, actions, next
    observations, terminations) of all of them end to end, and the number of steps of each."""
    obs, act, nxt, dones = [], [], [], []
    for ep in dataset:
        get = ep.__getitem__ if isinstance(ep, dict) else (lambda k: getattr(ep, k))
        o = np.asarray(get("observations"), np.float32)
        obs.append(o[:-1]), nxt.append(o[1:])
        act.append(np.asarray(get("actions"), np.float32))
        dones.append(np.asarray(get("terminations")))
    return (np.concatenate(obs), np.concatenate(act), np.concatenate(nxt), np.concatenate(dones),
            [a.shape[0] for a in act])


def episode_windows(lengths: Sequence[int], query_length: int):
    """(start, len, t0) of the relabel window of every step of every episode; ``start`` indexes
    the concatenated per-step arrays.  Closed form of the rolling loop at cref:172-211."""
    L = np.asarray(lengths, dtype=np.int64)
    ep_start = np.concatenate([[0], np.cumsum(L)[:-1]])
    step = np.arange(int(L.sum()), dtype=np.int64) - np.repeat(ep_start, L)  # step i inside its episode
    t0 = np.maximum(0, step + 1 - query_length)
    return np.repeat(ep_start, L) + t0, np.minimum(step + 1, query_length).astype(np.int32), t0.astype(np.int32)


def qlearning_dataset(dataset: Iterable, r_model, query_length: int = 1) -> Dict[str, np.ndarray]:
    """cref:158-225.  ``dataset`` iterates episodes (Minari ``EpisodeData`` or dicts) with
    ``observations`` [L+1, S], ``actions`` [L, A], ``terminations`` [L]."""
    obs, act, nxt, dones, lengths = _concat_episodes(dataset)
    if query_length > 1:
        if not isinstance(r_model, RewardPT):
            raise TypeError("query_length > 1 needs an iqlpref_amd RewardPT")
        dev = next(r_model.parameters()).device
        start, length, t0 = episode_windows(lengths, query_length)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        rewards = r_model.window_values(up(obs), up(act), up(start), up(length), query_length,
                                        win_t0=up(t0)).cpu().numpy()
    else:
        rewards = r_model(obs, act).cpu().numpy()
    return {"observations": obs, "actions": act, "next_observations": nxt,
            "rewards": rewards.astype(np.float32), "terminals": dones}


def return_reward_range(dataset, max_episode_steps):
    """cref:127-142 (same loop as the offline flavour, without trajectory lengths)."""
    from .relabel import return_reward_range as rr
    lo, hi, _ = rr(dataset, max_episode_steps)
    return lo, hi


def modify_reward(dataset: Dict[str, np.ndarray], env_name: str, max_episode_steps: int = 1000):
    """cref:145-155."""
    if any(s in env_name for s in ("halfcheetah", "hopper", "walker2d")):
        lo, hi = return_reward_range(dataset, max_episode_steps)
        dataset["rewards"] /= hi - lo
        dataset["rewards"] *= max_episode_steps
    elif "antmaze" in env_name:
        dataset["rewards"] -= 1.0


def evaluate(env, actor: nn.Module, num_episodes: int, seed: int, device: str) -> np.ndarray:
    """cref:559-579: ``num_episodes`` sequential episodes of a gymnasium-API environment
    (``reset(seed=seed + i)``), greedy actions from ``actor.act`` (one exact-fp32 forward on the GPU
    per step), undiscounted returns.  The actor is handed back in train mode (cref:578)."""
    actor.eval()
    episode_rewards = []
    try:
        for i in range(num_episodes):
            done = False
            state, _ = env.reset(seed=seed + i)
            episode_reward = 0.0
            while not done:
                state, reward, terminated, truncated, _ = env.step(actor.act(np.asarray(state), device))
                done = terminated or truncated
                episode_reward += reward
            episode_rewards.append(episode_reward)
    finally:
        actor.train()
    return np.asarray(episode_rewards)


# --------------------------------------------------------------------------- #
# numpy's legacy randint on the device (csrc/np_sampler.hip)
# --------------------------------------------------------------------------- #
NP_STATE_WORDS = 625  # key[624], pos


def pack_np_state(state) -> np.ndarray:
    """``RandomState.get_state()`` (legacy tuple) -> uint32 [625] = key[624], pos."""
    if state[0] != "MT19937":
        raise ValueError(f"not a legacy MT19937 state: {state[0]!r}")
    key, pos = np.asarray(state[1]), int(state[2])
    if key.shape != (624,) or not 0 <= pos <= 624:
        raise ValueError(f"bad MT19937 state: key shape {key.shape}, pos {pos}")
    out = np.empty(NP_STATE_WORDS, dtype=np.uint32)
    out[:624], out[624] = key, pos
    return out


def unpack_np_state(packed: np.ndarray, like) -> tuple:
    """uint32 [625] -> the legacy state tuple, with ``has_gauss`` / ``cached_gaussian`` of ``like``
    (the draw does not touch them)."""
    packed = np.asarray(packed).view(np.uint32)
    return ("MT19937", packed[:624].copy(), int(packed[624]), int(like[3]), float(like[4]))


class NumpyIndexStream:
    """``np.random.randint(0, hi, size=B)`` n times, for K generators at once, on the device.

    ``draw`` uploads the state of every generator (an ``np.random.RandomState``, or None for numpy's
    global one) into a device [K][625] buffer, draws [n][B] int64 indices per generator with ONE launch
    of ``iqlhip_np_randint`` and writes the advanced state back with ``set_state``: when ``draw``
    returns, every generator is where the host sampler would have left it, bit for bit.

    The draw runs on a stream of its own into one of two index areas used in turn; the consumer (the
    stream current at the call) waits on an event for the indices, and the draw of call n waits only
    for the consumer's work queued before call n - 1 (the last user of that area).  The host blocks
    for the short draw kernel, not for the training chunk queued just before it."""

    def __init__(self, device):
        self._lib = _lib.load()
        self._dev = _lib.require_gpu(device)
        G = _lib.MAX_GROUP
        self._state = torch.empty((G, NP_STATE_WORDS), dtype=torch.int32, device=self._dev)
        self._host_in = torch.empty((G, NP_STATE_WORDS), dtype=torch.int32).pin_memory()
        self._host_out = torch.empty((G, NP_STATE_WORDS), dtype=torch.int32).pin_memory()
        self._stream = torch.cuda.Stream(device=self._dev)
        self._slots: List[Optional[torch.Tensor]] = [None, None]
        self._free: List[Optional[torch.cuda.Event]] = [None, None]  # consumer done with the area
        self._done = torch.cuda.Event()
        self._turn = 0

    def draw(self, hi, n_batches: int, batch_size: int, generators: Optional[Sequence] = None) -> List[torch.Tensor]:
        """Returns K int64 device tensors [n_batches, batch_size] (views of the current index area,
        valid until the call after next).  ``hi``: one bound for all generators or one per generator."""
        gens = [None] if generators is None else list(generators)
        K = len(gens)
        his = [int(hi)] * K if np.ndim(hi) == 0 else [int(h) for h in hi]
        if not 1 <= K <= _lib.MAX_GROUP or len(his) != K:
            raise ValueError(f"1..{_lib.MAX_GROUP} generators, one hi per generator")
        n, B = int(n_batches), int(batch_size)
        if n < 1 or B < 1:
            raise ValueError("n_batches and batch_size must be >= 1")
        before = []
        for k, g in enumerate(gens):
            st = (np.random if g is None else g).get_state(legacy=True)
            self._host_in[k].numpy().view(np.uint32)[:] = pack_np_state(st)
            before.append(st)
        consumer = torch.cuda.current_stream(self._dev)
        slot = self._turn & 1
        ev = torch.cuda.Event()
        ev.record(consumer)  # the consumer's last use of the other area is queued by now
        self._free[slot ^ 1] = ev
        with torch.cuda.stream(self._stream):
            if self._free[slot] is not None:
                self._stream.wait_event(self._free[slot])
            area = self._slots[slot]
            if area is None or area.shape[0] < K or area.shape[1] < n * B:
                area = torch.empty((K, n * B), dtype=torch.int64, device=self._dev)
                self._slots[slot] = area
            self._state[:K].copy_(self._host_in[:K], non_blocking=True)
            outs = (C.c_void_p * K)(*[area[k].data_ptr() for k in range(K)])
            his_c = (C.c_int64 * K)(*his)
            with torch.cuda.device(self._dev):
                check(self._lib.iqlhip_np_randint(ptr(self._state), his_c, K, B, n, outs,
                                                  C.c_void_p(self._stream.cuda_stream)))
            self._host_out[:K].copy_(self._state[:K], non_blocking=True)
            self._done.record(self._stream)
        area.record_stream(consumer)
        self._done.synchronize()
        for k, g in enumerate(gens):
            (np.random if g is None else g).set_state(unpack_np_state(self._host_out[k].numpy(), before[k]))
        consumer.wait_event(self._done)
        self._turn += 1
        return [area[k, :n * B].view(n, B) for k in range(K)]


# --------------------------------------------------------------------------- #
# buffer and trainer
# --------------------------------------------------------------------------- #
class ReplayBuffer(_OfflineReplayBuffer):
    """cref:228-290: ``load_dataset`` + a sampler on numpy's GLOBAL generator -- after
    ``np.random.seed(s)`` the index stream is the reference's, draw for draw."""

    def load_dataset(self, data: Dict[str, np.ndarray]):
        self.load_d4rl_dataset(data)

    def index_bound(self) -> int:
        """The ``hi`` of cref:278: indices are drawn from [0, min(size, pointer))."""
        return min(self._size, self._pointer)

    def draw_indices(self, batch_size: int, n_batches: Optional[int] = None, rng=None) -> np.ndarray:
        """cref:278: ``np.random.randint(0, min(size, pointer), size=batch_size)``, once per batch
        (``rng``: an ``np.random.RandomState`` to draw from instead of the global generator)."""
        gen = np.random if rng is None else rng
        hi = self.index_bound()
        if n_batches is None:
            return gen.randint(0, hi, size=batch_size)
        return np.stack([gen.randint(0, hi, size=batch_size) for _ in range(n_batches)])

    def sample(self, batch_size: int, indices=None):
        if indices is None:
            indices = torch.from_numpy(self.draw_indices(batch_size)).to(self._dev)
        return super().sample(batch_size, indices)


class ImplicitQLearning(_OfflineIQL):
    """cref:438-556 on the same kernels: no autocast, convex Polyak form, the scheduler handed in."""

    def __init__(self, max_action, actor, actor_optimizer, actor_lr_scheduler, q_network, q_optimizer,
                 v_network, v_optimizer, iql_tau: float = 0.7, beta: float = 3.0, gamma: float = 0.99,
                 tau: float = 0.005, device: str = "cpu", *, seed: Optional[int] = None,
                 keep_grads: bool = False):
        super().__init__(max_action, actor, actor_optimizer, q_network, q_optimizer, v_network, v_optimizer,
                         iql_tau=iql_tau, beta=beta, max_steps=int(actor_lr_scheduler.T_max), discount=gamma,
                         tau=tau, device=device, precision="fp32", seed=seed, keep_grads=keep_grads,
                         polyak_form=1)
        self.actor_lr_scheduler = self.actor_lr_schedule = actor_lr_scheduler
        self.gamma = gamma

    def train_on_buffer(self, replay_buffer: ReplayBuffer, n_steps: int, batch_size: int, *,
                        sampler: str = "host", rng=None):
        """``n_steps`` x (sample with numpy's generator, train) in one library call.  ``sampler``:
        "host" draws the indices with numpy and uploads them, "device" draws the same indices with
        ``NumpyIndexStream``; both leave the generator (``rng``, default numpy's global one) in the
        same state.  Returns the [n_steps, 3] device loss tensor."""
        if sampler == "host":
            idx = torch.from_numpy(replay_buffer.draw_indices(batch_size, n_steps, rng=rng)).to(self._dev)
        elif sampler == "device":
            if getattr(self, "_index_stream", None) is None:
                self._index_stream = NumpyIndexStream(self.device)
            idx = self._index_stream.draw(replay_buffer.index_bound(), n_steps, batch_size, [rng])[0]
        else:
            raise ValueError("sampler must be 'host' or 'device'")
        return self.train_steps(replay_buffer, n_steps, batch_size, indices=idx)

    def state_dict(self) -> Dict[str, Any]:
        sd = super().state_dict()
        sd["actor_lr_scheduler"] = sd.pop("actor_lr_schedule")
        sd.pop("total_it")
        return sd  # cref:546-556

    def load_state_dict(self, state_dict: Dict[str, Any]):
        sd = dict(state_dict)
        sd["actor_lr_schedule"] = sd.pop("actor_lr_scheduler")
        sd.setdefault("total_it", int(sd["actor_lr_schedule"]["last_epoch"]))
        super().load_state_dict(sd)


# --------------------------------------------------------------------------- #
# train (cref:597-749)
# --------------------------------------------------------------------------- #
def _reward_model_missing(where: str, config, advice: str, readers: str):
    """``where`` got ``reward_model=None``: the reference would read an Orbax checkpoint with ``readers``,
    which are not built here.  ``advice``: what to pass instead."""
    try:
        import orbax.checkpoint  # noqa: F401
    except ImportError:
        raise ImportError(
            f"{where}: reward_model=None would read the Orbax checkpoint {config.reward_model_path!r}, "
            f"but orbax is not installed (and iqlpref_amd has no Orbax reader); pass reward_model= {advice}") from None
    raise NotImplementedError(
        f"{where}: iqlpref_amd has no Orbax checkpoint reader ({readers}); pass reward_model= {advice}")


def _minari():
    try:
        import minari
    except ImportError:
        raise ImportError("custom_offline.train: dataset=None loads the Minari dataset config.dataset_id, but "
                          "minari is not installed; pass dataset= (iterable of episodes) and eval_env=") from None
    return minari


def _build_trainer(config, seed: int, state_dim: int, action_dim: int, limits: Sequence, device: str,
                   policies=(GaussianPolicy, DeterministicPolicy), trainer_cls=ImplicitQLearning):
    """cref:655-689 for one seed: the nets are built right after ``torch.manual_seed(seed)`` on the
    CPU generator (in cref's order), then moved to the device.  ``limits``: the action limits that the
    policy and the trainer take ahead of their other arguments -- ``(max_action,)`` here, ``(max_actions,
    min_actions)`` for the BB flavour, which also hands in its own ``policies`` (Gaussian, deterministic)
    and ``trainer_cls``."""
    torch.manual_seed(seed)
    q_network = TwinQ(state_dim, action_dim).to(device)
    v_network = ValueFunction(state_dim).to(device)
    pol = policies[1] if config.iql_deterministic else policies[0]
    actor = pol(state_dim, action_dim, *limits, dropout=config.actor_dropout).to(device)
    v_optimizer = torch.optim.Adam(v_network.parameters(), lr=config.vf_lr)
    q_optimizer = torch.optim.Adam(q_network.parameters(), lr=config.qf_lr)
    actor_optimizer = torch.optim.Adam(actor.parameters(), lr=config.actor_lr)
    actor_lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(actor_optimizer, config.update_steps)
    return trainer_cls(
        *limits, actor=actor, actor_optimizer=actor_optimizer, actor_lr_scheduler=actor_lr_scheduler,
        q_network=q_network, q_optimizer=q_optimizer, v_network=v_network, v_optimizer=v_optimizer,
        iql_tau=config.iql_tau, beta=config.beta, gamma=config.gamma, tau=config.tau, device=device, seed=seed)


def train(config: TrainConfig, dataset=None, reward_model=None, eval_env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None,
          normalized_score: Optional[Callable] = None, seeds_per_gpu: int = 1, sampler: str = "device",
          device: Optional[str] = None, chunk: int = 2000):
    """cref:597-749 on the fused HIP step.

    ``dataset``: an iterable of Minari-style episodes (``observations``, ``actions``,
    ``terminations``); None loads ``config.dataset_id`` with minari.  ``eval_env``: a gymnasium-API
    environment (default: ``dataset.recover_environment()``).  ``reward_model``: a ``QMLP``
    (``query_length == 1``) or ``RewardPT`` holding its parameters; the Orbax checkpoint at
    ``reward_model_path`` cannot be read here.  ``logger(record, step)``: one call per ``wandb.log``
    of cref (default: wandb when importable, else print).  ``normalized_score(dataset, returns)``:
    default ``minari.get_normalized_score``; a ``ValueError`` from it keeps the raw mean return, as
    cref's ``contextlib.suppress`` does.  ``sampler``: "device" (``NumpyIndexStream``) or "host"
    (numpy); both give the same indices and the same final generator state.

    The steps run in chunks of at most ``chunk`` that end on evaluation boundaries; the losses of a
    chunk come back to the host once, after the next chunk has been queued (``_offline_loop.run``).

    ``seeds_per_gpu`` = K > 1: seed k is ``train_seed + rank K + k``, with its own nets (built right
    after ``torch.manual_seed(seed)``), its own ``np.random.RandomState(seed)`` index stream (the
    stream ``np.random.seed(seed)`` gives), its own checkpoints under ``seed_<seed>/`` and a ``seed``
    entry in its logger records; all K share one buffer and step as one ``SeedGroup`` with the
    indices of one K-stream draw.  Every seed is bit-identical to ``train()`` of that seed alone.
    Returns the trainer (K = 1) or the list of K trainers."""
    relabel = None
    if reward_model is not None:
        relabel = lambda ds: qlearning_dataset(ds, reward_model, config.query_length)
    return _train(config, dataset, eval_env, relabel, False, logger=logger, normalized_score=normalized_score,
                  seeds_per_gpu=seeds_per_gpu, sampler=sampler, device=device, chunk=chunk)


def _train(config, dataset, eval_env, relabel: Optional[Callable], best_by_return: bool, *, logger=None,
           normalized_score=None, seeds_per_gpu: int = 1, sampler: str = "device", device=None, chunk: int = 2000):
    """``train()`` with the two things a flavour chooses: ``relabel(dataset)`` builds the transition dict
    (None: there is no reward model to build it with, which is reported after the other argument checks), and
    ``best_by_return`` keeps the best model by the mean evaluation return even when a normalized score is
    logged (``custom_offline_br``)."""
    if sampler not in ("host", "device"):
        raise ValueError("sampler must be 'host' or 'device'")
    K = int(seeds_per_gpu)
    if not 1 <= K <= _lib.MAX_GROUP:
        raise ValueError(f"seeds_per_gpu must be in 1..{_lib.MAX_GROUP}")
    if device is None:
        device = D.local_device() or "cuda:0"
    minari = None
    if dataset is None:
        minari = _minari()
        dataset = minari.load_dataset(config.dataset_id)
    if eval_env is None:
        if not hasattr(dataset, "recover_environment"):
            raise ValueError("custom_offline.train: pass eval_env= (the dataset cannot recover_environment())")
        eval_env = dataset.recover_environment()
    if normalized_score is None:
        try:
            minari = minari or _minari()
            normalized_score = minari.get_normalized_score
        except ImportError:
            normalized_score = None
    if relabel is None:
        _reward_model_missing("custom_offline.train", config,
                              "a QMLP or RewardPT holding its parameters (load_flax_params)", "load_QMLP / load_PT")
    state_dim = eval_env.observation_space.shape[0]
    action_dim = eval_env.action_space.shape[0]
    max_action = float(eval_env.action_space.high[0])

    # ---- dataset, normalisation, buffer (cref:631-653) ----
    qdataset = relabel(dataset)
    if config.normalize_reward:
        modify_reward(qdataset, config.dataset_id)
    if config.normalize_state:
        state_mean, state_std = compute_mean_std(qdataset["observations"], eps=1e-3)
    else:
        state_mean, state_std = 0, 1
    qdataset["observations"] = normalize_states(qdataset["observations"], state_mean, state_std)
    qdataset["next_observations"] = normalize_states(qdataset["next_observations"], state_mean, state_std)
    from .train import _NormalizedEnv
    eval_env = _NormalizedEnv(eval_env, state_mean, state_std, 1.0)  # cref wrap_env, reward_scale 1
    replay_buffer = ReplayBuffer(state_dim, action_dim, config.buffer_size, device)
    replay_buffer.load_dataset(qdataset)

    seeds = [D.rank_seed(config.train_seed, K) + k for k in range(K)]
    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)

    # ---- seeds and nets (cref:659-689) ----
    set_seed(seeds[0])  # np, random, torch, PYTHONHASHSEED
    gens = [None] if K == 1 else [np.random.RandomState(s) for s in seeds]  # None: numpy's global generator
    trainers = [_build_trainer(config, s, state_dim, action_dim, (max_action,), device) for s in seeds]
    group = None
    if K > 1:
        from .multi import SeedGroup
        group = SeedGroup(trainers)
    stream = NumpyIndexStream(device) if sampler == "device" else None
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    def steps(t, n):
        if stream is not None:
            idx = stream.draw(replay_buffer.index_bound(), n, config.batch_size, gens)
        else:
            idx = [torch.from_numpy(replay_buffer.draw_indices(config.batch_size, n, rng=g)).to(trainers[0]._dev)
                   for g in gens]
        if group is None:
            return [trainers[0].train_steps(replay_buffer, n, config.batch_size, indices=idx[0])]
        return group.train_steps(replay_buffer, n, config.batch_size, indices=idx, return_losses=True)

    _offline_loop.run(
        trainers, seeds, group, int(config.update_steps), int(config.eval_every), chunk, logger, ckpt_dirs, steps,
        evaluate=lambda k, trainer, step: evaluate(eval_env, trainer.actor, config.eval_episodes, config.eval_seed,
                                                   device),
        normalized=None if normalized_score is None else (lambda scores: normalized_score(dataset, scores)),
        best_by_return=best_by_return)
    if group is not None:
        group.synchronize()
        group.close()
        return trainers
    return trainers[0]
