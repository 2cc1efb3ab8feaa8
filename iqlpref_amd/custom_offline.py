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

``train_runs()`` trains a list of configs -- the runs of a pen sweep grid, which differ in the reward
model and not in the seed -- each exactly as ``train()`` would train it alone, packed into seed groups:
one relabel per distinct reward model, one device buffer per distinct preparation, one K-stream index draw
and one group step per library call (``iqlpref_amd.sweep`` is the command line over it).

Reward models travel as plain ``.npz`` files (``save_reward_params`` / ``load_reward_model``): the flax
parameter tree as numpy arrays plus the constructor arguments, written on a machine that has jax.  A
``reward_model_path`` that ends in ``.npz``, or has such a file beside it (``best_model.ckpt.npz``), is
read from there when no model is handed in.

Not built (stated): the Orbax / flax-nnx checkpoint readers ``load_PT`` / ``load_QMLP``
(reward_models/pref_transformer.py:280-327, q_mlp.py:100-168) need orbax + jax, which are absent;
``load_pt_flax_params`` / ``QMLP.load_flax_params`` take the parameter pytree as numpy
arrays instead, and the ``.npz`` interchange above carries it between machines.  PT numerics stay "parity unpinned" (no runnable reference, no fixtures).
"""
import ctypes as C
import json
import uuid
import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _offline_loop, _resume
from . import distributed as D
from ._lib import check, ptr
from .iql import DeterministicPolicy, GaussianPolicy, TwinQ, ValueFunction, compute_mean_std, normalize_states, set_seed
from .iql import ImplicitQLearning as _OfflineIQL
from .iql import ReplayBuffer as _OfflineReplayBuffer
from .iql import load_config_for, mlp_forward_f32
from .multi import stepper
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


def load_config(config_path: Optional[str] = None, **overrides) -> TrainConfig:
    """The pyrallis ``--config_path`` behaviour (cref:597) with ``iql.load_config``'s rules."""
    return load_config_for(TrainConfig, "custom_offline.TrainConfig", config_path, **overrides)


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
# reward models as .npz files (the interchange that stands in for the Orbax readers)
# --------------------------------------------------------------------------- #
REWARD_KINDS = ("qmlp", "pt")
_META = "__meta__"


def _flatten_params(node, prefix: str, out: Dict[str, np.ndarray]):
    items = node.items() if isinstance(node, Mapping) else enumerate(node)
    for k, v in items:
        name = f"{prefix}/{k}" if prefix else str(k)
        if "/" in str(k) or name == _META:
            raise ValueError(f"parameter key {k!r} cannot be stored")
        if isinstance(v, (Mapping, list, tuple)):
            _flatten_params(v, name, out)
        else:
            out[name] = np.asarray(v)


def save_reward_params(path, kind: str, params, **ctor) -> str:
    """Write a reward model as one ``.npz`` file that ``load_reward_model`` reads.

    ``kind``: "qmlp" (``params``: the layers ``QMLP.load_flax_params`` takes, [{"kernel", "bias"}, ...]) or
    "pt" (``params``: the flax-nnx tree ``load_pt_flax_params`` takes).  The arrays go in under ``/``-joined
    keys (``0/kernel``, ``gpt/layers/0/attention/in_linear/kernel``); the one entry ``__meta__`` is a JSON
    string {"kind": ..., "ctor": {...}} with the constructor arguments besides the dims (qmlp:
    ``hidden_dims``, ``activations``, ``activation_final``; pt: ``max_episode_steps``, ``embd_dim``, ...).
    The file is written at ``path`` exactly (no suffix is appended).  Returns the path."""
    if kind not in REWARD_KINDS:
        raise ValueError(f"kind must be among {REWARD_KINDS}")
    arrays: Dict[str, np.ndarray] = {}
    _flatten_params(params, "", arrays)
    if not arrays:
        raise ValueError("no parameters to write")
    meta = json.dumps({"kind": kind, "ctor": ctor})
    path = os.fspath(path)
    with open(path, "wb") as f:
        np.savez(f, **{_META: np.asarray(meta)}, **arrays)
    return path


def _read_reward_file(path) -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """(meta, parameter tree) of a ``save_reward_params`` file."""
    with np.load(os.fspath(path), allow_pickle=False) as z:
        if _META not in z.files:
            raise ValueError(f"{path}: no {_META} entry (not written by save_reward_params)")
        meta = json.loads(str(z[_META]))
        tree: Dict[str, Any] = {}
        for name in z.files:
            if name == _META:
                continue
            node = tree
            *parents, leaf = name.split("/")
            for part in parents:
                node = node.setdefault(part, {})
            node[leaf] = z[name]
    if meta.get("kind") not in REWARD_KINDS:
        raise ValueError(f"{path}: kind {meta.get('kind')!r} is not among {REWARD_KINDS}")
    return meta, tree


def load_reward_model(path, state_dim: int, action_dim: int, device):
    """The ``QMLP`` or ``RewardPT`` of a ``save_reward_params`` file, on ``device``."""
    meta, tree = _read_reward_file(path)
    ctor = dict(meta.get("ctor") or {})
    if meta["kind"] == "qmlp":
        layers = [tree[k] for k in sorted(tree, key=int)]
        ctor.setdefault("hidden_dims", [int(l["kernel"].shape[1]) for l in layers[:-1]])
        ctor["hidden_dims"] = tuple(int(h) for h in ctor["hidden_dims"])
        return QMLP(state_dim, action_dim, **ctor).load_flax_params(layers).to(device)
    if "max_episode_steps" not in ctor:
        ctor["max_episode_steps"] = int(tree["timestep_embed"]["embedding"].shape[0]) - 1
    return load_pt_flax_params(RewardPT(state_dim, action_dim, **ctor), tree).to(device)


def reward_model_file(reward_model_path: str) -> Optional[str]:
    """The ``.npz`` file a ``reward_model_path`` is read from when no model is handed in: the path itself
    when it ends in ``.npz``, else ``<path>.npz`` when that exists (``best_model.ckpt`` ->
    ``best_model.ckpt.npz``), else None."""
    p = os.path.expanduser(str(reward_model_path))
    if p.endswith(".npz"):
        return p
    return p + ".npz" if os.path.isfile(p + ".npz") else None


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


def generator_state(gen=None) -> Dict[str, Any]:
    """The state of an ``np.random.RandomState`` (None: numpy's global generator) as a resume generation
    stores it: the MT19937 key as an int64 tensor, the position and the cached gaussian."""
    st = (np.random if gen is None else gen).get_state(legacy=True)
    if st[0] != "MT19937":
        raise ValueError(f"not a legacy MT19937 state: {st[0]!r}")
    return {"key": torch.from_numpy(np.asarray(st[1]).astype(np.int64)), "pos": int(st[2]), "has_gauss": int(st[3]),
            "cached_gaussian": float(st[4])}


def set_generator_state(gen, state: Mapping[str, Any]) -> None:
    """Put a generator (None: numpy's global one) where ``generator_state`` found it."""
    (np.random if gen is None else gen).set_state(
        ("MT19937", state["key"].numpy().astype(np.uint32), int(state["pos"]), int(state["has_gauss"]),
         float(state["cached_gaussian"])))


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
    npz = (f", or export the parameters with custom_offline.save_reward_params to "
           f"{os.path.expanduser(str(config.reward_model_path))}.npz (INTEGRATION.md)")
    try:
        import orbax.checkpoint  # noqa: F401
    except ImportError:
        raise ImportError(
            f"{where}: reward_model=None would read the Orbax checkpoint {config.reward_model_path!r}, "
            f"but orbax is not installed (and iqlpref_amd has no Orbax reader); pass reward_model= {advice}{npz}") from None
    raise NotImplementedError(
        f"{where}: iqlpref_amd has no Orbax checkpoint reader ({readers}); pass reward_model= {advice}{npz}")


def _minari(where: str = "custom_offline.train"):
    try:
        import minari
    except ImportError:
        raise ImportError(f"{where}: dataset=None loads the Minari dataset config.dataset_id, but "
                          "minari is not installed; pass dataset= (iterable of episodes) and eval_env=") from None
    return minari


def _minari_score(minari=None):
    """``minari.get_normalized_score`` (of the module, where a caller has imported it), or None without minari."""
    try:
        return (minari or _minari()).get_normalized_score
    except ImportError:
        return None


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


def _prepare(config, qdataset: Dict[str, np.ndarray], eval_env, state_dim: int, action_dim: int, device):
    """cref:631-653: the relabelled transitions (rewritten in place) -> the device buffer and the evaluation
    environment that normalises its observations with the same mean / std."""
    if getattr(config, "normalize_reward", False):  # (``minari_bc``'s config has no such field)
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
    return replay_buffer, eval_env


def _minari_setup(where: str, config, dataset, eval_env, normalized_score):
    """The Minari arguments of a ``train()`` with their defaults filled in: ``(dataset, eval_env, normalized_score,
    state_dim, action_dim, max_action)``.  ``where``: the caller's name in the messages."""
    minari = None
    if dataset is None:
        minari = _minari(where)
        dataset = minari.load_dataset(config.dataset_id)
    if eval_env is None:
        if not hasattr(dataset, "recover_environment"):
            raise ValueError(f"{where}: pass eval_env= (the dataset cannot recover_environment())")
        eval_env = dataset.recover_environment()
    if normalized_score is None:
        normalized_score = _minari_score(minari)
    return (dataset, eval_env, normalized_score, eval_env.observation_space.shape[0], eval_env.action_space.shape[0],
            float(eval_env.action_space.high[0]))


def _index_sources(seeds: Sequence[int], sampler: str, device):
    """Where the members' indices come from: ``(gens, stream)`` -- one ``np.random.RandomState(seed)`` per seed
    (one seed alone: None, numpy's global generator, which ``set_seed`` has seeded) and the ``NumpyIndexStream``
    that draws from them on the device (None: ``sampler="host"``)."""
    gens = [None] if len(seeds) == 1 else [np.random.RandomState(s) for s in seeds]
    return gens, NumpyIndexStream(device) if sampler == "device" else None


def _steps(stream, trainers, bufs, gens, B: int):
    """The ``steps(group, active, t, n)`` of ``_offline_loop.run``: member k steps on indices below the bound of
    ``bufs[k]`` from ``gens[k]``, drawn in ONE ``NumpyIndexStream`` launch for all, or on the host (``stream`` None)."""
    def steps(group, act, t, n):
        if stream is not None:
            idx = stream.draw([bufs[k].index_bound() for k in act], n, B, [gens[k] for k in act])
        else:
            idx = [torch.from_numpy(bufs[k].draw_indices(B, n, rng=gens[k])).to(trainers[k]._dev) for k in act]
        return group.train_steps([bufs[k] for k in act], n, B, indices=idx, return_losses=True)
    return steps


def train(config: TrainConfig, dataset=None, reward_model=None, eval_env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None,
          normalized_score: Optional[Callable] = None, seeds_per_gpu: int = 1, sampler: str = "device",
          device: Optional[str] = None, chunk: int = 2000, resume: bool = False):
    """cref:597-749 on the fused HIP step.

    ``dataset``: an iterable of Minari-style episodes (``observations``, ``actions``,
    ``terminations``); None loads ``config.dataset_id`` with minari.  ``eval_env``: a gymnasium-API
    environment (default: ``dataset.recover_environment()``).  ``reward_model``: a ``QMLP``
    (``query_length == 1``) or ``RewardPT`` holding its parameters; the Orbax checkpoint at
    ``reward_model_path`` cannot be read here; with None the model is read from the ``.npz`` file
    ``reward_model_file(config.reward_model_path)`` names (``save_reward_params``).  ``logger(record, step)``: one call per ``wandb.log``
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
    Returns the trainer (K = 1) or the list of K trainers.

    ``resume`` (needs ``checkpoints_path``, and the ``config.yaml`` there, if any, must have been written for
    the same config, paths aside; ValueError otherwise): at the end of every evaluation boundary every seed
    writes ``resume_{t}.pt`` into its checkpoint directory -- its trainer's ``resume_state()`` (with the target
    critics and the dropout counters), the state of its numpy generator (which stands exactly after the
    draws of step t: a chunk draws the steps it queues and ends on the boundary) and its best score / step and
    kept normalized score -- and the run starts from the newest complete generation instead of step 0
    (``_offline_loop.run``).  A run killed at any moment and started again with the same arguments logs the
    records and writes the files of the uninterrupted run from there on and returns the same trainers, bit for
    bit; the generators end where the uninterrupted run's end.  The dataset, the reward model and the
    evaluation environment must be the same again; an environment that keeps state of its own from one
    evaluation to the next is outside the contract.  ``custom_offline_br`` and ``custom_offline_bb`` do not
    resume (their relabel draws and block permutations come from global generators ahead of the loop)."""
    relabel = None
    if reward_model is not None:
        relabel = lambda ds: qlearning_dataset(ds, reward_model, config.query_length)
    return _train(config, dataset, eval_env, relabel, False, logger=logger, normalized_score=normalized_score,
                  seeds_per_gpu=seeds_per_gpu, sampler=sampler, device=device, chunk=chunk, resume=resume,
                  model_file=None if reward_model is not None else reward_model_file(config.reward_model_path))


def _train(config, dataset, eval_env, relabel: Optional[Callable], best_by_return: bool, *, logger=None,
           normalized_score=None, seeds_per_gpu: int = 1, sampler: str = "device", device=None, chunk: int = 2000,
           model_file: Optional[str] = None, resume: bool = False, where: str = "custom_offline.train"):
    """``train()`` with the two things a flavour chooses: ``relabel(dataset)`` builds the transition dict
    (None: there is no reward model to build it with, which is reported after the other argument checks --
    unless ``model_file`` names a ``save_reward_params`` file, read once the dims and the device are known),
    and ``best_by_return`` keeps the best model by the mean evaluation return even when a normalized score is
    logged (``custom_offline_br``).  A flavour without a reward model (``minari_iql``: the dataset's own
    rewards) always hands in a ``relabel``.  ``where``: the caller's name in the messages."""
    _offline_loop.check_sampler(sampler)
    seeds = _offline_loop.group_seeds(config.train_seed, seeds_per_gpu)
    K = len(seeds)
    if resume:
        _resume.check_config(config)
    if device is None:
        device = D.local_device() or "cuda:0"
    dataset, eval_env, normalized_score, state_dim, action_dim, max_action = _minari_setup(
        where, config, dataset, eval_env, normalized_score)
    if relabel is None and model_file is None:
        _reward_model_missing(where, config,
                              "a QMLP or RewardPT holding its parameters (load_flax_params)", "load_QMLP / load_PT")
    if relabel is None:
        file_model = load_reward_model(model_file, state_dim, action_dim, device)
        relabel = lambda ds: qlearning_dataset(ds, file_model, config.query_length)

    replay_buffer, eval_env = _prepare(config, relabel(dataset), eval_env, state_dim, action_dim, device)

    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds, resume=resume)

    # ---- seeds and nets (cref:659-689) ----
    set_seed(seeds[0])  # np, random, torch, PYTHONHASHSEED
    trainers = [_build_trainer(config, s, state_dim, action_dim, (max_action,), device) for s in seeds]
    gens, stream = _index_sources(seeds, sampler, device)
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    normalized = None if normalized_score is None else (lambda scores: normalized_score(dataset, scores))
    _offline_loop.run(
        trainers, seeds, lambda active: stepper(trainers), int(config.update_steps), int(config.eval_every), chunk,
        logger, ckpt_dirs, _steps(stream, trainers, [replay_buffer] * K, gens, config.batch_size),
        lambda k, trainer, step: evaluate(eval_env, trainer.actor, config.eval_episodes, config.eval_seed, device),
        _offline_loop.BestModelRecords(ckpt_dirs, normalized, best_by_return), resume=resume,
        sampler_state=lambda k: generator_state(gens[k]),
        set_sampler_state=lambda k, st: set_generator_state(gens[k], st))
    return trainers if K > 1 else trainers[0]


# --------------------------------------------------------------------------- #
# sweep grids: runs of different configs as seed groups
# --------------------------------------------------------------------------- #
def shape_key(config: TrainConfig, dims, device: str = "cuda") -> tuple:
    """What the runs of one launch batch must share: state / action dims, batch size, policy kind, actor
    dropout on/off and the device (the nets of this flavour are always 2 x 256, fp32, two critics).
    ``dims`` = (S, A), or None when unknown (the dataset id stands in)."""
    dims_key = tuple(int(d) for d in dims) if dims is not None else ("dataset", config.dataset_id)
    return (dims_key, int(config.batch_size), bool(config.iql_deterministic), bool(config.actor_dropout), str(device))


def plan_batches(configs: Sequence[TrainConfig], dims: Sequence, runs_per_gpu: int = 8,
                 device: str = "cuda") -> List[List[int]]:
    """``sweep.plan_batches`` with this flavour's ``shape_key``: launch batches as lists of config indices,
    filled greedily in config order.  ``dims``: one (S, A) or None per config."""
    from .sweep import plan_batches as plan
    return plan(configs, list(dims), runs_per_gpu, key=lambda cfg, d: shape_key(cfg, d, device))


def _relabel_key(config: TrainConfig) -> tuple:
    return (config.dataset_id, config.reward_model_path, int(config.query_length))


def _buffer_key(config: TrainConfig) -> tuple:
    return (_relabel_key(config), bool(config.normalize_reward), bool(config.normalize_state), int(config.buffer_size))


def _model_sources(configs: Sequence[TrainConfig], reward_models) -> Dict[tuple, Any]:
    """Relabel key -> where the run's reward model comes from: the model itself (found in the mapping under
    the path as written or expanded), ("file", path) for a ``save_reward_params`` file, or ("call",) for a
    callable ``reward_models``.  No device work; raises for the paths that have no model and for a
    ``query_length > 1`` whose model is known not to be a ``RewardPT``."""
    sources: Dict[tuple, Any] = {}
    missing, not_pt = [], []
    for cfg in configs:
        key = _relabel_key(cfg)
        if key in sources:
            continue
        path = str(cfg.reward_model_path)
        src, kind = None, None
        if callable(reward_models) and not isinstance(reward_models, Mapping):
            src = ("call",)
        else:
            for name in (path, os.path.expanduser(path)):
                if reward_models is not None and name in reward_models:
                    src = reward_models[name]
                    kind = "pt" if isinstance(src, RewardPT) else "other"
                    break
            if src is None:
                f = reward_model_file(path)
                if f is not None and os.path.isfile(f):
                    src, kind = ("file", f), _read_reward_file(f)[0]["kind"]
        if src is None:
            if path not in missing:
                missing.append(path)
            continue
        if int(cfg.query_length) > 1 and kind not in (None, "pt"):
            not_pt.append(path)
        sources[key] = src
    if missing:
        raise ValueError(
            "custom_offline.train_runs: no reward model for reward_model_path " + ", ".join(repr(m) for m in missing) +
            "; hand them in with reward_models= (a mapping path -> QMLP | RewardPT, or a callable config -> model) or "
            "export each with custom_offline.save_reward_params to <path>.npz (iqlpref_amd has no Orbax reader)")
    if not_pt:
        raise TypeError("query_length > 1 needs an iqlpref_amd RewardPT; not one: " + ", ".join(repr(m) for m in not_pt))
    return sources


def _per_id(given, ids: Sequence[str], what: str) -> Dict[str, Any]:
    """``given`` -- one object for every dataset id, or a mapping id -> object -- as a dict over ``ids``."""
    if not isinstance(given, Mapping):
        return {d: given for d in ids}
    lacking = [d for d in ids if d not in given]
    if lacking:
        raise ValueError(f"no {what} given for {', '.join(lacking)}")
    return {d: given[d] for d in ids}


def train_runs(configs: Sequence[TrainConfig], dataset=None, reward_models=None, eval_env=None, *,
               runs_per_gpu: int = 8, logger: Optional[Callable[[Dict[str, float], int], None]] = None,
               normalized_score: Optional[Callable] = None, sampler: str = "device", chunk: int = 2000,
               run_ids: Optional[Sequence[int]] = None, resume: bool = False) -> List[ImplicitQLearning]:
    """Train every config exactly as ``train(config, ...)`` would train it alone -- the same logged records
    (each with a ``run`` entry besides), evaluations (own actor, ``eval_seed``, ``eval_episodes``, the
    best-model rule of ``_offline_loop.BestModelRecords``), files under the run's own ``checkpoints_path``
    (``config.yaml``, ``checkpoint_{step}.pt``, ``best_model.pt``) and final parameters, target, Adam
    moments and actor learning rate, bit for bit -- with the runs packed into seed groups.

    Launch batches (``plan_batches``): runs of one ``shape_key`` (dims, ``batch_size``,
    ``iql_deterministic``, actor dropout on/off, device), at most ``runs_per_gpu`` (1..16) in config order,
    one batch after another.  Inside a batch everything else may differ: the reward model, the dataset when
    its dims match, ``train_seed`` / ``eval_seed`` / ``eval_episodes``, ``gamma``, ``tau``, ``beta``,
    ``iql_tau``, the learning rates, the dropout rate, ``normalize_reward`` / ``normalize_state``,
    ``update_steps`` and ``eval_every``.  All runs of a batch start at step 0; every library call runs to
    the next chunk, evaluation or end boundary of ANY active run; a finished run leaves and the group is
    rebuilt over the rest.  A batch of one run steps its trainer directly, with no ``SeedGroup``.

    Shared work: the dataset is relabelled once per distinct (``dataset_id``, ``reward_model_path``,
    ``query_length``), and one device buffer -- with its state mean / std and its normalising evaluation
    environment -- is built per distinct (that key, ``normalize_reward``, ``normalize_state``,
    ``buffer_size``); both are dropped after the last batch that uses them.  Per run: nets built right after
    ``torch.manual_seed(train_seed)``, an ``np.random.RandomState(train_seed)`` index stream of its own
    (two runs of one seed draw the same indices, as they would alone) below the bound of its own buffer.

    ``dataset``: one re-iterable of episodes for every run, a mapping ``dataset_id -> iterable``, or None
    (one ``minari.load_dataset`` per distinct id).  ``eval_env``: one environment, a mapping
    ``dataset_id -> env``, or None (``recover_environment()``).  ``reward_models``: a mapping
    ``reward_model_path -> QMLP | RewardPT`` (paths matched as the config writes them and after
    ``expanduser``) or a callable ``config -> model`` (called once per distinct relabel); a path that has no
    entry, and every path with None, is read from its ``.npz`` file (``reward_model_file``).
    ``logger(record, step)``: default one wandb run per process with keys ``run<r>/``, or print.
    ``run_ids``: the names of the runs in the records (default 0 .. n-1).

    Before any device work: ``runs_per_gpu`` in range, no two runs with one ``checkpoints_path``, a reward
    model for every run (the error names the paths without), a ``RewardPT`` where ``query_length > 1``.

    numpy's global generator is no part of this function's contract: ``train()`` alone draws its indices
    from it (and leaves it advanced); ``train_runs`` draws the same numbers from per-run generators and
    neither seeds nor reads the global one.

    ``resume`` (a ``checkpoints_path`` for every config, and the ``config.yaml`` there, if any, written for the
    same config, paths aside; ValueError otherwise, before any device work): as in ``train()``, per launch
    batch (``_offline_loop.run``).  At the end of every boundary at which a run of the batch evaluated or
    ended, every run active in it, due or not, writes ``resume_{t}.pt`` at the common step (trainer
    ``resume_state()``, the state of its own generator, best score / step, kept normalized score, whether it
    has ended); a batch starts from its newest complete generation with the ended runs left out (their
    trainers loaded from their final state) and the group built over the others.  Each rank resumes its own runs.

    Under torchrun rank r trains the configs with index = r (mod world size), with no collectives.
    Returns this rank's trainers in config order."""
    from . import sweep as SW
    configs = list(configs)
    run_ids, mine = SW.start_runs(configs, runs_per_gpu, run_ids, resume)
    _offline_loop.check_sampler(sampler)
    sources = _model_sources(configs, reward_models)
    if not mine:
        return []
    device = D.local_device() or "cuda:0"

    # ---- datasets and environments of this rank's runs ----
    ids = list(dict.fromkeys(configs[i].dataset_id for i in mine))
    minari = None
    if dataset is None:
        minari = _minari()
        datasets = {d: minari.load_dataset(d) for d in ids}
    else:
        datasets = _per_id(dataset, ids, "dataset")
    if eval_env is not None:
        envs = _per_id(eval_env, ids, "eval_env")
    else:
        envs = {}
        for d in ids:
            if not hasattr(datasets[d], "recover_environment"):
                raise ValueError(f"custom_offline.train_runs: pass eval_env= (the dataset of {d} cannot "
                                 "recover_environment())")
            envs[d] = datasets[d].recover_environment()
    if normalized_score is None:
        normalized_score = _minari_score(minari)
    dims = {d: (envs[d].observation_space.shape[0], envs[d].action_space.shape[0]) for d in ids}
    local = plan_batches([configs[i] for i in mine], [dims[configs[i].dataset_id] for i in mine], runs_per_gpu, device)
    batches = [[mine[j] for j in b] for b in local]
    if logger is None:
        logger = SW._default_logger(configs, mine, run_ids)

    # ---- relabelled datasets and device buffers: built when a batch first needs them, dropped after their last ----
    relabelled = SW.BatchCache(batches, lambda i: _relabel_key(configs[i]))
    buffers = SW.BatchCache(batches, lambda i: _buffer_key(configs[i]))

    def relabel(i):
        cfg, src = configs[i], sources[relabelled.key_of[i]]
        if isinstance(src, tuple) and src[0] == "call":
            src = reward_models(cfg)
        elif isinstance(src, tuple) and src[0] == "file":
            src = load_reward_model(src[1], *dims[cfg.dataset_id], device)
        return qlearning_dataset(datasets[cfg.dataset_id], src, cfg.query_length)

    def prepare(i):
        cfg = configs[i]
        # (_prepare rewrites its dict, and the rewards in place: every preparation gets its own)
        qd = dict(relabelled.get(i, lambda: relabel(i)))
        qd["rewards"] = qd["rewards"].copy()
        return _prepare(cfg, qd, envs[cfg.dataset_id], *dims[cfg.dataset_id], device)

    stream = NumpyIndexStream(device) if sampler == "device" else None
    trainers: Dict[int, ImplicitQLearning] = {}
    for bi, batch in enumerate(batches):
        cfgs = [configs[i] for i in batch]
        bufs, batch_envs = zip(*[buffers.get(i, lambda: prepare(i)) for i in batch])
        ckpt_dirs = [_offline_loop.checkpoint_dirs(cfg, [cfg.train_seed], resume=resume)[0] for cfg in cfgs]
        for i, cfg in zip(batch, cfgs):
            high = float(envs[cfg.dataset_id].action_space.high[0])
            trainers[i] = _build_trainer(cfg, cfg.train_seed, *dims[cfg.dataset_id], (high,), device)
        trs = [trainers[i] for i in batch]
        gens = [np.random.RandomState(cfg.train_seed) for cfg in cfgs]
        normalized = [None if normalized_score is None else
                      (lambda scores, ds=datasets[cfg.dataset_id]: normalized_score(ds, scores)) for cfg in cfgs]
        # member k has its own buffer, bound, generator, step count and evaluation period (one alone: a ``Solo``)
        _offline_loop.run(
            trs, [cfg.train_seed for cfg in cfgs], lambda act: stepper([trs[k] for k in act]),
            [int(cfg.update_steps) for cfg in cfgs], [int(cfg.eval_every) for cfg in cfgs], chunk, logger, ckpt_dirs,
            _steps(stream, trs, bufs, gens, int(cfgs[0].batch_size)),
            lambda k, trainer, step: evaluate(batch_envs[k], trainer.actor, cfgs[k].eval_episodes, cfgs[k].eval_seed,
                                              device),
            _offline_loop.BestModelRecords(ckpt_dirs, normalized),
            tagged=lambda rec, k: dict(rec, run=run_ids[batch[k]]), resume=resume,
            sampler_state=lambda k: generator_state(gens[k]),
            set_sampler_state=lambda k, st: set_generator_state(gens[k], st))
        del bufs, batch_envs
        relabelled.batch_done(bi)
        buffers.batch_done(bi)
    return [trainers[i] for i in mine]
