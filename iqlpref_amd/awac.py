"""``algorithms/offline/awac.py`` ("awac"): offline AWAC, the D4RL baseline that is IQL's direct ancestor -- the
policy loss is IQL's advantage-weighted regression with ``V(s)`` replaced by ``min Q(s, pi(s))``.

The step is four launches of its own (csrc/awac_step.hip, ``iqlhip_awac_*``): fp32 (awac has no autocast), three
hidden layers of ``hidden_dim`` (a multiple of 16 in 16..256), ``state_dim`` <= 128, ``action_dim`` <= 32, any
batch size up to 65536, plain Adam, 1..16 members per group.  What is kept from awac, because it decides what a run
computes:

* ``update`` (awac:301-310) in its order: the critics against ``r + gamma (1 - d) min Q_target(s', a')`` with
  ``a' = clamp(mu(s') + sigma eps_1, -1, 1)`` from the actor as it stands, ``mse + mse`` (a sum, awac:282), both Adam
  steps; then the actor at the critics just updated, ``pi = clamp(mu(s) + sigma eps_2, -1, 1)``,
  ``w = min(exp((min Q(s, a) - min Q(s, pi)) / lambda), 100)``, ``mean(-w log_prob(a | s))`` into ``_mlp`` and
  ``_log_std``; then ``t <- (1 - tau) t + tau s`` (awac:215: two products and a sum);
* the two draws of standard normals per update, eps_1 then eps_2, each [B, A]: injected (``eps=``, ``noise=``) or
  drawn on the device from the trainer's Philox key (Box-Muller; include/iqlhip.h has the stream);
* indices come from ``np.random.randint(0, min(size, pointer), size=B)`` on numpy's global generator (awac:120),
  drawn on the host or by ``custom_offline.NumpyIndexStream``;
* ``modify_reward`` (awac:395-401) is NOT IQL's: locomotion rewards are scaled without the ``- 1``, antmaze
  rewards get ``- 1``;
* one ``{"critic_loss", "actor_loss"}`` record per step at ``step=t`` (zero-based), at ``(t + 1) % eval_frequency
  == 0`` an evaluation with the old gym API on the unclamped mean (``actor.eval()``, awac:360-377), an
  ``eval_score`` and -- where the environment has ``get_normalized_score`` -- a ``d4rl_normalized_score =
  (get_normalized_score(scores) * 100).mean()`` record, and ``checkpoint_{t}.pt`` holding the three-key state
  dict of awac:312-317 (no optimisers, no targets); there is no ``load_model``.

Not here: bf16, ``resume``, sweep files, ``posthoc``, ``algorithms/finetune/awac.py``, widths above 256, other depths.
"""
import ctypes as C
import os
import uuid
from copy import deepcopy
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _arena, _d4rl, _lib, _offline_loop
from . import custom_offline as _co
from ._d4rl import eval_actor  # noqa: F401  (awac:360-377: on the unclamped mean, ``Actor.act`` in eval mode)
from ._lib import check, ptr, stream_ptr
from .iql import load_config_for, compute_mean_std, normalize_states, set_seed, mlp_forward_f32  # noqa: F401
from .multi import ArenaGroup
from .train import wrap_env  # noqa: F401  (awac:348-357)

TensorBatch = List[torch.Tensor]
NETS = ("actor", "critic_1", "critic_2", "target_critic_1", "target_critic_2")
MAX_HIDDEN, MAX_STATE, MAX_ACTION = 256, 128, 32
LOSS_NAMES = ("critic_loss", "actor_loss")
EPS_SHAPE = "eps must be a float32 device tensor [n_steps, 2, batch_size, action_dim]"


@dataclass
class TrainConfig:
    """awac:21-70, same fields and defaults."""
    project: str = "CORL"
    group: str = "AWAC-D4RL"
    name: str = "AWAC"
    env_name: str = "halfcheetah-medium-expert-v2"
    hidden_dim: int = 256
    learning_rate: float = 3e-4
    gamma: float = 0.99
    tau: float = 5e-3
    awac_lambda: float = 1.0
    num_train_ops: int = 1_000_000
    batch_size: int = 256
    buffer_size: int = 2_000_000
    normalize_reward: bool = False
    eval_frequency: int = 1000
    n_test_episodes: int = 10
    checkpoints_path: Optional[str] = None
    deterministic_torch: bool = False
    seed: int = 42
    test_seed: int = 69
    device: str = "cuda"

    def __post_init__(self):
        self.name = f"{self.name}-{self.env_name}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)


def load_config(config_path: Optional[str] = None, **overrides) -> TrainConfig:
    """The pyrallis ``--config_path`` behaviour (awac:415) with ``iql.load_config``'s rules."""
    return load_config_for(TrainConfig, "awac.TrainConfig", config_path, **overrides)


class ReplayBuffer(_co.ReplayBuffer):
    """awac:73-131 on the packed device rows: ``load_d4rl_dataset`` (its two ``ValueError``s), ``sample`` on
    ``np.random.randint(0, min(size, pointer), size=B)`` of numpy's global generator (awac:120); ``add_transition``
    raises ``NotImplementedError`` (awac:128-131)."""


# --------------------------------------------------------------------------- #
# networks (awac:134-215)
# --------------------------------------------------------------------------- #
def _mlp(in_dim: int, hidden_dim: int, out_dim: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                         nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, out_dim))


def _linears(module: nn.Module) -> List[nn.Linear]:
    return [m for m in getattr(module, "_mlp", ()) if isinstance(m, nn.Linear)]


def _forward(module: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """``module._mlp(x)`` on the stand-alone exact-fp32 MFMA forward (``iqlhip_mlp_forward``)."""
    lin = _linears(module)
    return mlp_forward_f32([l.weight for l in lin], [l.bias for l in lin], x, w_in_out=False, hidden_act=0, out_act=0)


class Actor(nn.Module):
    """awac:134-187 (same attribute and state-dict names: ``_mlp.N.weight``, ``_log_std``)."""

    def __init__(self, state_dim: int, action_dim: int, hidden_dim: int, min_log_std: float = -20.0,
                 max_log_std: float = 2.0, min_action: float = -1.0, max_action: float = 1.0):
        super().__init__()
        self._mlp = _mlp(state_dim, hidden_dim, action_dim)
        self._log_std = nn.Parameter(torch.zeros(action_dim, dtype=torch.float32))
        self._min_log_std, self._max_log_std = min_log_std, max_log_std
        self._min_action, self._max_action = min_action, max_action

    def _get_policy(self, state: torch.Tensor) -> torch.distributions.Distribution:
        mean = _forward(self, state)
        log_std = self._log_std.detach().clamp(self._min_log_std, self._max_log_std)
        return torch.distributions.Normal(mean, log_std.exp())

    def log_prob(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        return self._get_policy(state).log_prob(action).sum(-1, keepdim=True)

    def forward(self, state: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        policy = self._get_policy(state)
        action = policy.rsample()
        action.clamp_(self._min_action, self._max_action)
        return action, policy.log_prob(action).sum(-1, keepdim=True)

    @torch.no_grad()
    def act(self, state: np.ndarray, device: str) -> np.ndarray:
        """awac:179-187: a sample in train mode, the (unclamped) mean in eval mode."""
        state_t = torch.tensor(state[None], dtype=torch.float32, device=device)
        policy = self._get_policy(state_t)
        action_t = policy.sample() if self._mlp.training else policy.mean
        return action_t[0].cpu().numpy()


class Critic(nn.Module):
    """awac:190-210."""

    def __init__(self, state_dim: int, action_dim: int, hidden_dim: int):
        super().__init__()
        self._mlp = _mlp(state_dim + action_dim, hidden_dim, 1)

    def forward(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        return _forward(self, torch.cat([state, action], dim=-1))


def soft_update(target: nn.Module, source: nn.Module, tau: float):
    """awac:213-215 (host-side helper; the training step fuses this into k_awac_critic_update)."""
    for target_param, source_param in zip(target.parameters(), source.parameters()):
        target_param.data.copy_((1 - tau) * target_param.data + tau * source_param.data)


def _net_dims(actor: nn.Module, critics: Sequence[nn.Module]) -> Tuple[int, int, int]:
    """(state_dim, action_dim, hidden_dim) of networks of awac's shape; TypeError for anything else,
    NotImplementedError for constants the kernels do not carry."""
    la = _linears(actor)
    if len(la) != 4 or not isinstance(getattr(actor, "_log_std", None), nn.Parameter):
        raise TypeError("actor must be an iqlpref_amd.awac.Actor (four Linear layers in _mlp, a _log_std parameter)")
    S, A, H = la[0].in_features, la[3].out_features, la[0].out_features
    nets = [la] + [_linears(c) for c in critics]
    for i, lin in enumerate(nets):
        if len(lin) != 4:
            raise TypeError("a critic must be an iqlpref_amd.awac.Critic (four Linear layers in _mlp)")
        want = [(S if i == 0 else S + A, H), (H, H), (H, H), (H, A if i == 0 else 1)]
        if [(l.in_features, l.out_features) for l in lin] != want or any(l.bias is None for l in lin):
            raise NotImplementedError("the AWAC step trains networks of three hidden layers of one width, the critics "
                                      "on cat(state, action) with one output")
    if tuple(actor._log_std.shape) != (A,):
        raise TypeError("_log_std must have one entry per action")
    consts = (actor._min_log_std, actor._max_log_std, actor._min_action, actor._max_action)
    if consts != (-20.0, 2.0, -1.0, 1.0):
        raise NotImplementedError(f"the kernels clamp log_std to [-20, 2] and actions to [-1, 1] (got {consts})")
    return S, A, H


def _config(state_dim: int, action_dim: int, hidden_dim: int, batch_size: int) -> _lib.TrainerConfig:
    c = _lib.TrainerConfig()
    c.state_dim, c.action_dim, c.hidden_dim, c.n_hidden = state_dim, action_dim, hidden_dim, 3
    c.batch_size, c.precision, c.dropout_p = batch_size, _lib.PREC_FP32, -1.0
    return c


def _layout(cfg: _lib.TrainerConfig):
    offs, n, nt = (C.c_int64 * 25)(), C.c_int64(), C.c_int64()
    check(_lib.load().iqlhip_awac_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n), C.byref(nt)))
    return list(offs), n.value, nt.value


def check_envelope(state_dim: int, action_dim: int, hidden_dim: int, batch_size: int = 16) -> None:
    """NotImplementedError (ValueError for a dim < 1) when the step's kernels are not built for the shape
    (include/iqlhip.h); touches no device."""
    _layout(_config(state_dim, action_dim, hidden_dim, batch_size))


# --------------------------------------------------------------------------- #
# trainer (awac:218-322)
# --------------------------------------------------------------------------- #
class AdvantageWeightedActorCritic(_arena.ArenaTrainer):
    """awac:218-322 on ``iqlhip_awac_*``.  The parameters of the three trained networks, their gradients
    (``keep_grads``) and Adam moments live in arenas the library borrows (``_arena``), the two deep-copied targets
    in a target arena; all stay the ``nn.Parameter`` objects they were, and each ``optimizer.state_dict()`` stays
    what ``torch.optim.Adam`` writes.  ``seed``: the Philox key of the action noise drawn on the device."""
    _ENTRY = "iqlhip_awac"

    def __init__(self, actor: nn.Module, actor_optimizer: torch.optim.Optimizer, critic_1: nn.Module,
                 critic_1_optimizer: torch.optim.Optimizer, critic_2: nn.Module,
                 critic_2_optimizer: torch.optim.Optimizer, gamma: float = 0.99, tau: float = 5e-3,
                 awac_lambda: float = 1.0, exp_adv_max: float = 100.0, *, seed: int = 0, keep_grads: bool = False):
        self._state_dim, self._action_dim, self._hidden = _net_dims(actor, (critic_1, critic_2))
        self._optimizers = (actor_optimizer, critic_1_optimizer, critic_2_optimizer)
        _arena.check_plain_adam(self._optimizers,
                                "the optimisers must be plain torch.optim.Adam (no weight decay / amsgrad / maximize)")
        groups = [o.param_groups[0] for o in self._optimizers]
        if len({(tuple(g["betas"]), g["eps"]) for g in groups}) != 1:
            raise NotImplementedError("the three optimisers share betas and eps (they may differ in lr)")
        check_envelope(self._state_dim, self._action_dim, self._hidden)  # (nothing is uploaded for a refused shape)
        params = [p for m in (actor, critic_1, critic_2) for p in m.parameters()]
        if any(p.device.type != "cuda" for p in params) or len({p.device for p in params}) != 1:
            raise ValueError("the networks must live on one GPU before construction")
        self._lib = _lib.load()
        self._dev = _lib.require_gpu(params[0].device)
        self._actor, self._actor_optimizer = actor, actor_optimizer
        self._critic_1, self._critic_1_optimizer = critic_1, critic_1_optimizer
        self._critic_2, self._critic_2_optimizer = critic_2, critic_2_optimizer
        self._target_critic_1, self._target_critic_2 = deepcopy(critic_1), deepcopy(critic_2)
        self._gamma, self._tau, self._awac_lambda, self._exp_adv_max = gamma, tau, awac_lambda, exp_adv_max
        self._seed, self._keep_grads = int(seed), keep_grads
        self.total_it = 0
        self._build_arenas()

    # -- arenas ------------------------------------------------------------- #
    @staticmethod
    def _tensors(module: nn.Module) -> List[torch.Tensor]:
        return [t for l in _linears(module) for t in (l.weight, l.bias)]

    def _cfg(self, batch_size: int) -> _lib.TrainerConfig:
        c = _config(self._state_dim, self._action_dim, self._hidden, batch_size)
        ga, g1, g2 = (o.param_groups[0] for o in self._optimizers)
        c.discount, c.tau, c.beta = self._gamma, self._tau, self._awac_lambda
        c.lr_actor, c.lr_q, c.lr_v = float(ga["lr"]), float(g1["lr"]), float(g2["lr"])
        c.adam_beta1, c.adam_beta2, c.adam_eps = float(ga["betas"][0]), float(ga["betas"][1]), float(ga["eps"])
        c.seed = self._seed & 0xFFFFFFFFFFFFFFFF
        return c

    def _build_arenas(self):
        offs, n, nt = _layout(self._cfg(16))
        z = lambda k: torch.zeros(k, dtype=torch.float32, device=self._dev)
        self._params, self._exp_avg, self._exp_avg_sq, self._target = z(n), z(n), z(n), z(nt)
        self._grads = z(n) if self._keep_grads else None
        tensors = self._tensors(self._actor) + [self._actor._log_std] + self._tensors(self._critic_1) + \
            self._tensors(self._critic_2)
        self._views = _arena.bind_parameters(self._params, tensors, offs, self._grads)
        targets = self._tensors(self._target_critic_1) + self._tensors(self._target_critic_2)
        _arena.bind_parameters(self._target, targets, [o - offs[9] for o in offs[9:]])

    def _create_handle(self, batch_size: int):
        cfg = self._cfg(batch_size)
        ar = _lib.Arenas(ptr(self._params), ptr(self._exp_avg), ptr(self._exp_avg_sq), ptr(self._target),
                         ptr(self._grads))
        h = C.c_void_p()
        with torch.cuda.device(self._dev):
            torch.cuda.synchronize(self._dev)  # (the copies are built from the masters on the default stream)
            check(self._lib.iqlhip_awac_create(C.byref(h), C.byref(cfg), float(self._tau), float(self._exp_adv_max),
                                               C.byref(ar)))
        check(self._lib.iqlhip_awac_set_step(h, self.total_it))
        self._lr_sent = None
        return h

    def _copy_out(self, which: int, shape) -> torch.Tensor:
        out = torch.empty(shape, dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_awac_copy_out(self._handle, which, ptr(out), stream_ptr()))
        return out

    def last_eps(self) -> torch.Tensor:
        """The standard normals of the last update, [2, batch_size, action_dim]: [0] those of ``a'`` (awac:269), [1]
        those of ``pi`` (awac:250) -- injected or drawn on the device."""
        if self._handle is None or self.total_it == 0:
            raise RuntimeError("no step has run yet")
        return self._copy_out(0, (2, self._handle_batch, self._action_dim))

    def weight_copies(self) -> Dict[str, torch.Tensor]:
        """The copies the kernels read, as they stand (tests): ``<net>.w<l>`` the padded forward copy of Linear l
        (1..4) [out16, in16] of each of ``NETS``, ``<net>.w<l>t`` the transposed copy [in16, out16] of Linear 2..4 of
        the three trained networks (a critic's single output is padded to 16)."""
        if self._handle is None:
            raise RuntimeError("no step has run yet")
        r16 = lambda x: -(-x // 16) * 16
        S, A, H = self._state_dim, self._action_dim, self._hidden
        out = {}
        for n, name in enumerate(NETS):
            k1, op = (r16(S), r16(A)) if n == 0 else (r16(S + A), 16)
            shapes = [(H, k1), (H, H), (H, H), (op, H)]
            for l, shape in enumerate(shapes):
                out[f"{name}.w{l + 1}"] = self._copy_out(1 + 7 * n + l, shape)
                if l > 0 and n < 3:
                    out[f"{name}.w{l + 1}t"] = self._copy_out(1 + 7 * n + 3 + l, shape[::-1])
        return out

    def _refresh_lrs(self):
        lrs = tuple(float(o.param_groups[0]["lr"]) for o in self._optimizers)
        if lrs != getattr(self, "_lr_sent", None):
            check(self._lib.iqlhip_awac_set_lr(self._handle, *lrs))
            self._lr_sent = lrs

    def _check_eps(self, eps, n_steps: int, batch_size: int) -> Optional[torch.Tensor]:
        if eps is None:
            return None
        if not torch.is_tensor(eps) or eps.dtype != torch.float32 or eps.device.type != "cuda" or \
                tuple(eps.shape) != (n_steps, 2, batch_size, self._action_dim):
            raise ValueError(EPS_SHAPE)
        return eps.contiguous()

    # -- the step ----------------------------------------------------------- #
    def train_steps(self, replay_buffer: ReplayBuffer, n_steps: int, batch_size: int, *, indices: torch.Tensor,
                    eps: Optional[torch.Tensor] = None, return_losses: bool = True):
        """awac:478-480 ``n_steps`` times without host syncs: rows ``indices[i]`` (int64 device tensor [n_steps,
        batch_size]) of the buffer, one ``update`` each.  ``eps``: the standard normals of the updates (float32
        device tensor [n_steps, 2, batch_size, action_dim]) or None: drawn on the device.  Returns the float32
        device tensor [n_steps, 2] of (critic_loss, actor_loss) when ``return_losses``."""
        return self._steps_on_view(replay_buffer.view(), n_steps, batch_size, indices, eps, return_losses)

    def _steps_on_view(self, view: _lib.ReplayView, n_steps: int, batch_size: int, indices, eps, return_losses: bool):
        indices = _arena.check_indices(indices, n_steps, batch_size, True)
        eps = self._check_eps(eps, n_steps, batch_size)
        self._ensure_handle(batch_size)
        self._refresh_lrs()
        losses = torch.empty((n_steps, 2), dtype=torch.float32, device=self._dev) if return_losses else None
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_awac_train_steps(self._handle, C.byref(view), n_steps, ptr(indices), ptr(eps),
                                                    ptr(losses), stream_ptr()))
        self._after_steps(n_steps)
        return losses

    def update(self, batch: TensorBatch, eps: Optional[torch.Tensor] = None) -> Dict[str, float]:
        """awac:301-310 on an explicit batch [s, a, r, s', d]: the rows are laid out as replay rows of their own and
        stepped once in order.  ``eps``: [2, batch_size, action_dim] or None."""
        s, a, r, s2, d = [t.detach().to(device=self._dev, dtype=torch.float32) for t in batch]
        view, idx, _rows = self._batch_as_rows("batch shapes do not match the networks", s, a, r, d, s2)
        losses = self._steps_on_view(view, 1, s.shape[0], idx, None if eps is None else eps[None], True).cpu()
        return {"critic_loss": losses[0, 0].item(), "actor_loss": losses[0, 1].item()}

    # -- checkpoints (awac:312-322) ------------------------------------------ #
    def state_dict(self) -> Dict[str, Any]:
        if self._handle is not None:  # (without a handle no step was ever queued)
            torch.cuda.synchronize(self._dev)
        return {"actor": self._actor.state_dict(), "critic_1": self._critic_1.state_dict(),
                "critic_2": self._critic_2.state_dict()}

    def load_state_dict(self, state_dict: Dict[str, Any]):
        """awac:319-322: the three networks; optimisers, targets and the step count stay as they are."""
        torch.cuda.synchronize(self._dev)
        self._actor.load_state_dict(state_dict["actor"])  # copies into the arena views
        self._critic_1.load_state_dict(state_dict["critic_1"])
        self._critic_2.load_state_dict(state_dict["critic_2"])
        self.sync_weights()


class AWACGroup(ArenaGroup):
    """1..16 ``AdvantageWeightedActorCritic`` trainers of one shape stepped by the same four launches per step
    (``iqlhip_awac_group_*``): the part of ``multi.SeedGroup``'s surface ``_offline_loop.run`` uses, plus ``eps``.
    Every member is bit-identical to stepping it alone."""
    _ENTRY, _LOSSES = "iqlhip_awac", 2

    def train_steps(self, replay, n_steps: int, batch_size: int, *, indices: Sequence[torch.Tensor],
                    eps: Optional[Sequence[Optional[torch.Tensor]]] = None, return_losses: bool = False):
        """``AdvantageWeightedActorCritic.train_steps`` for every member: ``replay`` is one buffer for all or one
        per member, ``indices`` one tensor per member, ``eps`` None or one entry (a tensor or None) per member.
        Returns the list of [n_steps, 2] loss tensors when ``return_losses``."""
        K = len(self.trainers)
        eps = [None] * K if eps is None else list(eps)
        if len(eps) != K:
            raise ValueError("eps: one entry per trainer")
        check_eps = lambda: [t._check_eps(e, n_steps, batch_size) for t, e in zip(self.trainers, eps)]
        return self._group_steps(replay, n_steps, batch_size, indices, return_losses, extra=(check_eps,))


def stepper(trainers: Sequence[AdvantageWeightedActorCritic]) -> AWACGroup:
    """What steps these trainers together: an ``AWACGroup``, for one trainer too (``multi.Solo`` has no ``eps``)."""
    return AWACGroup(trainers)


# --------------------------------------------------------------------------- #
# dataset helpers (awac:380-401; the evaluation, awac:360-377, is ``_d4rl.eval_actor``)
# --------------------------------------------------------------------------- #
def return_reward_range(dataset, max_episode_steps):
    """awac:380-392."""
    returns, lengths = [], []
    ep_ret, ep_len = 0.0, 0
    for r, d in zip(dataset["rewards"], dataset["terminals"]):
        ep_ret += float(r)
        ep_len += 1
        if d or ep_len == max_episode_steps:
            returns.append(ep_ret)
            lengths.append(ep_len)
            ep_ret, ep_len = 0.0, 0
    lengths.append(ep_len)  # but still keep track of number of steps
    assert sum(lengths) == len(dataset["rewards"])
    return min(returns), max(returns)


def modify_reward(dataset, env_name, max_episode_steps=1000):
    """awac:395-401 -- not IQL's: no ``- 1`` for locomotion, ``- 1`` for antmaze."""
    if any(s in env_name for s in ("halfcheetah", "hopper", "walker2d")):
        min_ret, max_ret = return_reward_range(dataset, max_episode_steps)
        dataset["rewards"] /= max_ret - min_ret
        dataset["rewards"] *= max_episode_steps
    elif "antmaze" in env_name:
        dataset["rewards"] -= 1.0


# --------------------------------------------------------------------------- #
# train (awac:415-500)
# --------------------------------------------------------------------------- #
def _build_trainer(seed: int, state_dim: int, action_dim: int, config: TrainConfig,
                   device: str) -> AdvantageWeightedActorCritic:
    """awac:442-468 for one seed: actor, critic 1, critic 2 are built in this order right after
    ``torch.manual_seed(seed)`` on the CPU generator, then moved to the device."""
    torch.manual_seed(seed)
    kw = {"state_dim": state_dim, "action_dim": action_dim, "hidden_dim": config.hidden_dim}
    actor = Actor(**kw)
    critic_1, critic_2 = Critic(**kw), Critic(**kw)
    actor, critic_1, critic_2 = actor.to(device), critic_1.to(device), critic_2.to(device)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=config.learning_rate)
    return AdvantageWeightedActorCritic(
        actor=actor, actor_optimizer=adam(actor), critic_1=critic_1, critic_1_optimizer=adam(critic_1),
        critic_2=critic_2, critic_2_optimizer=adam(critic_2), gamma=config.gamma, tau=config.tau,
        awac_lambda=config.awac_lambda, seed=seed)


def _noise_source(noise, K: int, B: int, A: int, device) -> Optional[Callable]:
    """``noise`` as ``(k, t, n) -> float32 device tensor [n, 2, B, A]``, or None for "device"."""
    if isinstance(noise, str):
        if noise != "device":
            raise ValueError("noise must be 'device', an array [steps, 2, batch_size, action_dim] or a callable "
                             "(member, first step, steps) -> such an array")
        return None
    if callable(noise):
        get = noise
    else:
        if K != 1:
            raise ValueError("a noise array replays one seed; pass a callable for several")
        get = lambda k, t, n: noise[t:t + n]
    def source(k, t, n):
        e = get(k, t, n)
        e = e if torch.is_tensor(e) else torch.from_numpy(np.ascontiguousarray(e, dtype=np.float32))
        if tuple(e.shape) != (n, 2, B, A):
            raise ValueError(f"noise for steps {t}..{t + n - 1} must have shape {(n, 2, B, A)}, not {tuple(e.shape)}")
        return e.to(device=device, dtype=torch.float32).contiguous()
    return source


class _Records(_offline_loop.Records):
    """awac:487-492: ``eval_score``, the mean return, and -- where the environment has ``get_normalized_score`` --
    ``d4rl_normalized_score``, the mean of the episodes' scores x 100."""
    loss_names = LOSS_NAMES

    def __init__(self, env):
        self.env = env

    def evaluated(self, k, trainer, step, returns, log):
        log({"eval_score": returns.mean()})
        if hasattr(self.env, "get_normalized_score"):
            log({"d4rl_normalized_score": (self.env.get_normalized_score(returns) * 100.0).mean()})


def _steps(stream, trainers, buf, gens, B: int, source):
    """The ``steps(group, active, t, n)`` of ``_offline_loop.run``: ``custom_offline._steps`` plus the noise."""
    def steps(group, act, t, n):
        if stream is not None:
            idx = stream.draw([buf.index_bound() for _ in act], n, B, [gens[k] for k in act])
        else:
            idx = [torch.from_numpy(buf.draw_indices(B, n, rng=gens[k])).to(trainers[k]._dev) for k in act]
        eps = None if source is None else [source(k, t, n) for k in act]
        return group.train_steps(buf, n, B, indices=idx, eps=eps, return_losses=True)
    return steps


def train(config: TrainConfig, dataset=None, env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None, seeds_per_gpu: int = 1,
          sampler: str = "device", noise: Union[str, np.ndarray, torch.Tensor, Callable] = "device",
          device: Optional[str] = None, chunk: int = 2000):
    """awac:415-500 on the HIP step.

    ``dataset``: a D4RL transition dict (``observations``, ``actions``, ``next_observations``, ``rewards``,
    ``terminals``; rewritten in place as awac does); None: ``d4rl.qlearning_dataset(env)``.  ``env``: a gym < 0.26
    environment; None: ``gym.make(config.env_name)`` (gym and d4rl are imported only then).  ``logger``,
    ``sampler``, ``device`` and ``chunk`` as in ``custom_offline.train``; ``device`` defaults to the rank's GPU, else
    ``config.device``.  ``noise``: "device" draws the standard normals of every update on the device from the
    seed's Philox key; an array [steps, 2, batch_size, action_dim] (one seed) or a callable ``(member, first step,
    steps) -> array`` replays recorded ones.

    ``seeds_per_gpu`` = K > 1: seed k is ``rank_seed(seed, K) + k`` with its own networks (built right after
    ``torch.manual_seed(seed)``), its own ``np.random.RandomState(seed)`` index stream and noise key, checkpoints
    under ``seed_<seed>/`` and a ``seed`` entry in its records; all K share the buffer and step as one
    ``AWACGroup``.  Every seed is bit-identical to the run it is alone.  Returns the trainer (K = 1) or the list of
    K trainers."""
    _offline_loop.check_sampler(sampler)
    seeds = _offline_loop.group_seeds(config.seed, seeds_per_gpu)
    K = len(seeds)
    device = _d4rl.default_device(config, device)
    env = _d4rl.default_env(config.env_name, env, dataset)
    set_seed(seeds[0], env, deterministic_torch=config.deterministic_torch)  # awac:418
    state_dim = env.observation_space.shape[0]
    action_dim = env.action_space.shape[0]
    dataset = _d4rl.default_dataset(env, dataset)

    # (before anything is uploaded: nothing is launched for a refused shape)
    check_envelope(state_dim, action_dim, config.hidden_dim, config.batch_size)
    source = _noise_source(noise, K, config.batch_size, action_dim, device)

    if config.normalize_reward:
        modify_reward(dataset, config.env_name)
    state_mean, state_std = compute_mean_std(dataset["observations"], eps=1e-3)
    dataset["observations"] = normalize_states(dataset["observations"], state_mean, state_std)
    dataset["next_observations"] = normalize_states(dataset["next_observations"], state_mean, state_std)
    env = wrap_env(env, state_mean=state_mean, state_std=state_std)
    replay_buffer = ReplayBuffer(state_dim, action_dim, config.buffer_size, device)
    replay_buffer.load_d4rl_dataset(dataset)

    trainers = [_build_trainer(s, state_dim, action_dim, config, device) for s in seeds]
    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)
    gens, stream = _co._index_sources(seeds, sampler, device)
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    _offline_loop.run(
        trainers, seeds, lambda active: stepper([trainers[k] for k in active]), int(config.num_train_ops),
        int(config.eval_frequency), chunk, logger, ckpt_dirs,
        _steps(stream, trainers, replay_buffer, gens, config.batch_size, source),
        lambda k, trainer, step: eval_actor(env, trainer._actor, device, config.n_test_episodes, config.test_seed),
        _Records(env))
    return trainers if K > 1 else trainers[0]


def main(argv=None):
    """``python -m iqlpref_amd.awac --config_path file.yaml --field value ...`` (awac:415 pyrallis.wrap)."""
    _d4rl.cli("iqlpref_amd.awac", load_config, train, argv)


if __name__ == "__main__":
    main()
