"""``algorithms/offline/td3_bc.py`` ("tdbc"): offline TD3+BC, the actor-critic baseline the D4RL tables are most often
read against.

The step is the third family on the slab-step core (csrc/td3_bc_step.hip, ``iqlhip_td3bc_*``): fp32 (tdbc has no
autocast), two hidden layers of ``hidden_dim`` (a multiple of 16 in 16..256; tdbc's own is 256), ``state_dim`` <= 128,
``action_dim`` <= 32, any batch size up to 65536, plain Adam, 1..16 members per group.  A step is two launches, five
when the actor steps.  What is kept from tdbc, because it decides what a run computes:

* ``train`` (tdbc:324-380) in its order: ``a' = clamp(actor_target(s') + clamp(eps policy_noise, +-noise_clip),
  +-max_action)``, the critics against ``r + (1 - d) discount min Q_target(s', a')``, ``mse + mse`` (a sum), both Adam
  steps; when ``total_it % policy_freq == 0`` the actor on ``-lmbda mean Q1(s, pi) + mse(pi, a)`` with ``lmbda = alpha
  / mean|Q1(s, pi)|`` at the critic 1 just updated, then ``t <- (1 - tau) t + tau s`` for all three targets (tdbc:79);
  on any other step the actor, its optimiser (moments and ``step``) and the three targets keep their bits;
* one draw of standard normals per step, [B, A]: injected (``eps=``, ``noise=``) or drawn on the device from the
  trainer's Philox key (Box-Muller, stream 7; include/iqlhip.h);
* indices from ``np.random.randint(0, min(size, pointer), size=B)`` on numpy's global generator (tdbc:162);
* ``normalize`` / ``normalize_reward`` as tdbc:418-432; ``policy_noise`` and ``noise_clip`` times ``max_action``
  (tdbc:473-474);
* records at the ONE-based ``total_it`` (tdbc:499): ``critic_loss`` every step, ``actor_loss`` only where the actor
  stepped; at ``(t + 1) % eval_freq == 0`` an evaluation, ``d4rl_normalized_score =
  get_normalized_score(returns.mean()) * 100`` and ``checkpoint_{t}.pt`` (zero-based, tdbc:523) with the seven-key
  state dict of tdbc:382-391; ``load_model`` (tdbc:487-490).

Not here: bf16, ``resume``, sweep files, ``posthoc``, widths above 256, other depths.
"""
import ctypes as C
import os
import uuid
from copy import deepcopy
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import _arena, _d4rl, _lib, _offline_loop
from . import custom_offline as _co
from ._d4rl import eval_actor  # noqa: F401  (tdbc:200-217)
from ._lib import check, ptr, stream_ptr
from .awac import modify_reward, return_reward_range  # noqa: F401  (tdbc:220-241 are awac:380-401 word for word)
from .iql import load_config_for, compute_mean_std, normalize_states, set_seed, mlp_forward_f32  # noqa: F401
from .multi import ArenaGroup
from .train import wrap_env  # noqa: F401  (tdbc:92-111)

TensorBatch = List[torch.Tensor]
NETS = ("actor", "critic_1", "critic_2", "actor_target", "critic_1_target", "critic_2_target")
TRAINED = NETS[:3]
MAX_HIDDEN, MAX_STATE, MAX_ACTION = 256, 128, 32
LOSS_NAMES = ("critic_loss", "actor_loss")
EPS_SHAPE = "eps must be a float32 device tensor [n_steps, batch_size, action_dim]"


@dataclass
class TrainConfig:
    """tdbc:19-74, same fields and defaults."""
    project: str = "CORL"
    group: str = "TD3_BC-D4RL"
    name: str = "TD3_BC"
    env: str = "halfcheetah-medium-expert-v2"
    alpha: float = 2.5
    discount: float = 0.99
    expl_noise: float = 0.1
    tau: float = 0.005
    policy_noise: float = 0.2
    noise_clip: float = 0.5
    policy_freq: int = 2
    max_timesteps: int = int(1e6)
    buffer_size: int = 2_000_000
    batch_size: int = 256
    normalize: bool = True
    normalize_reward: bool = False
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
    """The pyrallis ``--config_path`` behaviour (tdbc:409) with ``iql.load_config``'s rules."""
    return load_config_for(TrainConfig, "td3_bc.TrainConfig", config_path, **overrides)


class ReplayBuffer(_co.ReplayBuffer):
    """tdbc:114-173 on the packed device rows: ``load_d4rl_dataset`` (its two ``ValueError``s), ``sample`` on
    ``np.random.randint(0, min(size, pointer), size=B)`` of numpy's global generator (tdbc:162)."""


# --------------------------------------------------------------------------- #
# networks (tdbc:244-282)
# --------------------------------------------------------------------------- #
def _linears(module: nn.Module) -> List[nn.Linear]:
    return [m for m in getattr(module, "net", ()) if isinstance(m, nn.Linear)]


class Actor(nn.Module):
    """tdbc:244-265 (the reference's ``net.{0,2,4}`` names); ``hidden_dim``: 256 there."""

    def __init__(self, state_dim: int, action_dim: int, max_action: float, hidden_dim: int = 256):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(state_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, action_dim), nn.Tanh())
        self.max_action = max_action

    def forward(self, state: torch.Tensor) -> torch.Tensor:
        lin = _linears(self)
        return self.max_action * mlp_forward_f32([l.weight for l in lin], [l.bias for l in lin], state,
                                                 w_in_out=False, hidden_act=0, out_act=1)

    @torch.no_grad()
    def act(self, state: np.ndarray, device: str = "cpu") -> np.ndarray:
        state = torch.tensor(state.reshape(1, -1), device=device, dtype=torch.float32)
        return self(state).cpu().data.numpy().flatten()


class Critic(nn.Module):
    """tdbc:268-282."""

    def __init__(self, state_dim: int, action_dim: int, hidden_dim: int = 256):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(state_dim + action_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1))

    def forward(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        lin = _linears(self)
        return mlp_forward_f32([l.weight for l in lin], [l.bias for l in lin], torch.cat([state, action], 1),
                               w_in_out=False, hidden_act=0, out_act=0)


def soft_update(target: nn.Module, source: nn.Module, tau: float):
    """tdbc:77-79 (host-side helper; the training step fuses this into its update launches)."""
    for target_param, source_param in zip(target.parameters(), source.parameters()):
        target_param.data.copy_((1 - tau) * target_param.data + tau * source_param.data)


def _net_dims(actor: nn.Module, critics: Sequence[nn.Module]):
    """(state_dim, action_dim, hidden_dim) of networks of tdbc's shape; TypeError for anything else,
    NotImplementedError for shapes the kernels do not carry."""
    la = _linears(actor)
    if len(la) != 3 or not isinstance(actor.net[-1], nn.Tanh):
        raise TypeError("actor must be an iqlpref_amd.td3_bc.Actor (three Linear layers and a Tanh in net)")
    S, A, H = la[0].in_features, la[2].out_features, la[0].out_features
    for i, lin in enumerate([la] + [_linears(c) for c in critics]):
        if len(lin) != 3:
            raise TypeError("a critic must be an iqlpref_amd.td3_bc.Critic (three Linear layers in net)")
        want = [(S if i == 0 else S + A, H), (H, H), (H, A if i == 0 else 1)]
        if [(l.in_features, l.out_features) for l in lin] != want or any(l.bias is None for l in lin):
            raise NotImplementedError("the TD3+BC step trains networks of two hidden layers of one width, the critics "
                                      "on cat(state, action) with one output")
    return S, A, H


def _config(state_dim: int, action_dim: int, hidden_dim: int, batch_size: int) -> _lib.TrainerConfig:
    c = _lib.TrainerConfig()
    c.state_dim, c.action_dim, c.hidden_dim, c.n_hidden = state_dim, action_dim, hidden_dim, 2
    c.batch_size, c.precision, c.dropout_p = batch_size, _lib.PREC_FP32, -1.0
    return c


def _layout(cfg: _lib.TrainerConfig):
    offs, n = (C.c_int64 * 18)(), C.c_int64()
    check(_lib.load().iqlhip_td3bc_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n)))
    return list(offs), n.value


def check_envelope(state_dim: int, action_dim: int, hidden_dim: int, batch_size: int = 16, policy_freq: int = 1) -> None:
    """NotImplementedError (ValueError for a dim < 1) when the step's kernels are not built for the shape
    (include/iqlhip.h); touches no device."""
    if int(policy_freq) < 1:
        raise NotImplementedError(f"policy_freq {policy_freq} < 1")
    _layout(_config(state_dim, action_dim, hidden_dim, batch_size))


def _actor_steps(total_it: int, n: int, policy_freq: int) -> int:
    """How many of the steps total_it + 1 .. total_it + n (one-based, tdbc:326) are actor steps."""
    return (total_it + n) // policy_freq - total_it // policy_freq


# --------------------------------------------------------------------------- #
# trainer (tdbc:285-406)
# --------------------------------------------------------------------------- #
class TD3_BC(_arena.ArenaTrainer):
    """tdbc:285-406 on ``iqlhip_td3bc_*``.  The parameters of the three trained networks, their gradients
    (``keep_grads``) and Adam moments live in arenas the library borrows (``_arena``), the three deep-copied targets in
    a target arena of the same layout; all stay the ``nn.Parameter`` objects they were, and each
    ``optimizer.state_dict()`` stays what ``torch.optim.Adam`` writes -- the actor's ``step`` is the count of its own
    updates.  ``seed``: the Philox key of the noise drawn on the device."""
    _ENTRY = "iqlhip_td3bc"

    def __init__(self, max_action: float, actor: nn.Module, actor_optimizer: torch.optim.Optimizer, critic_1: nn.Module,
                 critic_1_optimizer: torch.optim.Optimizer, critic_2: nn.Module,
                 critic_2_optimizer: torch.optim.Optimizer, discount: float = 0.99, tau: float = 0.005,
                 policy_noise: float = 0.2, noise_clip: float = 0.5, policy_freq: int = 2, alpha: float = 2.5,
                 device: str = "cpu", *, seed: int = 0, keep_grads: bool = False):
        self._state_dim, self._action_dim, self._hidden = _net_dims(actor, (critic_1, critic_2))
        self._optimizers = (actor_optimizer, critic_1_optimizer, critic_2_optimizer)
        _arena.check_plain_adam(self._optimizers,
                                "the optimisers must be plain torch.optim.Adam (no weight decay / amsgrad / maximize)")
        groups = [o.param_groups[0] for o in self._optimizers]
        if len({(tuple(g["betas"]), g["eps"]) for g in groups}) != 1:
            raise NotImplementedError("the three optimisers share betas and eps (they may differ in lr)")
        check_envelope(self._state_dim, self._action_dim, self._hidden, policy_freq=policy_freq)
        if float(getattr(actor, "max_action", max_action)) != float(max_action):
            raise ValueError("the actor's max_action is not the trainer's")
        params = [p for m in (actor, critic_1, critic_2) for p in m.parameters()]
        if any(p.device.type != "cuda" for p in params) or len({p.device for p in params}) != 1:
            raise ValueError("the networks must live on one GPU before construction")
        self._lib = _lib.load()
        self._dev = _lib.require_gpu(params[0].device)
        self.actor, self.actor_optimizer = actor, actor_optimizer
        self.critic_1, self.critic_1_optimizer = critic_1, critic_1_optimizer
        self.critic_2, self.critic_2_optimizer = critic_2, critic_2_optimizer
        self.actor_target, self.critic_1_target, self.critic_2_target = deepcopy(actor), deepcopy(critic_1), deepcopy(critic_2)
        self.max_action, self.discount, self.tau = max_action, discount, tau
        self.policy_noise, self.noise_clip, self.policy_freq, self.alpha = policy_noise, noise_clip, int(policy_freq), alpha
        self.device = device
        self._seed, self._keep_grads = int(seed), keep_grads
        self.total_it = 0
        self._actor_it = 0  # the actor optimiser's own step count
        self._build_arenas()

    def _modules(self) -> Dict[str, nn.Module]:
        return {n: getattr(self, n) for n in NETS}

    # -- arenas ------------------------------------------------------------- #
    @staticmethod
    def _tensors(module: nn.Module) -> List[torch.Tensor]:
        return [t for l in _linears(module) for t in (l.weight, l.bias)]

    def _cfg(self, batch_size: int) -> _lib.TrainerConfig:
        c = _config(self._state_dim, self._action_dim, self._hidden, batch_size)
        ga, g1, g2 = (o.param_groups[0] for o in self._optimizers)
        c.discount, c.tau = self.discount, self.tau
        c.lr_actor, c.lr_q, c.lr_v = float(ga["lr"]), float(g1["lr"]), float(g2["lr"])
        c.adam_beta1, c.adam_beta2, c.adam_eps = float(ga["betas"][0]), float(ga["betas"][1]), float(ga["eps"])
        c.seed = self._seed & 0xFFFFFFFFFFFFFFFF
        return c

    def _build_arenas(self):
        offs, n = _layout(self._cfg(16))
        z = lambda k: torch.zeros(k, dtype=torch.float32, device=self._dev)
        self._params, self._exp_avg, self._exp_avg_sq, self._target = z(n), z(n), z(n), z(n)
        self._grads = z(n) if self._keep_grads else None
        tensors = [t for m in (self.actor, self.critic_1, self.critic_2) for t in self._tensors(m)]
        self._views = _arena.bind_parameters(self._params, tensors, offs, self._grads)
        self._bind_targets()

    def _bind_targets(self):
        offs, _ = _layout(self._cfg(16))
        targets = [t for m in (self.actor_target, self.critic_1_target, self.critic_2_target) for t in self._tensors(m)]
        _arena.bind_parameters(self._target, targets, offs)

    def _create_handle(self, batch_size: int):
        cfg = self._cfg(batch_size)
        ar = _lib.Arenas(ptr(self._params), ptr(self._exp_avg), ptr(self._exp_avg_sq), ptr(self._target),
                         ptr(self._grads))
        h = C.c_void_p()
        with torch.cuda.device(self._dev):
            torch.cuda.synchronize(self._dev)  # (the copies are built from the masters on the default stream)
            check(self._lib.iqlhip_td3bc_create(C.byref(h), C.byref(cfg), float(self.tau), float(self.policy_noise),
                                                float(self.noise_clip), float(self.max_action), float(self.alpha),
                                                int(self.policy_freq), C.byref(ar)))
        check(self._lib.iqlhip_td3bc_set_step(h, self.total_it, self._actor_it))
        self._lr_sent = None
        return h

    def _send_step(self):
        if self._handle is not None:
            with torch.cuda.device(self._dev):
                check(self._lib.iqlhip_td3bc_set_step(self._handle, self.total_it, self._actor_it))

    # -- Adam state: the actor's optimiser counts its own steps --------------- #
    def _bind_optimizer_state(self, rebuild: bool = False):
        super()._bind_optimizer_state(rebuild)
        for p in self.actor_optimizer.param_groups[0]["params"]:
            self.actor_optimizer.state[p]["step"].fill_(float(self._actor_it))

    def _after_steps(self, n: int):
        self._actor_it += _actor_steps(self.total_it, n, self.policy_freq)
        super()._after_steps(n)

    def _copy_out(self, which: int, shape) -> torch.Tensor:
        out = torch.empty(shape, dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_td3bc_copy_out(self._handle, which, ptr(out), stream_ptr()))
        return out

    def last_eps(self) -> torch.Tensor:
        """The standard normals of the last step (tdbc:333), [batch_size, action_dim]: injected or drawn on the device."""
        if self._handle is None or self.total_it == 0:
            raise RuntimeError("no step has run yet")
        return self._copy_out(0, (self._handle_batch, self._action_dim))

    def weight_copies(self) -> Dict[str, torch.Tensor]:
        """The copies the kernels read, as they stand (tests): ``<net>.w<l>`` the padded forward copy of Linear l
        (1..3) [out16, in16] of each of ``NETS``, ``<net>.w<l>t`` the transposed copy [in16, out16] of Linear 2 and 3 of
        the three trained networks and of Linear 1 of critic 1 (a critic's single output is padded to 16)."""
        if self._handle is None:
            raise RuntimeError("no step has run yet")
        r16 = lambda x: -(-x // 16) * 16
        S, A, H = self._state_dim, self._action_dim, self._hidden
        out = {}
        for n, name in enumerate(NETS):
            k1, op = (r16(S), r16(A)) if n % 3 == 0 else (r16(S + A), 16)
            for l, shape in enumerate([(H, k1), (H, H), (op, H)]):
                out[f"{name}.w{l + 1}"] = self._copy_out(1 + 6 * n + l, shape)
                if n < 3 and (l > 0 or n == 1):
                    out[f"{name}.w{l + 1}t"] = self._copy_out(1 + 6 * n + 3 + l, shape[::-1])
        return out

    def _refresh_lrs(self):
        lrs = tuple(float(o.param_groups[0]["lr"]) for o in self._optimizers)
        if lrs != getattr(self, "_lr_sent", None):
            check(self._lib.iqlhip_td3bc_set_lr(self._handle, *lrs))
            self._lr_sent = lrs

    def _check_eps(self, eps, n_steps: int, batch_size: int) -> Optional[torch.Tensor]:
        if eps is None:
            return None
        if not torch.is_tensor(eps) or eps.dtype != torch.float32 or eps.device.type != "cuda" or \
                tuple(eps.shape) != (n_steps, batch_size, self._action_dim):
            raise ValueError(EPS_SHAPE)
        return eps.contiguous()

    # -- the step ----------------------------------------------------------- #
    def train_steps(self, replay_buffer: ReplayBuffer, n_steps: int, batch_size: int, *, indices: torch.Tensor,
                    eps: Optional[torch.Tensor] = None, return_losses: bool = True):
        """tdbc:496-498 ``n_steps`` times without host syncs: rows ``indices[i]`` (int64 device tensor [n_steps,
        batch_size]) of the buffer, one ``train`` each.  ``eps``: the standard normals of the steps (float32 device
        tensor [n_steps, batch_size, action_dim]) or None: drawn on the device.  Returns the float32 device tensor
        [n_steps, 2] of (critic_loss, actor_loss) when ``return_losses``; the actor_loss of a step without an actor
        update is 0.0."""
        return self._steps_on_view(replay_buffer.view(), n_steps, batch_size, indices, eps, return_losses)

    def _steps_on_view(self, view: _lib.ReplayView, n_steps: int, batch_size: int, indices, eps, return_losses: bool):
        indices = _arena.check_indices(indices, n_steps, batch_size, True)
        eps = self._check_eps(eps, n_steps, batch_size)
        self._ensure_handle(batch_size)
        self._refresh_lrs()
        losses = torch.empty((n_steps, 2), dtype=torch.float32, device=self._dev) if return_losses else None
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_td3bc_train_steps(self._handle, C.byref(view), n_steps, ptr(indices), ptr(eps),
                                                     ptr(losses), stream_ptr()))
        self._after_steps(n_steps)
        return losses

    def train(self, batch: TensorBatch, eps: Optional[torch.Tensor] = None) -> Dict[str, float]:
        """tdbc:324-380 on an explicit batch [s, a, r, s', d]: the rows are laid out as replay rows of their own and
        stepped once in order.  ``eps``: [batch_size, action_dim] or None.  ``actor_loss`` only on an actor step."""
        s, a, r, s2, d = [t.detach().to(device=self._dev, dtype=torch.float32) for t in batch]
        view, idx, _rows = self._batch_as_rows("batch shapes do not match the networks", s, a, r, d, s2)
        losses = self._steps_on_view(view, 1, s.shape[0], idx, None if eps is None else eps[None], True).cpu()
        log_dict = {"critic_loss": losses[0, 0].item()}
        if self.total_it % self.policy_freq == 0:
            log_dict["actor_loss"] = losses[0, 1].item()
        return log_dict

    # -- checkpoints (tdbc:382-406) ------------------------------------------ #
    def state_dict(self) -> Dict[str, Any]:
        if self._handle is not None:  # (without a handle no step was ever queued)
            torch.cuda.synchronize(self._dev)
        self._bind_optimizer_state(rebuild=True)
        return {"critic_1": self.critic_1.state_dict(), "critic_1_optimizer": self.critic_1_optimizer.state_dict(),
                "critic_2": self.critic_2.state_dict(), "critic_2_optimizer": self.critic_2_optimizer.state_dict(),
                "actor": self.actor.state_dict(), "actor_optimizer": self.actor_optimizer.state_dict(),
                "total_it": self.total_it}

    def load_state_dict(self, state_dict: Dict[str, Any]):
        """tdbc:393-406: the networks, the optimisers -- each with its own step count -- and ``total_it``; the three
        targets become copies of the networks loaded."""
        torch.cuda.synchronize(self._dev)
        for name in TRAINED:
            getattr(self, name).load_state_dict(state_dict[name])  # copies into the arena views
            getattr(self, name + "_optimizer").load_state_dict(state_dict[name + "_optimizer"])
        with torch.no_grad():
            self._target.copy_(self._params)  # (one layout: tdbc:396-404's three deepcopies)
        self.total_it = int(state_dict["total_it"])
        actor_state = [self.actor_optimizer.state.get(p) for p in self.actor_optimizer.param_groups[0]["params"]]
        steps = [int(float(st["step"])) for st in actor_state if st and "step" in st]
        self._actor_it = steps[0] if steps else 0
        self._adopt_optimizer_state()
        self._bind_optimizer_state(rebuild=True)
        self._send_step()
        self.sync_weights()


class TD3BCGroup(ArenaGroup):
    """1..16 ``TD3_BC`` trainers of one shape stepped by the same launches (``iqlhip_td3bc_group_*``): every
    hyperparameter and step count is the member's own, and the actor launches are issued on a step on which any
    member's actor steps.  Every member is bit-identical to stepping it alone."""
    _ENTRY, _LOSSES = "iqlhip_td3bc", 2

    def train_steps(self, replay, n_steps: int, batch_size: int, *, indices: Sequence[torch.Tensor],
                    eps: Optional[Sequence[Optional[torch.Tensor]]] = None, return_losses: bool = False):
        """``TD3_BC.train_steps`` for every member: ``replay`` is one buffer for all or one per member, ``indices``
        one tensor per member, ``eps`` None or one entry (a tensor or None) per member.  Returns the list of
        [n_steps, 2] loss tensors when ``return_losses``."""
        K = len(self.trainers)
        eps = [None] * K if eps is None else list(eps)
        if len(eps) != K:
            raise ValueError("eps: one entry per trainer")
        check_eps = lambda: [t._check_eps(e, n_steps, batch_size) for t, e in zip(self.trainers, eps)]
        return self._group_steps(replay, n_steps, batch_size, indices, return_losses, extra=(check_eps,))


def stepper(trainers: Sequence[TD3_BC]) -> TD3BCGroup:
    """What steps these trainers together: a ``TD3BCGroup``, for one trainer too (``multi.Solo`` has no ``eps``)."""
    return TD3BCGroup(trainers)


# --------------------------------------------------------------------------- #
# train (tdbc:409-529)
# --------------------------------------------------------------------------- #
def _build_trainer(seed: int, state_dim: int, action_dim: int, max_action: float, config: TrainConfig, device: str,
                   hidden_dim: int = 256) -> TD3_BC:
    """tdbc:453-485 for one seed: actor, critic 1, critic 2 are built in this order right after
    ``torch.manual_seed(seed)`` on the CPU generator, then moved to the device."""
    torch.manual_seed(seed)
    actor = Actor(state_dim, action_dim, max_action, hidden_dim).to(device)
    critic_1 = Critic(state_dim, action_dim, hidden_dim).to(device)
    critic_2 = Critic(state_dim, action_dim, hidden_dim).to(device)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=3e-4)
    return TD3_BC(max_action=max_action, actor=actor, actor_optimizer=adam(actor), critic_1=critic_1,
                  critic_1_optimizer=adam(critic_1), critic_2=critic_2, critic_2_optimizer=adam(critic_2),
                  discount=config.discount, tau=config.tau, device=device, policy_noise=config.policy_noise * max_action,
                  noise_clip=config.noise_clip * max_action, policy_freq=config.policy_freq, alpha=config.alpha, seed=seed)


def _noise_source(noise, K: int, B: int, A: int, device) -> Optional[Callable]:
    """``noise`` as ``(k, t, n) -> float32 device tensor [n, B, A]``, or None for "device"."""
    if noise is None or isinstance(noise, str):
        if noise not in (None, "device"):
            raise ValueError("noise must be None or 'device', an array [steps, batch_size, action_dim] or a callable "
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
        if tuple(e.shape) != (n, B, A):
            raise ValueError(f"noise for steps {t}..{t + n - 1} must have shape {(n, B, A)}, not {tuple(e.shape)}")
        return e.to(device=device, dtype=torch.float32).contiguous()
    return source


class _Records(_offline_loop.Records):
    """tdbc:499, 510-529: the records carry the one-based ``total_it``; ``critic_loss`` every step, ``actor_loss``
    only where the actor stepped -- decided from the step count, never from the column's value; an evaluation logs
    ``d4rl_normalized_score``, the score of the mean return x 100, alone."""
    loss_names = LOSS_NAMES

    def __init__(self, env, policy_freq: int, first_it: int = 0):
        self.env, self.policy_freq, self.step_offset = env, int(policy_freq), int(first_it) + 1

    def loss_record(self, k, row, step):
        rec = dict(zip(self.loss_names, row))
        if (step + self.step_offset) % self.policy_freq != 0:
            del rec["actor_loss"]
        return rec

    def evaluated(self, k, trainer, step, returns, log):
        log({"d4rl_normalized_score": self.env.get_normalized_score(returns.mean()) * 100.0})


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
          sampler: str = "device", noise: Union[None, str, np.ndarray, torch.Tensor, Callable] = None,
          device: Optional[str] = None, chunk: int = 2000, hidden_dim: int = 256):
    """tdbc:409-529 on the HIP step.

    ``dataset``: a D4RL transition dict (rewritten in place as tdbc does); None: ``d4rl.qlearning_dataset(env)``.
    ``env``: a gym < 0.26 environment with ``get_normalized_score``; None: ``gym.make(config.env)``.  ``logger``,
    ``sampler``, ``device`` and ``chunk`` as in ``custom_offline.train``.  ``noise``: None (or "device") draws the standard
    normals of every step on the device from the seed's Philox key; an array [steps, batch_size, action_dim] (one
    seed) or a callable ``(member, first step, steps) -> array`` replays recorded ones.  ``hidden_dim``: tdbc's
    networks are 256 wide; tests run narrower ones.

    ``seeds_per_gpu`` = K > 1: seed k is ``rank_seed(seed, K) + k`` with its own networks, index stream and noise
    key, evaluation seed (tdbc:508 evaluates on the training seed), checkpoints under ``seed_<seed>/`` and a ``seed``
    entry in its records; all K share the buffer and step as
    one ``TD3BCGroup``.  Every seed is bit-identical to the run it is alone.  Returns the trainer (K = 1) or the list
    of K trainers."""
    _offline_loop.check_sampler(sampler)
    seeds = _offline_loop.group_seeds(config.seed, seeds_per_gpu)
    K = len(seeds)
    device = _d4rl.default_device(config, device)
    env = _d4rl.default_env(config.env, env, dataset)
    state_dim = env.observation_space.shape[0]
    action_dim = env.action_space.shape[0]
    dataset = _d4rl.default_dataset(env, dataset)

    # (before anything is uploaded: nothing is launched for a refused shape)
    check_envelope(state_dim, action_dim, hidden_dim, config.batch_size, config.policy_freq)
    source = _noise_source(noise, K, config.batch_size, action_dim, device)

    if config.normalize_reward:
        modify_reward(dataset, config.env)
    if config.normalize:
        state_mean, state_std = compute_mean_std(dataset["observations"], eps=1e-3)
    else:
        state_mean, state_std = 0, 1
    dataset["observations"] = normalize_states(dataset["observations"], state_mean, state_std)
    dataset["next_observations"] = normalize_states(dataset["next_observations"], state_mean, state_std)
    env = wrap_env(env, state_mean=state_mean, state_std=state_std)
    replay_buffer = ReplayBuffer(state_dim, action_dim, config.buffer_size, device)
    replay_buffer.load_d4rl_dataset(dataset)
    max_action = float(env.action_space.high[0])

    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)
    set_seed(seeds[0], env)  # tdbc:451: after the buffer is loaded
    trainers = [_build_trainer(s, state_dim, action_dim, max_action, config, device, hidden_dim) for s in seeds]
    first_it = 0
    if config.load_model != "":  # tdbc:487-490
        for t in trainers:
            t.load_state_dict(torch.load(config.load_model))
        first_it = trainers[0].total_it
    gens, stream = _co._index_sources(seeds, sampler, device)
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    _offline_loop.run(
        trainers, seeds, lambda active: stepper([trainers[k] for k in active]), int(config.max_timesteps),
        int(config.eval_freq), chunk, logger, ckpt_dirs,
        _steps(stream, trainers, replay_buffer, gens, config.batch_size, source),
        lambda k, trainer, step: eval_actor(env, trainer.actor, device, config.n_episodes, seeds[k]),  # tdbc:508: its own seed
        _Records(env, config.policy_freq, first_it))
    return trainers if K > 1 else trainers[0]


def main(argv=None):
    """``python -m iqlpref_amd.td3_bc --config_path file.yaml --field value ...`` (tdbc:409 pyrallis.wrap)."""
    _d4rl.cli("iqlpref_amd.td3_bc", load_config, train, argv)


if __name__ == "__main__":
    main()
