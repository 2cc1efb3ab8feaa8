"""``algorithms/minari/any_percent_bc.py`` ("bcref"): any-percent behaviour cloning on a Minari dataset -- keep the
``top_fraction`` of the episodes by discounted return, clone their actions with one ``Actor`` under
``F.mse_loss`` and plain Adam.  The other task-reward baseline of the pen tables beside ``minari_iql``.

The step is a kernel pair of its own (csrc/bc_step.hip, ``iqlhip_bc_*``): one network, no critics, no advantage
weight, no schedule, no ``log_std``, no dropout, fp32 only (bcref has no autocast).  What is kept from bcref,
because it decides what a run computes:

* ``discounted_return`` accumulates from the last reward backwards in the arithmetic of the stored reward dtype
  (bcref:90-94); ``best_trajectories_ids`` sorts by descending return with a stable sort -- ties keep dataset
  order -- and keeps ``max(1, int(top_fraction * n))`` episodes (bcref:97-108);
* ``qlearning_dataset`` lays the rows out in the order of the selected ids, best first (bcref:117): that
  decides which row an index names; the state statistics are those of the selected rows (bcref:300-301);
* indices come from ``np.random.randint`` on numpy's global generator (bcref:181), drawn on the host or by
  ``custom_offline.NumpyIndexStream``;
* one ``{"actor_loss"}`` record per step, ``evaluation_return`` and (where the score function does not raise
  ``ValueError``) ``normalized_score`` at ``(step + 1) % eval_every == 0``, ``checkpoint_{step}.pt`` at the same
  boundaries, no best-model bookkeeping (bcref:339-365); ``BC.state_dict`` has exactly bcref's two keys.
"""
import ctypes as C
import os
import uuid
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _arena, _lib, _offline_loop
from . import custom_offline as _co
from . import distributed as D
from ._lib import check, ptr, stream_ptr
from .custom_offline import ReplayBuffer, evaluate  # noqa: F401  (bcref:133-192, 256-275)
from .iql import mlp_forward_f32, set_seed
from .multi import ArenaGroup
from .multi import stepper as _multi_stepper

HIDDEN = 256  # bcref:199-203
TensorBatch = List[torch.Tensor]


@dataclass
class TrainConfig:
    """bcref:22-48, same fields and defaults."""
    project: str = "CORL"
    group: str = "BC-Minari"
    name: str = "bc"
    gamma: float = 0.99
    top_fraction: float = 0.1
    dataset_id: str = "pen-human-v1"
    update_steps: int = int(1e6)
    buffer_size: int = 2_000_000
    batch_size: int = 256
    normalize_state: bool = True
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
# selection (bcref:90-130)
# --------------------------------------------------------------------------- #
def _field(ep, name):
    return ep[name] if isinstance(ep, dict) else getattr(ep, name)


def discounted_return(x: np.ndarray, gamma: float) -> np.ndarray:
    """bcref:90-94: from the last reward backwards, in the dtype the rewards are stored in (a float32 array
    accumulates in float32: ``gamma`` is a Python float, which does not widen it)."""
    x = np.asarray(x)
    g = x.dtype.type(gamma) if x.dtype.kind == "f" else gamma
    total_return = x[-1]
    for t in reversed(range(x.shape[0] - 1)):
        total_return = x[t] + g * total_return
    return total_return


def best_trajectories_ids(dataset: Iterable, top_fraction: float, gamma: float) -> List[int]:
    """bcref:97-108: the ids of the ``max(1, int(top_fraction * n))`` episodes of greatest discounted return,
    best first; ``sorted`` is stable, so episodes of one return stay in dataset order."""
    ids_and_return = [(_field(ep, "id"), discounted_return(_field(ep, "rewards"), gamma)) for ep in dataset]
    ids_and_returns = sorted(ids_and_return, key=lambda t: -t[1])
    top_ids = [i for (i, r) in ids_and_returns]
    return top_ids[: max(1, int(top_fraction * len(ids_and_returns)))]


def _episodes_by_id(dataset, traj_ids: Sequence[int]):
    if hasattr(dataset, "iterate_episodes"):
        return dataset.iterate_episodes(episode_indices=traj_ids)
    by_id = {_field(ep, "id"): ep for ep in dataset}
    return (by_id[i] for i in traj_ids)


def qlearning_dataset(dataset, traj_ids: Sequence[int]) -> Dict[str, np.ndarray]:
    """bcref:112-130: the transitions of the episodes ``traj_ids``, in that order."""
    obs, next_obs, actions, rewards, dones = [], [], [], [], []
    for ep in _episodes_by_id(dataset, traj_ids):
        o = np.asarray(_field(ep, "observations"))
        obs.append(o[:-1].astype(np.float32))
        next_obs.append(o[1:].astype(np.float32))
        actions.append(np.asarray(_field(ep, "actions")).astype(np.float32))
        rewards.append(np.asarray(_field(ep, "rewards")))
        dones.append(np.asarray(_field(ep, "terminations")))
    return {"observations": np.concatenate(obs), "actions": np.concatenate(actions),
            "next_observations": np.concatenate(next_obs), "rewards": np.concatenate(rewards),
            "terminals": np.concatenate(dones)}


# --------------------------------------------------------------------------- #
# network and trainer (bcref:195-253)
# --------------------------------------------------------------------------- #
class Actor(nn.Module):
    """bcref:195-214 (same parameter names).  ``forward`` outside the trainer is the stand-alone exact-fp32 MFMA
    forward (``iqlhip_mlp_forward``)."""

    def __init__(self, state_dim: int, action_dim: int, max_action: float):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(state_dim, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(),
                                 nn.Linear(HIDDEN, action_dim), nn.Tanh())
        self.max_action = max_action

    def linears(self) -> List[nn.Linear]:
        return [m for m in self.net if isinstance(m, nn.Linear)]

    def forward(self, state: torch.Tensor) -> torch.Tensor:
        lin = self.linears()
        return self.max_action * mlp_forward_f32([l.weight for l in lin], [l.bias for l in lin], state,
                                                 w_in_out=False, hidden_act=0, out_act=1)

    @torch.no_grad()
    def act(self, state: np.ndarray, device: str = "cpu") -> np.ndarray:
        state = torch.tensor(state.reshape(1, -1), device=device, dtype=torch.float32)
        return self(state).cpu().data.numpy().flatten()


class BC(_arena.ArenaTrainer):
    """bcref:217-253 on ``iqlhip_bc_*``.  The actor's parameters, gradients (``keep_grads``) and Adam moments live
    in arenas the library borrows (``_arena``); the parameters stay the same ``nn.Parameter`` objects and
    ``actor_optimizer.state_dict()`` stays what ``torch.optim.Adam`` writes."""
    _ENTRY = "iqlhip_bc"

    def __init__(self, max_action: float, actor: nn.Module, actor_optimizer: torch.optim.Optimizer,
                 device: str = "cpu", *, keep_grads: bool = False):
        self._lib = _lib.load()
        self._dev = _lib.require_gpu(device)
        self.actor, self.actor_optimizer = actor, actor_optimizer
        self._optimizers = (actor_optimizer,)
        self.max_action, self.device = max_action, device
        self.total_it = 0
        self._keep_grads = keep_grads
        lin = actor.linears() if isinstance(actor, Actor) else None
        if lin is None or len(lin) != 3:
            raise TypeError("actor must be an iqlpref_amd.minari_bc.Actor")
        self._state_dim, self._action_dim = lin[0].in_features, lin[2].out_features
        widths = (lin[0].out_features, lin[1].in_features, lin[1].out_features, lin[2].in_features)
        _arena.check_plain_adam(self._optimizers,
                                "the optimiser must be plain torch.optim.Adam (no weight decay / amsgrad / maximize)")
        self._hidden = widths[0] if len(set(widths)) == 1 else -1
        for p in actor.parameters():
            if p.device.type != "cuda":
                raise ValueError("the actor must live on the trainer's device before construction")
        self._build_arenas()

    # -- arenas ------------------------------------------------------------- #
    def _cfg(self, batch_size: int) -> _lib.TrainerConfig:
        g = self.actor_optimizer.param_groups[0]
        c = _lib.TrainerConfig()
        c.state_dim, c.action_dim, c.hidden_dim, c.n_hidden = self._state_dim, self._action_dim, self._hidden, 2
        c.batch_size, c.precision, c.dropout_p = batch_size, _lib.PREC_FP32, -1.0
        c.lr_actor = float(g["lr"])
        c.adam_beta1, c.adam_beta2, c.adam_eps = float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        return c

    def _build_arenas(self):
        offs, n = (C.c_int64 * 6)(), C.c_int64()
        cfg = self._cfg(16)
        check(self._lib.iqlhip_bc_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n)))  # (the envelope is checked here)
        z = lambda: torch.zeros(n.value, dtype=torch.float32, device=self._dev)
        self._params, self._exp_avg, self._exp_avg_sq = z(), z(), z()
        self._grads = z() if self._keep_grads else None
        tensors = [t for l in self.actor.linears() for t in (l.weight, l.bias)]
        self._views = _arena.bind_parameters(self._params, tensors, offs, self._grads)

    def _create_handle(self, batch_size: int):
        cfg = self._cfg(batch_size)
        ar = _lib.Arenas(ptr(self._params), ptr(self._exp_avg), ptr(self._exp_avg_sq), None, ptr(self._grads))
        h = C.c_void_p()
        with torch.cuda.device(self._dev):
            torch.cuda.synchronize(self._dev)  # (the copies are built from the masters on the default stream)
            check(self._lib.iqlhip_bc_create(C.byref(h), C.byref(cfg), float(self.max_action), C.byref(ar)))
        check(self._lib.iqlhip_bc_set_step(h, self.total_it))
        return h

    def weight_copies(self) -> Dict[str, torch.Tensor]:
        """The copies the kernels read, as they stand (tests): the padded forward copies ``w1`` [256, S16],
        ``w2`` [256, 256], ``w3`` [A16, 256] and the transposed ``w2t`` [256, 256], ``w3t`` [256, A16]."""
        if self._handle is None:
            raise RuntimeError("no step has run yet")
        S16, A16 = -(-self._state_dim // 16) * 16, -(-self._action_dim // 16) * 16
        shapes = {"w1": (HIDDEN, S16), "w2": (HIDDEN, HIDDEN), "w3": (A16, HIDDEN), "w2t": (HIDDEN, HIDDEN),
                  "w3t": (HIDDEN, A16)}
        out = {}
        with torch.cuda.device(self._dev):
            for i, (name, shape) in enumerate(shapes.items()):
                out[name] = torch.empty(shape, dtype=torch.float32, device=self._dev)
                check(self._lib.iqlhip_bc_copy_out(self._handle, i, ptr(out[name]), stream_ptr()))
        return out

    def _refresh_lrs(self):
        lr = float(self.actor_optimizer.param_groups[0]["lr"])
        if lr != getattr(self, "_lr_sent", None):
            check(self._lib.iqlhip_bc_set_lr(self._handle, lr))
            self._lr_sent = lr

    # -- the step ----------------------------------------------------------- #
    def train_steps(self, replay_buffer: ReplayBuffer, n_steps: int, batch_size: int, *,
                    indices: torch.Tensor, dropout_keep=None, return_losses: bool = True,
                    graph_unroll: Optional[int] = None, n_valid=None):
        """bcref:339-341 ``n_steps`` times without host syncs: rows ``indices[i]`` (int64 device tensor
        [n_steps, batch_size]) of the buffer, forward, mse loss, backward, Adam.  Returns the float32 device tensor
        [n_steps, 1] of the steps' ``actor_loss`` when ``return_losses``.

        The other keywords are those of ``ImplicitQLearning.train_steps``, so that ``multi.Solo`` steps either
        family: ``dropout_keep`` and ``n_valid`` must be None (the BC step has no dropout and pads its own batch),
        ``graph_unroll`` is accepted and unused (the step issues plain launches)."""
        if dropout_keep is not None or n_valid is not None:
            raise NotImplementedError("the BC step has no dropout and pads its own batch: dropout_keep and n_valid "
                                      "must be None")
        return self._steps_on_view(replay_buffer.view(), n_steps, batch_size, indices, return_losses)

    def _steps_on_view(self, view: _lib.ReplayView, n_steps: int, batch_size: int, indices, return_losses: bool):
        self._ensure_handle(batch_size)
        self._refresh_lrs()
        indices = _arena.check_indices(indices, n_steps, batch_size, True)
        losses = torch.empty((n_steps, 1), dtype=torch.float32, device=self._dev) if return_losses else None
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_bc_train_steps(self._handle, C.byref(view), n_steps, ptr(indices), ptr(losses),
                                                  stream_ptr()))
        self._after_steps(n_steps)
        return losses

    def train(self, batch: TensorBatch) -> Dict[str, float]:
        """bcref:230-243 on an explicit batch [s, a, ...]: the rows are laid out as replay rows of their own and
        stepped once in order."""
        state, action = [t.detach().to(device=self._dev, dtype=torch.float32) for t in batch[:2]]
        view, idx, _rows = self._batch_as_rows("batch shapes do not match the actor", state, action)
        return {"actor_loss": self._steps_on_view(view, 1, state.shape[0], idx, True).item()}

    # -- checkpoints (bcref:245-253) ----------------------------------------- #
    def state_dict(self) -> Dict[str, Any]:
        if self._handle is not None:  # (without a handle no step was ever queued)
            torch.cuda.synchronize(self._dev)
        # (fresh views: whatever was done to the optimiser's state from outside, the checkpoint holds the arenas')
        if self.total_it > 0:  # (before the first step the optimiser holds no state, as bcref's)
            self._bind_optimizer_state(rebuild=True)
        return {"actor": self.actor.state_dict(), "actor_optimizer": self.actor_optimizer.state_dict()}

    def load_state_dict(self, state_dict: Dict[str, Any]):
        torch.cuda.synchronize(self._dev)
        self.actor.load_state_dict(state_dict["actor"])  # copies into the arena views
        self.actor_optimizer.load_state_dict(state_dict["actor_optimizer"])
        # (optimizer.load_state_dict made fresh moment tensors; the count is the optimiser's, bcref keeps no other)
        self.total_it = self._adopt_optimizer_state() or 0
        if self.total_it > 0:
            self._bind_optimizer_state(rebuild=True)
        self._send_step()
        self.sync_weights()


def check_envelope(state_dim: int, action_dim: int, batch_size: int = 16) -> None:
    """NotImplementedError (ValueError for a dim < 1) when the step's kernels are not built for the shape
    (include/iqlhip.h: state_dim <= 128, action_dim <= 32); touches no device."""
    c = _lib.TrainerConfig()
    c.state_dim, c.action_dim, c.hidden_dim, c.n_hidden = state_dim, action_dim, HIDDEN, 2
    c.batch_size, c.precision, c.dropout_p = batch_size, _lib.PREC_FP32, -1.0
    offs, n = (C.c_int64 * 6)(), C.c_int64()
    check(_lib.load().iqlhip_bc_arena_layout(C.byref(c), C.byref(offs), C.byref(n)))


class BCGroup(ArenaGroup):
    """K ``BC`` trainers of one shape stepped by the same two launches per step (``iqlhip_bc_group_*``): the part
    of ``multi.SeedGroup``'s surface ``_offline_loop.run`` uses.  Every member is bit-identical to stepping it
    alone.  One trainer needs no group: ``stepper`` hands back a ``multi.Solo``."""
    _ENTRY, _LOSSES = "iqlhip_bc", 1

    def train_steps(self, replay, n_steps: int, batch_size: int, *, indices: Sequence[torch.Tensor],
                    return_losses: bool = False):
        """``BC.train_steps`` for every member: ``replay`` is one buffer for all or one per member, ``indices``
        one tensor per member.  Returns the list of [n_steps, 1] loss tensors when ``return_losses``."""
        return self._group_steps(replay, n_steps, batch_size, indices, return_losses)


def stepper(trainers: Sequence[BC]):
    """What steps these trainers together: ``multi.Solo`` for one, ``BCGroup`` for more."""
    return _multi_stepper(trainers, group=BCGroup)


# --------------------------------------------------------------------------- #
# train (bcref:278-365)
# --------------------------------------------------------------------------- #
def _build_trainer(seed: int, state_dim: int, action_dim: int, max_action: float, device: str) -> BC:
    """bcref:327-337 for one seed: the net is built right after ``torch.manual_seed(seed)`` on the CPU generator,
    then moved to the device."""
    torch.manual_seed(seed)
    actor = Actor(state_dim, action_dim, max_action).to(device)
    return BC(max_action=max_action, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
              device=device)


def train(config: TrainConfig, dataset=None, eval_env=None, *,
          logger: Optional[Callable[[Dict[str, float], int], None]] = None,
          normalized_score: Optional[Callable] = None, seeds_per_gpu: int = 1, sampler: str = "device",
          device: Optional[str] = None, chunk: int = 2000):
    """bcref:278-365 on the HIP step.

    ``dataset``: a Minari-style dataset -- iterable of episodes with ``id``, ``observations``, ``actions``,
    ``rewards``, ``terminations``, and ``iterate_episodes(episode_indices=)`` (a plain list of episodes is looked
    up by id); None loads ``config.dataset_id`` with minari.  ``eval_env``, ``logger``, ``normalized_score``,
    ``sampler``, ``device`` and ``chunk`` as in ``custom_offline.train``.

    ``seeds_per_gpu`` = K > 1, as there: seed k is ``rank_seed(train_seed, K) + k`` with its own net (built right
    after ``torch.manual_seed(seed)``), its own ``np.random.RandomState(seed)`` index stream, its own checkpoints
    under ``seed_<seed>/`` and a ``seed`` entry in its records; all K share the buffer and step as one
    ``BCGroup`` on the indices of one K-stream draw.  Every seed is bit-identical to the run it is alone.
    Returns the trainer (K = 1) or the list of K trainers."""
    _offline_loop.check_sampler(sampler)
    seeds = _offline_loop.group_seeds(config.train_seed, seeds_per_gpu)
    K = len(seeds)
    if device is None:
        device = D.local_device() or "cuda:0"
    dataset, eval_env, normalized_score, state_dim, action_dim, max_action = _co._minari_setup(
        "minari_bc.train", config, dataset, eval_env, normalized_score)

    check_envelope(state_dim, action_dim)  # (before the buffer is packed: nothing is launched for a refused shape)

    qdataset = qlearning_dataset(dataset, best_trajectories_ids(dataset, config.top_fraction, config.gamma))
    replay_buffer, eval_env = _co._prepare(config, qdataset, eval_env, state_dim, action_dim, device)  # bcref:300-312

    ckpt_dirs = _offline_loop.checkpoint_dirs(config, seeds)
    set_seed(seeds[0])  # np, random, torch, PYTHONHASHSEED (bcref:327)
    trainers = [_build_trainer(s, state_dim, action_dim, max_action, device) for s in seeds]
    gens, stream = _co._index_sources(seeds, sampler, device)
    if logger is None:
        logger = _offline_loop.default_logger(config, K)

    normalized = None if normalized_score is None else (lambda scores: normalized_score(dataset, scores))
    _offline_loop.run(
        trainers, seeds, lambda active: stepper(trainers), int(config.update_steps), int(config.eval_every), chunk,
        logger, ckpt_dirs, _co._steps(stream, trainers, [replay_buffer] * K, gens, config.batch_size),
        lambda k, trainer, step: evaluate(eval_env, trainer.actor, config.eval_episodes, config.eval_seed, device),
        _offline_loop.EvalRecords(normalized, ("actor_loss",)))
    return trainers if K > 1 else trainers[0]
