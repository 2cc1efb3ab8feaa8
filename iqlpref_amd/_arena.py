"""What an arena-backed trainer is, once (``iql.ImplicitQLearning``, ``minari_bc.BC``,
``awac.AdvantageWeightedActorCritic``): parameters, gradients and Adam moments are views of flat fp32 arenas that the
library borrows, behind ``nn.Parameter`` objects and ``optimizer.state`` entries that stay what torch expects, and one
native handle per batch size that lives and dies by one set of rules.  The free functions are pure torch: no library,
any device.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from ._lib import ReplayView, check, ptr, stream_ptr

Views = List[Tuple[torch.nn.Parameter, int]]
INDICES = "indices must be an int64 device tensor [n_steps, batch_size]"


def _cut(arena: torch.Tensor, p: torch.Tensor, o: int) -> torch.Tensor:
    return arena[o:o + p.numel()].view(p.shape)


def bind_parameters(arena: torch.Tensor, params: Sequence[torch.Tensor], offsets: Sequence[int],
                    grads: Optional[torch.Tensor] = None) -> Views:
    """Every parameter becomes a view of ``arena`` at its offset, holding the value it had (and ``p.grad`` the
    same view of ``grads``).  The Parameter objects stay: optimisers keep their references.  Returns the
    (parameter, offset) pairs."""
    views = list(zip(params, (int(o) for o in offsets)))
    with torch.no_grad():
        for p, o in views:
            view = _cut(arena, p, o)
            view.copy_(p.data)
            p.data = view
            if grads is not None:
                p.grad = _cut(grads, p, o)
    return views


def _owned(views: Views, optimizers):
    """(parameter, offset, its optimiser) for every view an optimiser steps."""
    owner = {id(q): opt for opt in optimizers for q in opt.param_groups[0]["params"]}
    return [(p, o, owner[id(p)]) for p, o in views if id(p) in owner]


def bind_adam_state(views: Views, optimizers, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int):
    """The Adam state of every view's parameter becomes views of the moment arenas and a fresh ``step`` counter
    (the float32 scalar torch keeps), so ``optimizer.state_dict()`` stays what ``torch.optim.Adam`` would write.
    Returns the step tensors: moving the counters later is ``fill_`` on each."""
    steps = []
    for p, o, opt in _owned(views, optimizers):
        st = opt.state[p]
        st["step"] = torch.tensor(float(step))
        st["exp_avg"], st["exp_avg_sq"] = _cut(exp_avg, p, o), _cut(exp_avg_sq, p, o)
        steps.append(st["step"])
    return steps


def adopt_adam_state(views: Views, optimizers, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor) -> Optional[int]:
    """The inverse, after ``optimizer.load_state_dict`` made fresh moment tensors: the arenas are zeroed (a
    checkpoint taken before the first step has no moments: they are zero, not stale) and take the moments the
    optimisers hold.  Returns the step count found there, None without any state."""
    found = None
    with torch.no_grad():
        exp_avg.zero_()
        exp_avg_sq.zero_()
        for p, o, opt in _owned(views, optimizers):
            st = opt.state.get(p)
            if st and "exp_avg" in st:
                _cut(exp_avg, p, o).copy_(st["exp_avg"])
                _cut(exp_avg_sq, p, o).copy_(st["exp_avg_sq"])
                found = int(float(st["step"]))
    return found


def check_plain_adam(optimizers, message: str) -> None:
    """NotImplementedError(message) unless every optimiser is ``torch.optim.Adam`` without weight decay, amsgrad
    or maximize: the update kernels are that and nothing else."""
    for opt in optimizers:
        g = opt.param_groups[0]
        if not isinstance(opt, torch.optim.Adam) or g["weight_decay"] != 0 or g["amsgrad"] or g["maximize"]:
            raise NotImplementedError(message)


def check_indices(indices: Optional[torch.Tensor], n_steps: int, batch_size: int, required: bool,
                  message: str = INDICES, device_type: str = "cuda") -> Optional[torch.Tensor]:
    """Injected batch indices as the kernels read them: int64 [n_steps, batch_size] on the device, handed back
    contiguous.  None passes unless ``required``.  ValueError(message) before anything is launched -- a host
    tensor's address would be read on the device (``device_type``: what counts as the device; tests)."""
    if indices is None and not required:
        return None
    if indices is None or indices.dtype != torch.int64 or tuple(indices.shape) != (n_steps, batch_size):
        raise ValueError(message)
    if indices.device.type != device_type:
        raise ValueError(f"{message} (got a tensor on the host)")
    return indices.contiguous()


class ArenaTrainer:
    """The host side of a trainer whose state lives in arenas.  A subclass sets ``_lib``, ``_dev``, ``total_it``,
    ``_views``, ``_exp_avg``, ``_exp_avg_sq`` and ``_optimizers``, names its entry points with ``_ENTRY``
    (``<_ENTRY>_destroy`` / ``_sync_weights`` / ``_set_step``) and builds its native handle in
    ``_create_handle(batch_size)``, in the order of calls its library wants."""
    _ENTRY = ""
    _handle = _handle_batch = None
    _group_owner = None  # the group (``multi.DeviceGroup``) whose device-side handle refers to this one
    _step_tensors = None
    _optimizers: Tuple[torch.optim.Optimizer, ...] = ()

    def _entry(self, name: str):
        return getattr(self._lib, f"{self._ENTRY}_{name}")

    # -- Adam state ---------------------------------------------------------- #
    def _bind_optimizer_state(self, rebuild: bool = False):
        """Adam moments live in the arenas; expose them through ``optimizer.state``.  The views are made once
        (and again with ``rebuild``: ``load_state_dict`` replaces the state tensors, ``state_dict`` trusts
        nothing done to them from outside); afterwards a call only moves the step counters."""
        if self._step_tensors is None or rebuild:
            self._step_tensors = bind_adam_state(self._views, self._optimizers, self._exp_avg, self._exp_avg_sq,
                                                 self.total_it)
            return
        t = float(self.total_it)
        for st in self._step_tensors:
            st.fill_(t)

    def _adopt_optimizer_state(self) -> Optional[int]:
        """After ``optimizer.load_state_dict``: the moments move into the arenas; the views are stale until the
        next ``_bind_optimizer_state``, which rebuilds them.  Returns the optimisers' step count (None: no state)."""
        self._step_tensors = None
        return adopt_adam_state(self._views, self._optimizers, self._exp_avg, self._exp_avg_sq)

    # -- the native handle --------------------------------------------------- #
    def _create_handle(self, batch_size: int):
        raise NotImplementedError

    def _ensure_handle(self, batch_size: int):
        if self._handle is not None and self._handle_batch == batch_size:
            return
        self._destroy_handle()
        self._handle, self._handle_batch = self._create_handle(batch_size), batch_size

    def _destroy_handle(self):
        if self._handle is not None:
            if self._group_owner is not None:  # the device-side group refers to this handle: dissolve it first
                self._group_owner._drop_group()
            torch.cuda.synchronize(self._dev)
            self._entry("destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy_handle()
        except Exception:
            pass

    def _send_step(self):
        """The library's step count (Adam's bias correction, the schedules and streams keyed by it) := ``total_it``."""
        if self._handle is not None:
            with torch.cuda.device(self._dev):
                check(self._entry("set_step")(self._handle, self.total_it))

    def sync_weights(self):
        """Call after writing parameters from outside: the copies the kernels read are rebuilt from the fp32
        masters."""
        if self._handle is not None:
            with torch.cuda.device(self._dev):
                check(self._entry("sync_weights")(self._handle, stream_ptr()))

    # -- steps ---------------------------------------------------------------- #
    def _after_steps(self, n: int):
        """``n`` steps were queued: the count and the optimisers' step counters follow.  (A family with host-side
        schedules overrides this.)"""
        self.total_it += n
        self._bind_optimizer_state()

    def _batch_as_rows(self, message: str, state, action, reward=None, done=None, next_state=None):
        """An explicit batch laid out as replay rows of its own (include/iqlhip.h: s | a | r | d ... s'; a trainer
        that reads only s and a passes only those; needs ``_state_dim`` / ``_action_dim``).  Returns (the view over
        the rows, the indices [1, n] that step them once in order, the rows: keep them until the step is queued).
        RuntimeError(message) when the shapes are not the networks'."""
        n, S, A = state.shape[0], self._state_dim, self._action_dim
        if tuple(state.shape) != (n, S) or tuple(action.shape) != (n, A) or \
                (next_state is not None and tuple(next_state.shape) != (n, S)):
            raise RuntimeError(message)
        stride = self._lib.iqlhip_replay_row_stride(S, A)
        rows = torch.zeros((n, stride), dtype=torch.float32, device=self._dev)
        rows[:, :S], rows[:, S:S + A] = state, action
        if next_state is not None:
            nxt = self._lib.iqlhip_replay_next_offset(S, A)
            rows[:, nxt:nxt + S] = next_state
            rows[:, S + A], rows[:, S + A + 1] = reward.reshape(n), done.reshape(n)
        view = ReplayView(ptr(rows), n, stride, S, A, 0)
        return view, torch.arange(n, dtype=torch.int64, device=self._dev)[None], rows
