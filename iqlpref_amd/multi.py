"""Several independent IQL seeds on ONE GPU.

One seed at batch 256 is a latency chain that leaves most of an MI355X idle;
the reference runs several W&B agents per GPU for the same reason
(``ensemble_sweeps/launch.sh:12`` AGENTS_PER_GPU).  ``SeedGroup`` is that, inside one process.
The trainers share nothing (own arenas, own Philox stream) and the arithmetic of every seed
is bit-identical to running it alone.  Two execution modes:

``mode="group"``
    ONE launch sequence steps all seeds: every kernel of the step runs with gridDim.y = K
    (``iqlhip_group_train_steps``; with per-step valid-row counts ``iqlhip_group_train_steps_valid``).  K x the work-groups per launch, one third of the kernel
    boundaries per seed-step.
``mode="streams"``
    every trainer replays its own hipGraph on its own HIP stream; the launches interleave.
``mode="split"`` (``n_streams=G``, default 2; the default mode for trainers of one shape)
    G sub-groups, each stepped by its own launch sequence on its own HIP stream, every stream
    confined to its own slice of the compute units (bit i of the CU mask belongs to slice i % G,
    ``iqlhip_stream_create_cu_slice``; the mask runs round-robin over the 8 XCDs, so two slices
    are the even and the odd XCDs).  The sub-groups share no CU and no L2, only the memory system:
    one's HBM-bound k_update runs beside the other's latency-bound k_forward / k_backward.
    Measured (tools/group_streams.py, tools/group_scan.py): 2 / 4 / 8 / 16 seeds as two sub-groups
    107k / 160k / 202k / 250k steps/s against 93k / 130k / 171k / 204k as one group.  Two slices are the
    sweet spot (three do not divide the chip's 8 XCDs evenly, four leave each sub-group too few CUs).
``mode="general"``
    ``mode="group"`` for trainers that run on the general layer-wise step (``step_kind() ==
    "general"``: n_hidden != 2 or a hidden_dim other than 64 / 128 / 256): ONE launch sequence for
    up to ``MAX_GROUP`` such trainers of one shape, hipGraphs of ``graph_unroll`` steps.  Never
    picked by default: general-step trainers default to ``"streams"``.
"""
import ctypes as C
import os
from typing import List, Optional, Sequence, Union

import torch

from . import _lib
from ._arena import check_indices
from ._lib import check, ptr, stream_ptr
from .iql import ImplicitQLearning, ReplayBuffer


# The CU-slice streams of a device are created once per process and shared by every split-mode
# group: a slice stream created after an earlier one was destroyed landed on the hardware queue
# of its sibling (both halves of the chip then serialised: 91k instead of 190k steps/s).
_SLICE_STREAMS = {}


def _slice_streams(lib, dev, n_slices: int):
    key = (torch.device(dev).index or 0, n_slices)
    if key not in _SLICE_STREAMS:
        raw = []
        with torch.cuda.device(dev):
            for g in range(n_slices):
                st = C.c_void_p()
                check(lib.iqlhip_stream_create_cu_slice(C.byref(st), g, n_slices))
                raw.append(st)
        _SLICE_STREAMS[key] = (raw, [torch.cuda.ExternalStream(st.value, device=dev) for st in raw])
    return list(_SLICE_STREAMS[key][1])


def _shape_key(t: ImplicitQLearning):
    return (t._state_dim, t._action_dim, t._hidden, t._n_hidden, t._precision, t._deterministic, t._n_critics,
            bool(t._dropout))


def _on_tuned_step(t: ImplicitQLearning) -> bool:
    """Group launches exist for the tuned three-kernel step only (include/iqlhip.h, shape envelope);
    trainers of other shapes (n_hidden != 2, other widths) are stepped one by one, each on its stream."""
    return t._n_hidden == 2 and t._hidden in (64, 128, 256)


GROUP_MODES = ("group", "split", "streams", "general")


def check_group_mode(group_mode: Optional[str]) -> Optional[str]:
    """The ``group_mode`` keyword of ``train()`` / ``sweep.train_runs()``: None (the SeedGroup default) or a
    SeedGroup mode.  Host-only: callers validate before any device work."""
    if group_mode is not None and group_mode not in GROUP_MODES:
        raise ValueError(f"group_mode must be None or one of {', '.join(repr(m) for m in GROUP_MODES)} "
                         f"(got {group_mode!r})")
    return group_mode


def resolve_group_mode(group_mode: Optional[str], trainers: Sequence[ImplicitQLearning], batch_size: int):
    """The SeedGroup mode for these trainers under ``group_mode``.  "general" holds for trainers that run on
    the general layer-wise step; asked for trainers of the tuned step (a grid may hold both kinds of batch)
    it falls back to None, the SeedGroup default.  Every other value passes through."""
    check_group_mode(group_mode)
    if group_mode == "general" and not all(t.step_kind(batch_size) == "general" for t in trainers):
        return None
    return group_mode


def _per_member(K: int, replay, indices, dropout_keep, n_valid):
    """The arguments of ``train_steps`` as one entry per trainer each: (buffers, indices, dropout_keep, n_valid)."""
    bufs = list(replay) if isinstance(replay, (list, tuple)) else [replay] * K
    if len(bufs) != K:
        raise ValueError("one replay buffer per trainer (or a single shared one)")
    idx = list(indices) if indices is not None else [None] * K
    keep = list(dropout_keep) if dropout_keep is not None else [None] * K
    if len(idx) != K or len(keep) != K:
        raise ValueError("indices / dropout_keep: one entry per trainer")
    valid = [n_valid] * K if n_valid is None or isinstance(n_valid, torch.Tensor) else list(n_valid)
    if len(valid) != K:
        raise ValueError("n_valid: one tensor for all trainers or one entry per trainer")
    return bufs, idx, keep, valid


class DeviceGroup:
    """A native group over the handles of member trainers (``_arena.ArenaTrainer``), built from the members' handle
    values and keyed on that tuple: a member whose handle was rebuilt (another batch size) dissolves the group
    through ``_group_owner`` first, and the next step builds a new one.  A subclass sets ``trainers``, ``_lib`` and
    ``_dev`` and supplies ``_create_group`` / ``_destroy_group``."""
    _group = _key = None
    trainers: Sequence = ()

    def _create_group(self, batch_size: int, handles, n: int) -> C.c_void_p:
        raise NotImplementedError

    def _destroy_group(self, group) -> None:
        raise NotImplementedError

    def _ensure_group(self, batch_size: int):
        for t in self.trainers:
            t._ensure_handle(batch_size)
        key = tuple(t._handle.value for t in self.trainers)
        if self._group is not None and key == self._key:
            return
        self._drop_group()
        self._group, self._key = self._create_group(batch_size, (C.c_void_p * len(key))(*key), len(key)), key
        for t in self.trainers:
            t._group_owner = self

    def _drop_group(self):
        if self._group is not None:
            self._destroy_group(self._group)
            self._group = None
            for t in self.trainers:
                t._group_owner = None

    def close(self):
        """Dissolve the device-side group; the trainers stay usable on their own."""
        self._drop_group()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        torch.cuda.current_stream(self._dev).synchronize()


class ArenaGroup(DeviceGroup):
    """The group of a family whose native group steps K trainers of one shape by injected indices
    (``minari_bc.BCGroup``, ``awac.AWACGroup``).  A subclass names the family's entry points (``_ENTRY``:
    ``<_ENTRY>_group_create`` / ``_destroy`` / ``_train_steps``) and the width of a step's loss record (``_LOSSES``)."""
    _ENTRY, _LOSSES = "", 1

    def __init__(self, trainers: Sequence):
        if not 1 <= len(trainers) <= _lib.MAX_GROUP:
            raise NotImplementedError(f"a group has 1..{_lib.MAX_GROUP} members")
        if len({id(t) for t in trainers}) != len(trainers) or len({t._dev for t in trainers}) != 1:
            raise ValueError("the members of a group are distinct trainers on one device")
        self.trainers = list(trainers)
        self._lib, self._dev = trainers[0]._lib, trainers[0]._dev

    def __len__(self):
        return len(self.trainers)

    def _group_entry(self, name: str):
        return getattr(self._lib, f"{self._ENTRY}_group_{name}")

    def _create_group(self, batch_size: int, handles, n: int):
        g = C.c_void_p()
        check(self._group_entry("create")(C.byref(g), handles, n))
        return g

    def _destroy_group(self, group):
        torch.cuda.synchronize(self._dev)
        self._group_entry("destroy")(group)

    def _group_steps(self, replay, n_steps: int, batch_size: int, indices, return_losses: bool, extra=()):
        """The family's ``train_steps`` for every member: ``replay`` one buffer for all or one per member,
        ``indices`` one tensor per member.  ``extra``: callables that check and hand back one more per-member list
        of optional device tensors each, passed on between the indices and the losses (all None: a null array);
        they run after the indices are checked and before anything is created.  Returns the list of [n_steps,
        _LOSSES] loss tensors when ``return_losses``."""
        K = len(self.trainers)
        bufs, idx, _, _ = _per_member(K, replay, indices, None, None)
        idx = [check_indices(i, n_steps, batch_size, True) for i in idx]
        more = [e() for e in extra]
        self._ensure_group(batch_size)
        for t in self.trainers:
            t._refresh_lrs()
        losses = [torch.empty((n_steps, self._LOSSES), dtype=torch.float32, device=self._dev) for _ in range(K)] \
            if return_losses else None
        views = (_lib.ReplayView * K)(*[b.view() for b in bufs])
        parr = lambda ts: None if ts is None or all(t is None for t in ts) else \
            (C.c_void_p * K)(*[None if t is None else t.data_ptr() for t in ts])
        with torch.cuda.device(self._dev):
            check(self._group_entry("train_steps")(self._group, views, n_steps, parr(idx), *map(parr, more), parr(losses),
                                                   stream_ptr()))
        for t in self.trainers:
            t._after_steps(n_steps)
        return losses


class SeedGroup(DeviceGroup):
    def __init__(self, trainers: Sequence[ImplicitQLearning], chunk: int = 2000, mode: Optional[str] = None,
                 n_streams: int = 2):
        if not trainers:
            raise ValueError("SeedGroup needs at least one trainer")
        devs = {t._dev for t in trainers}
        if len(devs) != 1:
            raise ValueError("all trainers of a SeedGroup must live on one device")
        if len({id(t) for t in trainers}) != len(trainers):
            raise ValueError("a trainer may appear only once in a SeedGroup")
        one_shape = len({_shape_key(t) for t in trainers}) == 1 and len(trainers) <= _lib.MAX_GROUP and \
            all(_on_tuned_step(t) for t in trainers)
        if mode is None:  # the fastest arrangement measured for the shape at hand
            mode = ("split" if len(trainers) >= 2 else "group") if one_shape else "streams"
        if mode not in ("group", "streams", "split", "general"):
            raise ValueError("mode must be 'group', 'streams', 'split' or 'general'")
        if mode == "general":
            if len({_shape_key(t) for t in trainers}) != 1 or len(trainers) > _lib.MAX_GROUP:
                raise ValueError(f"mode='general' needs at most {_lib.MAX_GROUP} trainers of one shape (dims, hidden, "
                                 "n_hidden, precision, policy kind, critics, dropout on/off)")
            self._check_general(trainers)
        if mode in ("group", "split") and not one_shape:
            raise ValueError(f"mode='group' needs at most {_lib.MAX_GROUP} trainers of one shape (dims, hidden, "
                             "precision, policy kind, critics, dropout on/off) that runs on the tuned step "
                             "(n_hidden = 2, hidden_dim 64 / 128 / 256)")
        self.mode = mode
        self.trainers: List[ImplicitQLearning] = list(trainers)
        self._dev = next(iter(devs))
        self._lib = _lib.load()
        self._streams = [torch.cuda.Stream(device=self._dev) for _ in self.trainers] if mode == "streams" else []
        self._chunk = int(chunk)
        self._children: List["SeedGroup"] = []
        self._child_slices: List[slice] = []
        if mode == "split":
            G = max(1, min(int(n_streams), len(self.trainers)))
            base, extra, lo = len(self.trainers) // G, len(self.trainers) % G, 0
            for g in range(G):  # contiguous runs of trainers, sizes differing by at most one
                hi = lo + base + (1 if g < extra else 0)
                self._children.append(SeedGroup(self.trainers[lo:hi], mode="group"))
                self._child_slices.append(slice(lo, hi))
                lo = hi
            self._chunk = min(self._chunk, 500)  # short turns keep the queues of all streams fed

    def __len__(self):
        return len(self.trainers)

    @staticmethod
    def _check_general(trainers, batch_size: Optional[int] = None):
        """mode="general" is for members on the general layer-wise step.  Asked of the device handle where one
        exists (IQLHIP_FORCE_GENERAL moves shapes over); without a handle the library's rule for the shape."""
        def kind(t):
            if batch_size is not None:
                return t.step_kind(batch_size)
            if t._handle is not None:
                return t.step_kind(t._handle_batch)
            return "tuned" if _on_tuned_step(t) and not os.environ.get("IQLHIP_FORCE_GENERAL") else "general"
        tuned = [i for i, t in enumerate(trainers) if kind(t) != "general"]
        if tuned:
            raise ValueError(f"mode='general' is for trainers on the general layer-wise step; members {tuned} run "
                             "on the tuned step (use mode='group' or 'split')")

    # -- group handle --------------------------------------------------------- #
    def _create_group(self, batch_size: int, handles, n: int):
        if self.mode == "general":
            self._check_general(self.trainers, batch_size)
        g = C.c_void_p()
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_group_create(C.byref(g), handles, n))
        return g

    def _destroy_group(self, group):
        self._lib.iqlhip_group_destroy(group)  # (waits for the device itself)

    def close(self):
        for ch in getattr(self, "_children", []):
            ch.close()
        self._drop_group()
        if getattr(self, "mode", None) == "split":
            for st in self._streams:
                st.synchronize()
            self._streams = []  # (the slice streams themselves are shared and stay, see _slice_streams)

    # -- stepping ------------------------------------------------------------- #
    def train_steps(self, replay: Union[ReplayBuffer, Sequence[ReplayBuffer]], n_steps: int, batch_size: int, *,
                    indices: Optional[Sequence[Optional[torch.Tensor]]] = None,
                    dropout_keep: Optional[Sequence[Optional[torch.Tensor]]] = None,
                    return_losses: bool = False, graph_unroll: Optional[int] = None,
                    n_valid: Union[None, torch.Tensor, Sequence[Optional[torch.Tensor]]] = None):
        """``n_steps`` x (sample + train) for every seed.  ``replay`` is one buffer shared by all
        seeds (a sweep varies the seed only) or one per seed; ``indices`` / ``dropout_keep`` are
        optional per-seed lists (entries may be None) with the meaning of
        ``ImplicitQLearning.train_steps``.  ``n_valid``: the per-step valid-row counts of
        ``ImplicitQLearning.train_steps`` -- one int32 [n_steps] device tensor shared by all seeds (the
        short last batch of a BB epoch falls on the same step for every seed) or one entry per seed
        (None: that seed uses its whole batch); fp32 trainers on the tuned step only, every other group
        raises NotImplementedError before anything is launched.  Returns a list of [n_steps, 3] loss tensors when
        ``return_losses``.  Asynchronous: call ``synchronize()`` (or read the losses) before
        touching the parameters."""
        K = len(self.trainers)
        bufs, idx, keep, valid = _per_member(K, replay, indices, dropout_keep, n_valid)
        valid = self._check_valid(valid, n_steps, batch_size)
        if self.mode == "streams":
            return self._train_streams(bufs, n_steps, batch_size, idx, keep, return_losses, graph_unroll, valid)
        if self.mode == "split":
            return self._train_split(bufs, n_steps, batch_size, idx, keep, return_losses, graph_unroll, valid)
        self._ensure_group(batch_size)
        idx = [check_indices(t, n_steps, batch_size, False, "indices must be int64 [n_steps, batch_size]") for t in idx]
        keep = [None if k is None else t._check_keep(k, n_steps, batch_size) for t, k in zip(self.trainers, keep)]
        losses = [torch.empty((n_steps, 3), dtype=torch.float32, device=self._dev) for _ in range(K)] \
            if return_losses else None
        views = (_lib.ReplayView * K)(*[b.view() for b in bufs])
        parr = lambda ts: (C.c_void_p * K)(*[None if t is None else t.data_ptr() for t in ts])
        any_idx, any_keep = any(t is not None for t in idx), any(t is not None for t in keep)
        any_valid = any(t is not None for t in valid)
        for t in self.trainers:
            t._refresh_lrs()
        # (group launches: graphs of 50 steps 202-204k steps/s for 8 seeds, plain launches 198-200k)
        unroll = 50 if graph_unroll is None else graph_unroll
        with torch.cuda.device(self._dev):
            check(self._lib.iqlhip_group_train_steps_valid(
                self._group, views, n_steps, parr(idx) if any_idx else None,
                parr(valid) if any_valid else None, parr(keep) if any_keep else None, parr(losses) if losses is not None else None,
                unroll, stream_ptr()))
        for t in self.trainers:
            t._after_steps(n_steps)
        return losses

    def _check_valid(self, valid, n_steps: int, batch_size: int) -> List[Optional[torch.Tensor]]:
        """``n_valid``, one entry per trainer, checked as ``ImplicitQLearning.train_steps`` checks it; the
        groups the counted step is not built for are refused here, before any member is stepped."""
        for i, t in enumerate(valid):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n_steps,) or \
                    t.device.type != "cuda":
                raise ValueError("n_valid must be an int32 device tensor [n_steps]")
            valid[i] = t.contiguous()
        if all(t is None for t in valid):
            return valid
        if self.mode == "general" or any(t.step_kind(batch_size) == "general" for t in self.trainers):
            raise NotImplementedError("per-step valid-row counts (a short batch) run on the tuned step only (n_hidden 2, "
                                      "hidden_dim 64 / 128 / 256); this group runs the general layer-wise step")
        if any(t._precision != _lib.PREC_FP32 for t in self.trainers):
            raise NotImplementedError("per-step valid-row counts (a short batch) are built for precision fp32 only")
        return valid

    def _train_streams(self, bufs, n_steps, batch_size, idx, keep, return_losses, graph_unroll, valid):
        cur = torch.cuda.current_stream(self._dev)
        for st in self._streams:
            st.wait_stream(cur)
        out = [[] for _ in self.trainers]
        done = 0
        while done < n_steps:  # round-robin in chunks so that the queues of all streams stay fed
            c = min(self._chunk, n_steps - done)
            for k, (tr, st, buf) in enumerate(zip(self.trainers, self._streams, bufs)):
                with torch.cuda.stream(st):
                    # (one host thread feeds every stream: graphs keep its share per step small)
                    r = tr.train_steps(buf, c, batch_size, return_losses=return_losses,
                                       indices=None if idx[k] is None else idx[k][done:done + c],
                                       dropout_keep=None if keep[k] is None else keep[k][done:done + c],
                                       n_valid=None if valid[k] is None else valid[k][done:done + c],
                                       graph_unroll=8 if graph_unroll is None else graph_unroll)
                    if return_losses:
                        out[k].append(r)
            done += c
        for st in self._streams:
            cur.wait_stream(st)
        return [torch.cat(o) for o in out] if return_losses else None

    def _ensure_slice_streams(self):
        if self._streams:
            return
        try:
            self._streams = _slice_streams(self._lib, self._dev, len(self._children))
        except Exception as e:  # no CU-masked streams here: plain streams keep the results, not the speed
            import warnings
            warnings.warn(f"SeedGroup(mode='split'): CU-slice streams unavailable ({e}); using plain streams")
            self._streams = [torch.cuda.Stream(device=self._dev) for _ in self._children]

    def _train_split(self, bufs, n_steps, batch_size, idx, keep, return_losses, graph_unroll, valid):
        self._ensure_slice_streams()
        cur = torch.cuda.current_stream(self._dev)
        for st in self._streams:
            st.wait_stream(cur)
        out = [[] for _ in self.trainers]
        done = 0
        while done < n_steps:
            c = min(self._chunk, n_steps - done)
            for ch, sl, st in zip(self._children, self._child_slices, self._streams):
                cut = lambda ts: [None if t is None else t[done:done + c] for t in ts[sl]]
                with torch.cuda.stream(st):
                    r = ch.train_steps(bufs[sl], c, batch_size, indices=cut(idx), dropout_keep=cut(keep),
                                       return_losses=return_losses, graph_unroll=graph_unroll, n_valid=cut(valid))
                if return_losses:
                    for k, rk in zip(range(sl.start, sl.stop), r):
                        out[k].append(rk)
            done += c
        for st in self._streams:
            cur.wait_stream(st)
        return [torch.cat(o) for o in out] if return_losses else None

    def kernel_times(self, replay, batch_size: int, n_steps: int = 200):
        """Average duration (us) of the forward / backward / update launches of this group
        (mode "group"): ``n_steps`` eager steps with a HIP-event pair around every launch."""
        if self.mode not in ("group", "general"):
            raise ValueError("kernel_times needs mode='group' or 'general'")
        self._ensure_group(batch_size)
        check(self._lib.iqlhip_group_set_timing(self._group, 1))
        try:
            self.train_steps(replay, n_steps, batch_size, graph_unroll=0)
            avg, n = (C.c_double * 3)(), C.c_int64()
            check(self._lib.iqlhip_group_get_timing(self._group, C.byref(avg), C.byref(n)))
        finally:
            check(self._lib.iqlhip_group_set_timing(self._group, 0))
        return {"k_forward": avg[0] * 1e3, "k_backward": avg[1] * 1e3, "k_update": avg[2] * 1e3,
                "launches": int(n.value)}

    def launch_counts(self):
        """(steps issued as plain launches, hipGraph replays issued) of this group's launch sequence since
        its device-side group was created (modes "group" / "general"; a step of K members counts once)."""
        if self.mode not in ("group", "general"):
            raise ValueError("launch_counts needs mode='group' or 'general'")
        if self._group is None:
            return (0, 0)
        eager, graphs = C.c_int64(), C.c_int64()
        check(self._lib.iqlhip_group_launch_counts(self._group, C.byref(eager), C.byref(graphs)))
        return (int(eager.value), int(graphs.value))

    def synchronize(self):
        for st in self._streams:
            st.synchronize()
        super().synchronize()


class Solo:
    """ONE trainer behind the part of ``SeedGroup``'s surface the training loops use, so that a loop drives one
    seed and K seeds with the same calls.  Nothing is added on the device: no group is created, the trainer
    is never owned, there is no stream of its own, and ``train_steps`` is one ``trainer.train_steps`` call with
    ``SeedGroup.train_steps``' argument conventions and ValueErrors (every per-member list holds one entry;
    ``graph_unroll`` None leaves the unroll to the trainer) that returns ``[losses]`` or None.  Every trainer
    family whose ``train_steps`` takes these keywords is served: ``ImplicitQLearning`` and ``minari_bc.BC``."""
    mode = "solo"

    def __init__(self, trainer):
        self.trainers = [trainer]

    def __len__(self):
        return 1

    def train_steps(self, replay, n_steps: int, batch_size: int, *, indices=None, dropout_keep=None,
                    return_losses: bool = False, graph_unroll: Optional[int] = None, n_valid=None):
        (buf,), (idx,), (keep,), (valid,) = _per_member(1, replay, indices, dropout_keep, n_valid)
        losses = self.trainers[0].train_steps(buf, n_steps, batch_size, indices=idx, dropout_keep=keep,
                                              return_losses=return_losses, graph_unroll=graph_unroll, n_valid=valid)
        return [losses] if return_losses else None

    def synchronize(self):
        torch.cuda.current_stream(self.trainers[0]._dev).synchronize()

    def close(self):
        pass


def stepper(trainers: Sequence, mode: Optional[str] = None, *, group=None, **kw):
    """What steps these trainers together: ``Solo`` for one; for more ``SeedGroup(trainers, mode=mode, **kw)``, or
    ``group(trainers, **kw)`` for a family with a group class of its own (``minari_bc.BCGroup``)."""
    if len(trainers) == 1:
        return Solo(trainers[0])
    return SeedGroup(trainers, mode=mode, **kw) if group is None else group(trainers, **kw)
