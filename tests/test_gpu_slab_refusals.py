"""What the host code under the BC and AWAC steps (csrc/slab_step.h: ``slab_group_create``, the per-member view
check of ``slab_run``) turns down, for both families, through ctypes straight on the handles -- ``BCGroup`` /
``AWACGroup`` refuse most of it before the library sees it.  -m gpu.

Trainers of the smallest shapes (BC: S 3, A 1; AWAC: S 3, A 1, H 16).  Group create: 0 members, 17 members, a null
member, a member listed twice, members that differ in batch size, members that differ in ``max_action`` (BC) or
``gamma`` (AWAC).  ``train_steps`` of one trainer and of a group: a view of other dims, a view of 0 rows, null
indices.  Each refusal gives its error code and a fragment of its message, every one comes back before any launch,
and the step count did not move: after all of them one step from the trainer equals, bit for bit, the same step of
a twin that saw none (Adam's bias correction is keyed by the library's count, and the refused calls asked for 3
steps).
"""
import ctypes as C

import pytest
import torch

from tests import slab_digests as sd

pytestmark = pytest.mark.gpu
DEV, S, A, H = "cuda:0", 3, 1, 16
N_ROWS = 8


def _family(name):
    """(build(batch, other) -> trainer with a handle, the shape-mismatch fragment, its null-indices fragment,
    train(lib, handle, view, n, idx, losses), group_train(lib, group, views, n, idx array, losses))."""
    if name == "bc":
        def build(batch, other=False, seed=0):
            tr = sd._bc(S, A, 0.75 if other else 0.5, seed=seed)
            tr._ensure_handle(batch)
            return tr
        train = lambda lib, h, view, n, idx: lib.iqlhip_bc_train_steps(h, view, n, idx, None, None)
        gtrain = lambda lib, g, views, n, idx: lib.iqlhip_bc_group_train_steps(g, views, n, idx, None, None)
        return build, "share dims, batch size and max_action", "behaviour cloning takes its indices", train, gtrain
    def build(batch, other=False, seed=0):
        tr = sd._awac(S, A, H, 1.0, seed=seed, gamma=0.9 if other else 0.99)
        tr._ensure_handle(batch)
        return tr
    train = lambda lib, h, view, n, idx: lib.iqlhip_awac_train_steps(h, view, n, idx, None, None, None)
    gtrain = lambda lib, g, views, n, idx: lib.iqlhip_awac_group_train_steps(g, views, n, idx, None, None, None)
    return build, "share dims, width, batch size, gamma", "AWAC takes its indices", train, gtrain


@pytest.mark.parametrize("name", ["bc", "awac"])
def test_refusals_come_back_before_any_launch(name):
    from iqlpref_amd import _lib
    lib = _lib.load()
    build, shape_text, idx_text, train, gtrain = _family(name)
    create = getattr(lib, f"iqlhip_{name}_group_create")
    destroy = getattr(lib, f"iqlhip_{name}_group_destroy")
    B = 1
    tr, twin, mate = build(B), build(B), build(B, seed=1)
    other_batch, other_const = build(17, seed=2), build(B, other=True, seed=3)
    everyone = (tr, twin, mate, other_batch, other_const)

    def refused(rc, code, text):
        msg = lib.iqlhip_last_error().decode()
        assert rc == code and text in msg, (rc, msg)
        assert all(t.total_it == 0 for t in everyone)

    # ---- group create ----
    def group_of(handles, n=None):
        arr = (C.c_void_p * max(len(handles), 1))(*handles)
        out = C.c_void_p()
        rc = create(C.byref(out), arr, len(handles) if n is None else n)
        assert not out.value
        return rc

    h, hm = tr._handle.value, mate._handle.value
    refused(group_of([h], n=0), _lib.ERR_UNSUPPORTED, "a group has 1..16 members (got 0)")
    refused(group_of([h] * 17), _lib.ERR_UNSUPPORTED, "a group has 1..16 members (got 17)")
    refused(group_of([h, None]), _lib.ERR_INVALID, "member 1 is null")
    refused(group_of([h, hm, h]), _lib.ERR_INVALID, "member 2 appears twice")
    refused(group_of([h, other_batch._handle.value]), _lib.ERR_INVALID, "member 1: the members of a group " + shape_text)
    refused(group_of([h, other_const._handle.value]), _lib.ERR_INVALID, "member 1: the members of a group " + shape_text)
    out = C.c_void_p()
    refused(create(C.byref(out), None, 1), _lib.ERR_INVALID, "null argument")

    # ---- train_steps, one trainer and a group of two ----
    stride = lib.iqlhip_replay_row_stride(S, A)
    torch.manual_seed(0)
    rows = torch.randn((N_ROWS, stride), dtype=torch.float32, device=DEV)
    idx = torch.zeros((3, B), dtype=torch.int64, device=DEV)
    good = _lib.ReplayView(rows.data_ptr(), N_ROWS, stride, S, A, 0)
    other_dims = _lib.ReplayView(rows.data_ptr(), N_ROWS, lib.iqlhip_replay_row_stride(S + 1, A), S + 1, A, 0)
    empty = _lib.ReplayView(rows.data_ptr(), 0, stride, S, A, 0)
    group = C.c_void_p()
    assert create(C.byref(group), (C.c_void_p * 2)(h, hm), 2) == 0 and group.value
    both = (C.c_void_p * 2)(idx.data_ptr(), idx.data_ptr())
    with torch.cuda.device(DEV):
        for view, idx_p, text in ((other_dims, idx.data_ptr(), "member 0: the replay view does not have the trainer's dims"),
                                  (empty, idx.data_ptr(), "member 0: empty replay view"),
                                  (good, None, "member 0: " + idx_text)):
            refused(train(lib, tr._handle, C.byref(view), 3, idx_p), _lib.ERR_INVALID, text)
        for view, idx_arr, text in ((other_dims, both, "member 1: the replay view does not have the trainer's dims"),
                                    (empty, both, "member 1: empty replay view"),
                                    (good, (C.c_void_p * 2)(idx.data_ptr(), None), "member 1: " + idx_text)):
            refused(gtrain(lib, group, (_lib.ReplayView * 2)(good, view), 3, idx_arr), _lib.ERR_INVALID, text)
        refused(gtrain(lib, group, None, 3, both), _lib.ERR_INVALID, "null views or indices")
        refused(train(lib, tr._handle, C.byref(good), -1, idx.data_ptr()), _lib.ERR_INVALID, "n_steps must be >= 0")
    torch.cuda.synchronize()
    assert destroy(group) == 0

    # ---- the library's own step count did not move ----
    class View:  # (what ``train_steps`` asks of a replay buffer)
        def view(self):
            return good
    kw = {"eps": torch.zeros((1, 2, B, A), dtype=torch.float32, device=DEV)} if name == "awac" else {}
    got, want = (t.train_steps(View(), 1, B, indices=idx[:1], **kw) for t in (tr, twin))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert tr.total_it == twin.total_it == 1 and not torch.equal(tr._params, mate._params)
    for arena in ("_params", "_exp_avg", "_exp_avg_sq"):
        assert torch.equal(getattr(tr, arena), getattr(twin, arena)), arena
