"""What the TD3+BC family turns down before any launch, with the slab core's codes and texts (csrc/slab_step.h:
``slab_group_create``, ``slab_check_call``) -- modelled on tests/test_gpu_slab_refusals.py.  -m gpu.

From Python: an index tensor on the host, eps of another shape or on the host, shapes outside the envelope, an
optimiser that is not plain Adam, a policy_freq below 1, a group of 17.  Through ctypes straight on the handles
(``TD3BCGroup`` refuses most of it before the library sees it): group create with 0 and 17 members, a null member, a
member listed twice, members that differ in batch size or in shape -- members that differ in their hyperparameters
only are NOT refused: every one is the member's own --; ``train_steps`` of one trainer and of a group on a view of other
dims, a view of 0 rows, null indices, a negative step count.  Every refusal comes back before any launch and the step
counts did not move: after all of them one step from the trainer equals, bit for bit, the same step of a twin that saw
none.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import td3_bc_cases as tc

pytestmark = pytest.mark.gpu
DEV, S, A, H = "cuda:0", 3, 1, 16
N_ROWS = 8


def _params(S_, H_, seed):
    torch.manual_seed(seed)
    named = lambda m: {"net." + n: v.detach().numpy().copy() for n, v in m.state_dict().items()}
    return {"actor": named(tc.mlp(S_, H_, A)), "critic_1": named(tc.mlp(S_ + A, H_, 1)), "critic_2": named(tc.mlp(S_ + A, H_, 1))}


def _trainer(batch, seed=0, S_=S, H_=H, **over):
    tr = tc.build_trainer(S_, A, H_, _params(S_, H_, seed), tc.hyper("s3_a1_b1_h16"), seed=seed, keep_grads=False, **over)
    tr._ensure_handle(batch)
    return tr


def test_python_surface_refuses_before_anything_is_created():
    from iqlpref_amd import td3_bc
    adam = lambda m, **kw: torch.optim.Adam(m.parameters(), lr=3e-4, **kw)

    def mk(S_, A_, H_, policy_freq=2, **kw):
        a, c1, c2 = td3_bc.Actor(S_, A_, 1.0, H_).to(DEV), td3_bc.Critic(S_, A_, H_).to(DEV), td3_bc.Critic(S_, A_, H_).to(DEV)
        return td3_bc.TD3_BC(1.0, a, adam(a, **kw), c1, adam(c1), c2, adam(c2), policy_freq=policy_freq, device=DEV)

    for S_, A_, H_ in ((129, 6, 64), (17, 33, 64), (17, 6, 24), (17, 6, 272)):
        with pytest.raises(NotImplementedError):
            mk(S_, A_, H_)
    with pytest.raises(NotImplementedError):
        mk(17, 6, 64, weight_decay=1e-2)
    with pytest.raises(NotImplementedError):
        mk(17, 6, 64, betas=(0.8, 0.999))
    with pytest.raises(NotImplementedError):
        mk(17, 6, 64, policy_freq=0)
    ok = mk(17, 6, 32)
    assert ok._handle is None  # nothing was created, nothing launched
    with pytest.raises(NotImplementedError):
        td3_bc.TD3BCGroup([ok] * 17)
    host = torch.zeros((1, 16), dtype=torch.int64)
    buf = td3_bc.ReplayBuffer(17, 6, 4, DEV)
    buf.load_d4rl_dataset({"observations": np.zeros((4, 17), np.float32), "actions": np.zeros((4, 6), np.float32),
                           "rewards": np.zeros(4, np.float32), "next_observations": np.zeros((4, 17), np.float32),
                           "terminals": np.zeros(4, np.float32)})
    with pytest.raises(ValueError, match="indices"):
        ok.train_steps(buf, 1, 16, indices=host)
    dev = host.to(DEV)
    for eps in (torch.zeros((1, 16, 6)), torch.zeros((1, 2, 16, 6), device=DEV), torch.zeros((1, 16, 5), device=DEV),
                torch.zeros((2, 16, 6), device=DEV), torch.zeros((1, 16, 6), device=DEV, dtype=torch.float64)):
        with pytest.raises(ValueError, match="eps"):
            ok.train_steps(buf, 1, 16, indices=dev, eps=eps)
    group = td3_bc.TD3BCGroup([ok, mk(17, 6, 32)])
    with pytest.raises(ValueError, match="eps"):
        group.train_steps(buf, 1, 16, indices=[dev, dev], eps=[None, torch.zeros((1, 16, 5), device=DEV)])
    with pytest.raises(ValueError, match="indices"):
        group.train_steps(buf, 1, 16, indices=[dev, host])
    assert ok._handle is None and ok.total_it == 0 and group._group is None


def test_library_refusals_come_back_before_any_launch():
    from iqlpref_amd import _lib
    lib = _lib.load()
    create, destroy = lib.iqlhip_td3bc_group_create, lib.iqlhip_td3bc_group_destroy
    train = lambda h, view, n, idx: lib.iqlhip_td3bc_train_steps(h, view, n, idx, None, None, None)
    gtrain = lambda g, views, n, idx: lib.iqlhip_td3bc_group_train_steps(g, views, n, idx, None, None, None)
    B = 1
    tr, twin, mate = _trainer(B), _trainer(B), _trainer(B, seed=1, alpha=1.0, policy_freq=3, max_action=2.0)
    other_batch, other_width, other_dims = _trainer(17, seed=2), _trainer(B, seed=3, H_=32), _trainer(B, seed=4, S_=4)
    everyone = (tr, twin, mate, other_batch, other_width, other_dims)
    shape_text = "member 1: the members of a group share dims, width and batch size"

    def refused(rc, code, text):
        msg = lib.iqlhip_last_error().decode()
        assert rc == code and text in msg, (rc, msg)
        assert all(t.total_it == 0 and t._actor_it == 0 for t in everyone)

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
    for other in (other_batch, other_width, other_dims):
        refused(group_of([h, other._handle.value]), _lib.ERR_INVALID, shape_text)
    out = C.c_void_p()
    refused(create(C.byref(out), None, 1), _lib.ERR_INVALID, "null argument")

    stride = lib.iqlhip_replay_row_stride(S, A)
    torch.manual_seed(0)
    rows = torch.randn((N_ROWS, stride), dtype=torch.float32, device=DEV)
    idx = torch.zeros((3, B), dtype=torch.int64, device=DEV)
    good = _lib.ReplayView(rows.data_ptr(), N_ROWS, stride, S, A, 0)
    wrong = _lib.ReplayView(rows.data_ptr(), N_ROWS, lib.iqlhip_replay_row_stride(S + 1, A), S + 1, A, 0)
    empty = _lib.ReplayView(rows.data_ptr(), 0, stride, S, A, 0)
    group = C.c_void_p()
    # (members that differ in alpha, policy_freq and max_action share a group: those are each member's own)
    assert create(C.byref(group), (C.c_void_p * 2)(h, hm), 2) == 0 and group.value
    both = (C.c_void_p * 2)(idx.data_ptr(), idx.data_ptr())
    with torch.cuda.device(DEV):
        for view, idx_p, text in ((wrong, idx.data_ptr(), "member 0: the replay view does not have the trainer's dims"),
                                  (empty, idx.data_ptr(), "member 0: empty replay view"),
                                  (good, None, "member 0: TD3+BC takes its indices")):
            refused(train(tr._handle, C.byref(view), 3, idx_p), _lib.ERR_INVALID, text)
        for view, idx_arr, text in ((wrong, both, "member 1: the replay view does not have the trainer's dims"),
                                    (empty, both, "member 1: empty replay view"),
                                    (good, (C.c_void_p * 2)(idx.data_ptr(), None), "member 1: TD3+BC takes its indices")):
            refused(gtrain(group, (_lib.ReplayView * 2)(good, view), 3, idx_arr), _lib.ERR_INVALID, text)
        refused(gtrain(group, None, 3, both), _lib.ERR_INVALID, "null views or indices")
        refused(train(tr._handle, C.byref(good), -1, idx.data_ptr()), _lib.ERR_INVALID, "n_steps must be >= 0")
    torch.cuda.synchronize()
    assert destroy(group) == 0

    class View:  # (what ``train_steps`` asks of a replay buffer)
        def view(self):
            return good
    eps = torch.zeros((2, B, A), dtype=torch.float32, device=DEV)
    idx2 = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    got, want = (t.train_steps(View(), 2, B, indices=idx2, eps=eps) for t in (tr, twin))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert tr.total_it == twin.total_it == 2 and tr._actor_it == 1 and not torch.equal(tr._params, mate._params)
    for arena in ("_params", "_target", "_exp_avg", "_exp_avg_sq"):
        assert torch.equal(getattr(tr, arena), getattr(twin, arena)), arena
