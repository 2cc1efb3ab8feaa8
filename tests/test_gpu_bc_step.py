"""The behaviour-cloning step (csrc/bc_step.hip: k_bc_fwd_bwd / k_bc_update) over its envelope.  -m gpu.

``BC.train_steps`` with injected indices, three steps per case, every step judged at the GPU's own parameters of
the step before (the scheme of tests/test_gpu_general_step_envelope.py): before and after a step the test reads
the parameters, the Adam moments (``optimizer.state``) and ``p.grad``; the reference of step t is evaluated at
what the GPU held BEFORE step t, so the two sides never drift apart.  Step 1 runs on the copies made at creation,
steps 2 and 3 on the copies k_bc_update wrote.

Shapes (S, A, B): (45, 24, 64), (17, 6, 17), (96, 32, 48), (3, 1, 1), (45, 24, 256) -- tests/minari_cases.py.  The
mean is over the B x A real elements.  Padding rows must contribute nothing: every dataset row that no index
names holds 1e30, and the memory right behind each step's B indices names such rows, so a kernel that filled its
last slab by reading on, or from row 0, would produce inf.

Compared per step: the loss, every gradient, both Adam moments and the new value of every parameter, and -- bit
for bit against the new parameters -- the padded forward copies and the transposed copies the next step reads.
Bound per tensor: 4 x the largest |fp32 torch - float64 torch| of that tensor on the same inputs, both computed
here (tests/minari_cases.py: autograd of the reference's modules' arithmetic; ``torch.optim.Adam`` itself), floored
at the tensor's fp32 rounding unit at its largest entry.  For the loss and the gradients the same inputs are the
GPU's parameters and the batch; for the moments and the new parameters they are the GPU's own p0, m0, v0 and
gradient.  The only thing left out are the (row, hidden unit) pairs whose float64 pre-activation is within 1e-5 of
zero: relu' of such a pair may fall either way in fp32, so what the pair can contribute to each gradient entry
(|gradient with relu' = 1 on those pairs - gradient with relu' = 0|, float64) is added to that entry's bound.
Their share is asserted to stay under 1 in 1,000 per step (tests/test_bc_step_host.py shows it for the float64
restatement alone); with no such pair nothing is added.  Every figure is printed (IQLTEST lines with -s).

An MI355X gave, as the largest error / bound over the five cases and three steps: loss 0.75, gradients 0.81
(net.4.bias of the one-row case; 0.65 elsewhere), new parameters 0.25, exp_avg 0.25, exp_avg_sq 0.94; every copy
equal to the new parameters bit for bit; at most 4 pairs of a step near a kink (3e-5 of them), no inf or nan.

Below the step cases: the life of handles and groups (a ``BCGroup`` whose members change batch size, are closed,
deleted and stepped on alone, bit for bit against twins stepped alone), and the refusal of host ``indices`` by both
trainer families and ``SeedGroup`` before anything is launched.
"""
import numpy as np
import pytest
import torch

from tests import minari_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _say(line):
    print("IQLTEST bc-step " + line)


def _trainer(case, keep_grads=True):
    from iqlpref_amd import custom_offline as co, minari_bc
    S, A, B, max_action, params, data, idx, poison = mc.bc_case_inputs(case)
    actor = minari_bc.Actor(S, A, max_action)
    actor.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    actor = actor.to(DEV)
    tr = minari_bc.BC(max_action, actor, torch.optim.Adam(actor.parameters(), lr=mc.LR), DEV, keep_grads=keep_grads)
    buf = co.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_dataset(data)
    return tr, buf, (S, A, B, max_action, data, idx)


def _read(tr):
    torch.cuda.synchronize()
    named = dict(tr.actor.named_parameters())
    p = {k: v.detach().cpu().numpy().copy() for k, v in named.items()}
    m, v = {}, {}
    for k, par in named.items():
        st = tr.actor_optimizer.state.get(par) or {}
        m[k], v[k] = (st[x].detach().cpu().numpy().copy() if x in st else np.zeros(tuple(par.shape), np.float32)
                      for x in ("exp_avg", "exp_avg_sq"))
    return p, m, v


@pytest.mark.parametrize("case", list(mc.CASES))
def test_step_at_the_gpus_own_parameters(case):
    tr, buf, (S, A, B, max_action, data, idx) = _trainer(case)
    idx_t = torch.from_numpy(idx).to(DEV)
    failures = []
    for t in range(mc.STEPS):
        p0, m0, v0 = _read(tr)
        # (a view of the index row: the poisoned indices lie right behind the B real ones in memory)
        loss = tr.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B))
        p1, m1, v1 = _read(tr)
        loss = float(loss.cpu()[0, 0])
        grads = {k: par.grad.detach().cpu().numpy().copy() for k, par in tr.actor.named_parameters()}
        assert tr.total_it == t + 1
        rows = idx[t, :B]
        s, a = data["observations"][rows], data["actions"][rows]
        l64, g64, zs = mc.bc_forward_backward(p0, s, a, max_action, torch.float64)
        l32, g32, _ = mc.bc_forward_backward(p0, s, a, max_action, torch.float32)
        near = mc.near_kink(zs)
        n_near = sum(int(x.sum()) for x in near)
        share = n_near / sum(x.size for x in near)
        assert share <= mc.KINK_CAP, f"{case} step {t + 1}: {share} of the pairs within {mc.KINK} of a kink"
        extra = {k: 0.0 for k in g64}
        if n_near:
            on = mc.bc_forward_backward(p0, s, a, max_action, torch.float64, force=(*near, 1.0))[1]
            off = mc.bc_forward_backward(p0, s, a, max_action, torch.float64, force=(*near, 0.0))[1]
            extra = {k: np.abs(on[k] - off[k]) for k in g64}
        # 1. the loss
        ratio, bound = mc.judge(loss, l64, l32)
        _say(f"{case} step {t + 1}: loss {loss!r} against {l64!r}: {ratio:.3f} of its bound {bound:.2e}; "
             f"{n_near} pairs near a kink ({share:.1e})")
        if not (np.isfinite(loss) and ratio <= 1):
            failures.append(f"step {t + 1} loss: {loss!r} against {l64!r}, {ratio:.2f} of the bound {bound:.2e}")
        # 2. every gradient
        worst = {}
        for k in mc.NAMES:
            _, bound = mc.judge(grads[k], g64[k], g32[k])
            err = np.abs(grads[k].astype(np.float64) - g64[k])
            ratio = float(np.max(err / (bound + extra[k]))) if np.all(np.isfinite(err)) else np.inf
            worst["grad " + k] = ratio
            if not ratio <= 1:
                failures.append(f"step {t + 1} gradient {k}: {ratio:.2f} of the bound {bound:.2e} "
                                f"(largest entry {np.abs(g64[k]).max():.2e})")
        # 3. the update, from the GPU's own numbers
        for k in mc.NAMES:
            want = mc.adam_step(p0[k], m0[k], v0[k], grads[k], t + 1, torch.float64)
            f32 = mc.adam_step(p0[k], m0[k], v0[k], grads[k], t + 1, torch.float32)
            for what, got, w64, w32 in zip(("parameter", "exp_avg", "exp_avg_sq"), (p1[k], m1[k], v1[k]), want, f32):
                ratio, bound = mc.judge(got, w64, w32)
                worst[f"{what} {k}"] = ratio
                if not ratio <= 1:
                    failures.append(f"step {t + 1} {what} {k}: {ratio:.2f} of the bound {bound:.2e}")
        _say(f"{case} step {t + 1}: error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        # 4. the copies the next step reads: the new parameters bit for bit, zero padding
        copies = {k: v.cpu().numpy() for k, v in tr.weight_copies().items()}
        S16, A16 = copies["w1"].shape[1], copies["w3"].shape[0]
        pad = lambda w, shape: np.pad(w, [(0, n - d) for n, d in zip(shape, w.shape)])
        want = {"w1": pad(p1["net.0.weight"], (mc.H, S16)), "w2": p1["net.2.weight"],
                "w3": pad(p1["net.4.weight"], (A16, mc.H)), "w2t": p1["net.2.weight"].T,
                "w3t": pad(p1["net.4.weight"], (A16, mc.H)).T}
        for k, w in want.items():
            if not np.array_equal(copies[k].view(np.uint32), np.ascontiguousarray(w).view(np.uint32)):
                failures.append(f"step {t + 1} copy {k}: {int((copies[k] != w).sum())} entries differ from the new parameters")
    assert not failures, f"{case}:\n  " + "\n  ".join(failures)


def test_train_on_an_explicit_batch_is_the_same_step():
    """``BC.train(batch)`` (bcref:230-243) = ``train_steps`` on the same rows, bit for bit, and returns the
    reference's one-entry dict."""
    case = "s17_a6_b17"
    tr_a, buf, (S, A, B, max_action, data, idx) = _trainer(case, keep_grads=False)
    tr_b, _, _ = _trainer(case, keep_grads=False)
    rows = torch.from_numpy(idx[0, :B]).to(DEV)
    la = tr_a.train_steps(buf, 1, B, indices=rows.view(1, B)).item()
    s, a = (torch.from_numpy(data[k][idx[0, :B]]).to(DEV) for k in ("observations", "actions"))
    out = tr_b.train([s, a, None, None, None])
    assert list(out) == ["actor_loss"] and out["actor_loss"] == la
    for (k, p), q in zip(tr_a.actor.named_parameters(), tr_b.actor.parameters()):
        assert torch.equal(p, q), k
    assert sorted(tr_b.state_dict()) == ["actor", "actor_optimizer"]


def test_outside_the_envelope_is_refused_before_any_launch():
    from iqlpref_amd import minari_bc
    mk = lambda actor: minari_bc.BC(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), DEV)
    for S, A in ((129, 24), (45, 33), (200, 40)):
        with pytest.raises(NotImplementedError):
            mk(minari_bc.Actor(S, A, 1.0).to(DEV))
    narrow = minari_bc.Actor(45, 24, 1.0)
    narrow.net[0], narrow.net[2], narrow.net[4] = torch.nn.Linear(45, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 24)
    with pytest.raises(NotImplementedError):
        mk(narrow.to(DEV))
    uneven = minari_bc.Actor(45, 24, 1.0)
    uneven.net[0], uneven.net[2] = torch.nn.Linear(45, 128), torch.nn.Linear(128, 256)
    with pytest.raises(NotImplementedError):
        mk(uneven.to(DEV))
    actor = minari_bc.Actor(45, 24, 1.0).to(DEV)
    with pytest.raises(NotImplementedError):
        minari_bc.BC(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4, weight_decay=1e-2), DEV)
    with pytest.raises(TypeError):
        mk(torch.nn.Sequential(torch.nn.Linear(45, 24)).to(DEV))
    ok = mk(actor)
    with pytest.raises(NotImplementedError):
        minari_bc.BCGroup([ok] * 17)
    assert ok._handle is None  # nothing was created, nothing launched
    # the library itself: precision, width and depth are refused by the layout call, which touches no device
    import ctypes as C
    from iqlpref_amd import _lib
    lib = _lib.load()
    for field, value in (("precision", _lib.PREC_BF16), ("hidden_dim", 128), ("n_hidden", 3), ("dropout_p", 0.1),
                         ("state_dim", 129), ("action_dim", 33)):
        cfg = ok._cfg(64)
        setattr(cfg, field, value)
        offs, n = (C.c_int64 * 6)(), C.c_int64()
        assert lib.iqlhip_bc_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n)) == _lib.ERR_UNSUPPORTED, field
        h = C.c_void_p()
        ar = _lib.Arenas(1, 1, 1, None, None)  # (never dereferenced: the config is refused first)
        assert lib.iqlhip_bc_create(C.byref(h), C.byref(cfg), 1.0, C.byref(ar)) == _lib.ERR_UNSUPPORTED, field
    cfg = ok._cfg(0)
    assert lib.iqlhip_bc_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n)) == _lib.ERR_INVALID


# --------------------------------------------------------------------------- #
# the lifecycle of handles and groups
# --------------------------------------------------------------------------- #
def _lifecycle_inputs():
    """Two members of the shape of case ``s3_a1_b1`` (S 3, A 1): member 0 starts at the case's parameters, member 1
    at torch's initialisation under another seed.  Batch 1 steps on the case's own rows and indices; batch 17 on
    the rows and indices of case ``s17_a6_b17`` cut to the first 3 state columns and the first action column (its
    indices name unpoisoned rows only), member 1 on the same rows in reverse order."""
    S, A, B1, max_action, params, d1, i1, _ = mc.bc_case_inputs("s3_a1_b1")
    _, _, B17, _, _, d17, i17, _ = mc.bc_case_inputs("s17_a6_b17")
    cut = {k: np.ascontiguousarray(v[:, :S] if "observations" in k else v[:, :A] if k == "actions" else v)
           for k, v in d17.items()}
    torch.manual_seed(7)
    other = {"net." + k: v.detach().numpy().copy()
             for k, v in torch.nn.Sequential(torch.nn.Linear(S, mc.H), torch.nn.ReLU(), torch.nn.Linear(mc.H, mc.H),
                                             torch.nn.ReLU(), torch.nn.Linear(mc.H, A)).state_dict().items()}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    idx1, idx17 = up(i1[:, :B1]), up(i17[:, :B17])
    return S, A, max_action, (params, other), (d1, cut), ((B1, [idx1, idx1]), (B17, [idx17, up(i17[:, :B17][:, ::-1])]))


def _same(a, b, where=""):
    """Equal key for key; tensors bit for bit."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}/{i}")
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), where
    else:
        assert a == b, where


def _same_trainer(got, want, where):
    torch.cuda.synchronize()
    assert got.total_it == want.total_it, where
    for (k, p), q in zip(got.actor.named_parameters(), want.actor.parameters()):
        assert torch.equal(p, q), f"{where}: {k}"
    assert torch.equal(got._exp_avg, want._exp_avg) and torch.equal(got._exp_avg_sq, want._exp_avg_sq), where
    _same(got.state_dict(), want.state_dict(), where)


def test_group_lifecycle_matches_members_stepped_alone():
    """Two ``BC`` trainers as a ``BCGroup``: three steps at batch 1, three at batch 17 -- every member handle is
    rebuilt there, so the group is dissolved through its owner and built again -- against twins stepped alone
    through the same calls: losses, parameters, moments and ``state_dict()`` bit for bit.  Then the group is
    closed, one member is deleted while the other lives, and the survivor steps on alone like its twin."""
    import gc
    from iqlpref_amd import custom_offline as co, minari_bc
    S, A, max_action, params, datas, calls = _lifecycle_inputs()

    def build():
        out = []
        for p in params:
            actor = minari_bc.Actor(S, A, max_action)
            actor.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
            actor = actor.to(DEV)
            out.append(minari_bc.BC(max_action, actor, torch.optim.Adam(actor.parameters(), lr=mc.LR), DEV))
        return out

    bufs = []
    for d in datas:
        bufs.append(co.ReplayBuffer(S, A, len(d["observations"]), DEV))
        bufs[-1].load_dataset(d)
    members, twins = build(), build()
    group = minari_bc.BCGroup(members)
    handles = []
    for buf, (B, idx) in zip(bufs, calls):
        got = group.train_steps(buf, mc.STEPS, B, indices=idx, return_losses=True)
        want = [t.train_steps(buf, mc.STEPS, B, indices=i) for t, i in zip(twins, idx)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == (mc.STEPS, 1) and torch.equal(g, w), f"batch {B} member {k}"
            assert bool(torch.isfinite(g).all())
        assert all(t._group_owner is group and t._handle_batch == B for t in members)
        handles.append(group._group.value)
        for k, (m, t) in enumerate(zip(members, twins)):
            _same_trainer(m, t, f"batch {B} member {k}")
    assert all(t.total_it == 2 * mc.STEPS for t in members) and None not in handles
    assert not torch.equal(members[0]._params, members[1]._params)

    group.close()
    assert all(t._group_owner is None and t._handle is not None for t in members)
    survivor = members[1]
    del group, members
    gc.collect()
    (B, idx), buf = calls[1], bufs[1]
    got = survivor.train_steps(buf, 1, B, indices=idx[1][:1])
    want = twins[1].train_steps(buf, 1, B, indices=idx[1][:1])
    assert torch.equal(got, want)
    _same_trainer(survivor, twins[1], "the survivor")


@pytest.mark.parametrize("who", ["bc", "iql", "seed_group"])
def test_host_indices_are_refused_before_any_launch(who):
    """An ``indices`` tensor on the host is a ValueError of ``BC.train_steps``, ``ImplicitQLearning.train_steps``
    and ``SeedGroup.train_steps`` alike: nothing is launched and no step is counted."""
    if who == "bc":
        tr, buf, (S, A, B, _, _, idx) = _trainer("s17_a6_b17", keep_grads=False)
        good = torch.from_numpy(idx[:1, :B]).to(DEV)
        tr.train_steps(buf, 1, B, indices=good)
        before = tr._params.clone()
        with pytest.raises(ValueError, match="indices"):
            tr.train_steps(buf, 1, B, indices=good.cpu())
        torch.cuda.synchronize()
        assert tr.total_it == 1 and torch.equal(tr._params, before)
        return
    import iqlpref_amd as ia
    from tests import gpu_helpers, helpers
    d, hyper, data, nets = helpers.load_traj("traj_antmaze", "fp32")
    B = hyper["batch"]
    buf = gpu_helpers.make_buffer(hyper, data)
    good = torch.from_numpy(d["indices"][:1]).to(DEV)
    trs = [gpu_helpers.make_trainer(hyper, nets, "fp32", seed=s) for s in ((1,) if who == "iql" else (1, 2))]
    if who == "iql":
        stepped, step = trs[0], lambda i: trs[0].train_steps(buf, 1, B, indices=i)
    else:
        stepped = ia.SeedGroup(trs, mode="group")
        step = lambda i: stepped.train_steps(buf, 1, B, indices=[i, good])
    step(good)
    counts = [x.launch_counts() for x in [stepped] + trs]
    before = [t._params.clone() for t in trs]
    with pytest.raises(ValueError, match="indices"):
        step(good.cpu())
    torch.cuda.synchronize()
    assert [x.launch_counts() for x in [stepped] + trs] == counts
    assert all(t.total_it == 1 and torch.equal(t._params, p) for t, p in zip(trs, before))
    if who == "seed_group":
        stepped.close()
