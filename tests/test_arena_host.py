"""``iqlpref_amd._arena``: what an arena-backed trainer is, on CPU tensors against torch's own Adam.  No library, no
GPU: binding parameters into a flat arena, adopting and binding Adam state, the index check and the plain-Adam check.
(The device check of ``check_indices`` runs in tests/test_gpu_bc_step.py.)"""
import copy

import pytest
import torch

from iqlpref_amd import _arena

STEPS = 3


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.ReLU(), torch.nn.Linear(4, 4), torch.nn.ReLU(),
                               torch.nn.Linear(4, 2))  # 3 in, 4 hidden, 2 out: six tensors, as a trainer's actor has


def _step(net, optimizers, steps=STEPS):
    torch.manual_seed(5)
    for _ in range(steps):
        x = torch.randn(8, 3)
        for opt in optimizers:
            opt.zero_grad()
        net(x).square().mean().backward()
        for opt in optimizers:
            opt.step()


def _layout(params):
    """Offsets with a gap of 3 floats behind every tensor (an arena need not be dense), and the arena size."""
    offsets, n = [], 0
    for p in params:
        offsets.append(n)
        n += p.numel() + 3
    return offsets, n


def _same_state_dict(got, want):
    assert got["param_groups"] == want["param_groups"]
    assert list(got["state"]) == list(want["state"])
    for i, st in want["state"].items():
        assert list(got["state"][i]) == list(st) == ["step", "exp_avg", "exp_avg_sq"]
        for k, v in st.items():
            g = got["state"][i][k]
            assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), (i, k)
        step = got["state"][i]["step"]
        assert step.dtype == torch.float32 and step.dim() == 0 and step.item() == float(STEPS)


@pytest.fixture(scope="module")
def stepped():
    """(reference net, its Adam) after STEPS steps, unbound: what everything is compared with.  Left unchanged."""
    ref = _net()
    ref_opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    _step(ref, [ref_opt])
    return ref, ref_opt


def test_bound_parameters_step_like_unbound_ones(stepped):
    ref, _ = stepped
    net = _net()
    params = list(net.parameters())
    assert len(params) == 6
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    offsets, n = _layout(params)
    arena, grads = torch.full((n,), 7.0), torch.zeros(n)
    views = _arena.bind_parameters(arena, params, offsets, grads)
    assert [id(p) for p, _ in views] == [id(p) for p in params] and [o for _, o in views] == offsets
    assert all(a is b for a, b in zip(net.parameters(), params))
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], params))
    for p, o in views:  # (the kernels write gradients there; torch's own backward below makes tensors of its own)
        assert p.grad.shape == p.shape and p.grad.data_ptr() == grads[o:].data_ptr()
    _step(net, [opt])
    for p, q, o in zip(params, ref.parameters(), offsets):
        assert torch.equal(p, q)
        assert torch.equal(arena[o:o + p.numel()].view(p.shape), q)          # the arena holds them
        assert p.data_ptr() == arena[o:].data_ptr()
        assert torch.equal(arena[o + p.numel():o + p.numel() + 3], torch.full((3,), 7.0))  # and nothing beside
    # without a gradient arena p.grad is left alone
    lone = torch.nn.Parameter(torch.ones(2))
    _arena.bind_parameters(torch.zeros(2), [lone], [0])
    assert lone.grad is None and torch.equal(lone, torch.ones(2))


@pytest.mark.parametrize("split", [False, True])
def test_adopted_and_bound_adam_state_is_torchs(stepped, split):
    """One optimiser over all parameters, or two over disjoint halves: the moments go into the arenas and come
    back as views; every ``state_dict()`` equals the unbound optimiser's over the same parameters."""
    ref, ref_opt = stepped
    net = copy.deepcopy(ref)
    params = list(net.parameters())
    halves = [params[:2], params[2:]] if split else [params]
    opts = [torch.optim.Adam(h, lr=1e-2) for h in halves]
    want = []
    lo = 0
    for opt, h in zip(opts, halves):  # the stepped state of the reference, cut to this optimiser's parameters
        sd = copy.deepcopy(ref_opt.state_dict())
        sd["state"] = {i - lo: v for i, v in sd["state"].items() if lo <= i < lo + len(h)}
        sd["param_groups"][0]["params"] = list(range(len(h)))
        opt.load_state_dict(copy.deepcopy(sd))
        want.append(sd)
        lo += len(h)
    offsets, n = _layout(params)
    views = list(zip(params, offsets))
    m, v = torch.full((n,), 9.0), torch.full((n,), 9.0)  # stale contents: adopting zeroes them first
    assert _arena.adopt_adam_state(views, opts, m, v) == STEPS
    for p, o in views:
        assert torch.equal(m[o + p.numel():o + p.numel() + 3], torch.zeros(3))
    steps = _arena.bind_adam_state(views, opts, m, v, STEPS)
    assert len(steps) == len(params)
    for opt, sd in zip(opts, want):
        _same_state_dict(opt.state_dict(), sd)
    for (p, o), q in zip(views, ref.parameters()):
        opt = opts[-1] if split and o >= offsets[2] else opts[0]
        assert opt.state[p]["exp_avg"].data_ptr() == m[o:].data_ptr()
        assert opt.state[p]["exp_avg_sq"].data_ptr() == v[o:].data_ptr()
        assert torch.equal(opt.state[p]["exp_avg"], ref_opt.state[q]["exp_avg"])
    # the returned tensors are the counters: moving them moves what state_dict() writes
    for st in steps:
        st.fill_(4.0)
    assert all(s["step"].item() == 4.0 for opt in opts for s in opt.state_dict()["state"].values())


def test_an_optimizer_that_has_not_stepped():
    net = _net()
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    offsets, n = _layout(params)
    views = list(zip(params, offsets))
    m, v = torch.ones(n), torch.ones(n)
    assert _arena.adopt_adam_state(views, [opt], m, v) is None
    assert not m.any() and not v.any()
    assert opt.state_dict()["state"] == {}  # nothing until bound
    _arena.bind_adam_state(views, [opt], m, v, 0)
    state = opt.state_dict()["state"]
    assert list(state) == [0, 1, 2, 3, 4, 5] and all(s["step"].item() == 0.0 and not s["exp_avg"].any() for s in state.values())


def test_check_indices():
    good = torch.zeros((3, 5), dtype=torch.int64)
    for bad in (good.to(torch.int32), good[:2], good[:, :4], good.reshape(-1), None):
        with pytest.raises(ValueError, match="indices must be an int64 device tensor"):
            _arena.check_indices(bad, 3, 5, True)
    with pytest.raises(ValueError, match="my words"):
        _arena.check_indices(good.to(torch.int32), 3, 5, False, "my words")
    assert _arena.check_indices(None, 3, 5, False) is None
    # dtype and shape right, but on the host: refused too (with a GPU tensor: tests/test_gpu_bc_step.py)
    with pytest.raises(ValueError, match="indices must be an int64 device tensor .* host"):
        _arena.check_indices(good, 3, 5, True)
    # where the host counts as the device (only here): a strided tensor comes back contiguous and equal, a
    # contiguous one as the same object
    cut = torch.arange(30, dtype=torch.int64).reshape(3, 10)[:, ::2]
    out = _arena.check_indices(cut, 3, 5, True, device_type="cpu")
    assert not cut.is_contiguous() and out.is_contiguous() and torch.equal(out, cut)
    assert _arena.check_indices(good, 3, 5, False, device_type="cpu") is good


def test_check_plain_adam():
    p = [torch.nn.Parameter(torch.zeros(2))]
    _arena.check_plain_adam([torch.optim.Adam(p), torch.optim.Adam(p, lr=1.0, betas=(0.5, 0.6), eps=1e-3)], "no")
    for bad in (torch.optim.Adam(p, weight_decay=1e-2), torch.optim.Adam(p, amsgrad=True),
                torch.optim.Adam(p, maximize=True), torch.optim.SGD(p, lr=0.1)):
        with pytest.raises(NotImplementedError, match="plain Adam only"):
            _arena.check_plain_adam([torch.optim.Adam(p), bad], "plain Adam only")
