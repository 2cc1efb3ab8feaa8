"""The AWAC step (csrc/awac_step.hip: k_awac_critic_fwd_bwd / k_awac_critic_update / k_awac_actor_fwd_bwd /
k_awac_actor_update) over its envelope.  -m gpu.

``AdvantageWeightedActorCritic.train_steps`` with injected indices and standard normals, three steps per case,
every step judged at the GPU's own parameters of the step before (the scheme of tests/test_gpu_bc_step.py): the
critic half of the update is restated at what the GPU held BEFORE the step, the actor half at the GPU's old actor
and its NEW critics (awac:301-304: the actor loss reads the critics just updated), Adam from the GPU's own p0, m0,
v0 and gradient, the targets from the GPU's old targets and new critics.  Step 1 runs on the copies made at
creation, steps 2 and 3 on the copies the update kernels wrote.

Shapes (S, A, B, H): (3, 1, 1, 16), (17, 6, 17, 256), (45, 24, 64, 64) at lambda 0.1 (some weights at the cap of
100, some below), (96, 32, 48, 128), (29, 8, 256, 256) -- tests/awac_cases.py.  Every dataset row that no index
names holds 1e30 in every column, and the memory right behind each step's B indices names such rows.

Compared per step: both losses, every gradient of the three networks and of ``_log_std`` (entry 0 of the 17-row
case lies beyond the clamp: exactly zero), both Adam moments and every new parameter.  Bound per tensor: 4 x the
largest |fp32 torch - float64 torch| of that tensor on the same inputs, floored at the tensor's fp32 rounding unit
at its largest entry; for the losses and the gradients the fp32 side is the largest gap over eight summation orders of
the same restatement (the hidden units of every network permuted: ``awac_cases.fp32_gap`` has the reason -- one fp32
evaluation is one sample of the fp32 error, and a one-entry tensor has nothing else); for the (row, hidden unit)
pairs of a differentiated network whose float64 pre-activation is within 1e-5 of zero, what the pair can contribute to each gradient entry is added to that entry's bound, and their
share stays under 1 in 1,000.  Bit for bit: the forward and transposed copies of all five networks against the
new parameters and targets, the targets against the numpy-float32 evaluation of awac:215 at the GPU's own values,
and the eps read back against the eps injected.  No inf or nan anywhere.  Every ratio is printed (IQLTEST lines
with -s).

An MI355X gave, as the largest error / bound over the five cases and three steps: critic_loss 0.25, actor_loss 0.25,
gradients 0.32, new parameters 0.26, exp_avg 0.25, exp_avg_sq 0.98; every copy and every target bit for bit; at most
20 pairs of a step near a kink (7.2e-5 of them), 10 to 15 of the 64 weights of the lambda case at the cap, no inf or
nan.  (With ONE fp32 evaluation as the fp32 side, an earlier version of this test had the gradient of a critic's last
bias -- a one-entry tensor -- at 4.80 of its bound in step 1 of the 17-row case: 3.6e-8 off at a value of 0.104, where
torch's own fp32 lies up to 3.6e-8 off, depending on the summation order.)  The device's noise equalled the numpy
restatement in all 12,288 entries (0.00 spacings), mean +0.0064 (bound 0.0451), var - 1 +0.0058 (bound 0.0638).

Noise drawn on the device (the (29, 8, 256, 256) case): a step with ``eps=None``, its eps read back, equals bit
for bit a twin stepped with those eps injected; the eps equal a numpy Box-Muller restatement on ``oracle.philox``.
The kernel evaluates log, sqrt, sinpi and cospi in float64 and rounds once, so what separates it from numpy's
float64 evaluation is the libm error of both sides (a few 1e-16 relative) -- nothing fp32 can show except where
the two float64 values straddle a rounding boundary: the bound is one fp32 spacing at the value, and the test
prints the largest difference in spacings and how many entries differ at all.  (The step the issue describes -- measure
the device's fp32 log / sin / cos error against float64, bound at 4 x it, record it -- is dropped: the kernel has no
fp32 transcendental to measure, and the bound used is the tighter one.)  Over the n values drawn,
|mean| <= 5 / sqrt(n) and |var - 1| <= 5 sqrt(2 / n); the eps differ between steps and between the two streams.

Group: three members with their own parameters and data stepped as one ``AWACGroup`` -- at batch 1, then at batch
17, where every member handle is rebuilt and the group with them -- match twins stepped alone bit for bit.  The
members of a group share their batch size (``iqlhip_awac_group_create`` refuses anything else, as the BC group
does): "different batch sizes" is covered as a change of the whole group over time, never across members.  Then the
group is closed, two members are deleted and the survivor steps on like its twin.
"""
import gc

import numpy as np
import pytest
import torch

from tests import awac_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _say(line):
    print("IQLTEST awac-step " + line)


def _build(S, A, H, params, lam, seed=0, keep_grads=True, tau=ac.TAU):
    from iqlpref_amd import awac
    actor, c1, c2 = awac.Actor(S, A, H), awac.Critic(S, A, H), awac.Critic(S, A, H)
    for m, n in ((actor, "actor"), (c1, "critic_1"), (c2, "critic_2")):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        m.to(DEV)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=ac.LR)
    tr = awac.AdvantageWeightedActorCritic(actor, adam(actor), c1, adam(c1), c2, adam(c2), gamma=ac.GAMMA, tau=tau,
                                           awac_lambda=lam, seed=seed, keep_grads=keep_grads)
    if "target_critic_1" in params:
        with torch.no_grad():
            for m, n in ((tr._target_critic_1, "target_critic_1"), (tr._target_critic_2, "target_critic_2")):
                for k, p in m.named_parameters():
                    p.copy_(torch.from_numpy(params[n][k]))
    return tr


def _trainer(case, **kw):
    from iqlpref_amd import awac
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
    tr = _build(S, A, H, params, lam, **kw)
    buf = awac.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_d4rl_dataset(data)
    return tr, buf, (S, A, B, H, lam, data, idx, eps)


def _modules(tr):
    return {"actor": tr._actor, "critic_1": tr._critic_1, "critic_2": tr._critic_2,
            "target_critic_1": tr._target_critic_1, "target_critic_2": tr._target_critic_2}


def _read(tr):
    torch.cuda.synchronize()
    p, m, v = {}, {}, {}
    opts = dict(zip(ac.TRAINED, tr._optimizers))
    for n, mod in _modules(tr).items():
        p[n] = {k: x.detach().cpu().numpy().copy() for k, x in mod.named_parameters()}
        if n not in opts:
            continue
        m[n], v[n] = {}, {}
        for k, par in mod.named_parameters():
            st = opts[n].state.get(par) or {}
            m[n][k], v[n][k] = (st[x].detach().cpu().numpy().copy() if x in st else np.zeros(tuple(par.shape), np.float32)
                                for x in ("exp_avg", "exp_avg_sq"))
    return p, m, v


def _grads(tr):
    return {f"{n}.{k}": par.grad.detach().cpu().numpy().copy() for n, mod in _modules(tr).items() if n in ac.TRAINED
            for k, par in mod.named_parameters()}


def _kink_extra(half, args, zs, g64, kw):
    near = ac.near_kink(zs)
    n_near = sum(int(x.sum()) for x in near)
    extra = {k: 0.0 for k in g64}
    if n_near:
        on = half(*args, torch.float64, force=(near, 1.0), **kw)[1]
        off = half(*args, torch.float64, force=(near, 0.0), **kw)[1]
        extra = {k: np.abs(on[k] - off[k]) for k in g64}
    return n_near, sum(x.size for x in near), extra


@pytest.mark.parametrize("case", list(ac.CASES))
def test_step_at_the_gpus_own_parameters(case):
    tr, buf, (S, A, B, H, lam, data, idx, eps) = _trainer(case)
    idx_t, eps_t = torch.from_numpy(idx).to(DEV), torch.from_numpy(eps).to(DEV)
    failures, r16 = [], lambda x: -(-x // 16) * 16
    for t in range(ac.STEPS):
        p0, m0, v0 = _read(tr)
        # (a view of the index row: the poisoned indices lie right behind the B real ones in memory)
        losses = tr.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=eps_t[t:t + 1])
        p1, m1, v1 = _read(tr)
        losses = losses.cpu().numpy()[0]
        grads = _grads(tr)
        assert tr.total_it == t + 1
        assert np.array_equal(tr.last_eps().cpu().numpy().view(np.uint32), eps[t].view(np.uint32))
        batch = ac.batch_of(data, idx[t, :B])
        worst = {}

        def check(what, got, w64, w32=None, extra=0.0, gap=None):
            _, bound = ac.judge(got, w64, w32) if gap is None else ac.judge_gap(got, w64, gap)
            err = np.abs(np.asarray(got, np.float64) - np.asarray(w64, np.float64))
            ratio = float(np.max(err / (bound + extra))) if np.all(np.isfinite(err)) else np.inf
            worst[what] = ratio
            if not ratio <= 1:
                failures.append(f"step {t + 1} {what}: {ratio:.2f} of the bound {bound:.2e}")

        # 1. the critic half at the GPU's old parameters
        cnets = (p0["actor"], p0["critic_1"], p0["critic_2"], p0["target_critic_1"], p0["target_critic_2"])
        cargs = cnets + (batch, eps[t, 0])
        lc64, gc64, zc, _ = ac.critic_half(*cargs, torch.float64)
        lc_gap, gc_gap = ac.fp32_gap(ac.critic_half, cnets, (batch, eps[t, 0]), {"critic_1": 1, "critic_2": 2}, lc64, gc64)
        near_c, pairs_c, extra_c = _kink_extra(ac.critic_half, cargs, zc, gc64, {})
        # 2. the actor half at the GPU's old actor and NEW critics
        anets = (p0["actor"], p1["critic_1"], p1["critic_2"])
        aargs = anets + (batch, eps[t, 1], lam)
        la64, ga64, za, xa = ac.actor_half(*aargs, torch.float64)
        la_gap, ga_gap = ac.fp32_gap(ac.actor_half, anets, (batch, eps[t, 1], lam), {"actor": 0}, la64, ga64)
        near_a, pairs_a, extra_a = _kink_extra(ac.actor_half, aargs, za, ga64, {})
        share = (near_c + near_a) / (pairs_c + pairs_a)
        assert share <= ac.KINK_CAP, f"{case} step {t + 1}: {share} of the pairs within {ac.KINK} of a kink"
        assert np.all(np.isfinite(losses))
        check("critic_loss", losses[0], lc64, gap=lc_gap)
        check("actor_loss", losses[1], la64, gap=la_gap)
        g64, ggap, extra = {**gc64, **ga64}, {**gc_gap, **ga_gap}, {**extra_c, **extra_a}
        for k in g64:
            check("grad " + k, grads[k], g64[k], extra=extra[k], gap=ggap[k])
        if case == "s17_a6_b17_h256":  # beyond the clamp: the derivative is 0, not small
            assert grads["actor._log_std"][0] == 0.0 and ga64["actor._log_std"][0] == 0.0
        # 3. the updates, from the GPU's own numbers
        for n in ac.TRAINED:
            for k in p0[n]:
                g = grads[f"{n}.{k}"]
                want = ac.adam_step(p0[n][k], m0[n][k], v0[n][k], g, t + 1, torch.float64, lr=ac.LR)
                f32 = ac.adam_step(p0[n][k], m0[n][k], v0[n][k], g, t + 1, torch.float32, lr=ac.LR)
                for what, got, w64, w32 in zip(("parameter", "exp_avg", "exp_avg_sq"), (p1[n][k], m1[n][k], v1[n][k]), want, f32):
                    check(f"{what} {n}.{k}", got, w64, w32)
        # 4. the targets: awac:215 in numpy float32 at the GPU's own values, bit for bit
        for c, tg in zip(ac.TRAINED[1:], ac.TARGETS):
            for k in p0[tg]:
                want = ac.polyak32(p0[tg][k], p1[c][k])
                if not np.array_equal(p1[tg][k].view(np.uint32), want.view(np.uint32)):
                    failures.append(f"step {t + 1} {tg}.{k}: {int((p1[tg][k] != want).sum())} entries differ from awac:215")
        # 5. the copies the next step reads: the new parameters bit for bit, zero padding
        copies = {k: v.cpu().numpy() for k, v in tr.weight_copies().items()}
        pad = lambda w, shape: np.pad(w, [(0, n_ - d) for n_, d in zip(shape, w.shape)])
        for n in p1:
            for l, layer in enumerate(ac.LAYERS):
                w = p1[n][layer + ".weight"]
                full = pad(w, (r16(w.shape[0]), r16(w.shape[1])))
                names = [(f"{n}.w{l + 1}", full)] + ([(f"{n}.w{l + 1}t", full.T)] if l > 0 and n in ac.TRAINED else [])
                for name, want in names:
                    if not np.array_equal(copies[name].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)):
                        failures.append(f"step {t + 1} copy {name}: {int((copies[name] != want).sum())} entries differ")
        for n in p1:
            assert all(np.all(np.isfinite(x)) for x in p1[n].values()), f"{case} step {t + 1}: inf or nan in {n}"
        groups = {}
        for k, r in worst.items():
            key = k.split(" ")[0] if k.split(" ")[0] in ("grad", "parameter", "exp_avg", "exp_avg_sq") else k
            groups[key] = max(groups.get(key, 0.0), r)
        top = max((k for k in worst if k.startswith("grad ")), key=lambda k: worst[k])
        _say(f"{case} step {t + 1}: error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in groups.items()) +
             f"; worst gradient {top}; {near_c + near_a} pairs near a kink ({share:.1e}); "
             f"w at the cap {int((xa['w'] >= ac.EXP_ADV_MAX).sum())} of {B}")
    assert not failures, f"{case}:\n  " + "\n  ".join(failures)


def test_update_on_an_explicit_batch_is_the_same_step():
    """``update(batch)`` (awac:301-310) = ``train_steps`` on the same rows, bit for bit, and returns the
    reference's two-key dict; the state dict has awac's three keys and its tensor names."""
    case = "s17_a6_b17_h256"
    tr_a, buf, (S, A, B, H, lam, data, idx, eps) = _trainer(case, keep_grads=False)
    tr_b, _, _ = _trainer(case, keep_grads=False)
    rows = torch.from_numpy(idx[0, :B]).to(DEV)
    e = torch.from_numpy(eps[:1]).to(DEV)
    la = tr_a.train_steps(buf, 1, B, indices=rows.view(1, B), eps=e).cpu().numpy()[0]
    batch = [torch.from_numpy(x).to(DEV) for x in ac.batch_of(data, idx[0, :B])]
    out = tr_b.update(batch, eps=e[0])
    assert list(out) == ["critic_loss", "actor_loss"]
    assert out["critic_loss"] == float(la[0]) and out["actor_loss"] == float(la[1])
    assert torch.equal(tr_a._params, tr_b._params) and torch.equal(tr_a._target, tr_b._target)
    sd = tr_b.state_dict()
    assert sorted(sd) == ["actor", "critic_1", "critic_2"]
    assert list(sd["actor"]) == ["_log_std"] + list(ac.MLP_NAMES) and list(sd["critic_1"]) == list(ac.MLP_NAMES)


def test_targets_at_a_tau_whose_rounding_matters():
    """awac:215 multiplies by float32(1 - tau) of the Python double.  At tau = 0.33 that is not float32(1 -
    float32(tau)): a step that derived 1 - tau from an fp32 tau would be one ulp off in every target entry."""
    tau = 0.33
    assert np.float32(1 - tau) != np.float32(1.0 - float(np.float32(tau)))
    case = "s17_a6_b17_h256"
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
    from iqlpref_amd import awac
    tr = _build(S, A, H, params, lam, keep_grads=False, tau=tau)
    buf = awac.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_d4rl_dataset(data)
    p0, _, _ = _read(tr)
    tr.train_steps(buf, 1, B, indices=torch.from_numpy(idx[:1, :B]).to(DEV), eps=torch.from_numpy(eps[:1]).to(DEV))
    p1, _, _ = _read(tr)
    for c, tg in zip(ac.TRAINED[1:], ac.TARGETS):
        for k in p0[tg]:
            want = ac.polyak32(p0[tg][k], p1[c][k], tau)
            assert np.array_equal(p1[tg][k].view(np.uint32), want.view(np.uint32)), f"{tg}.{k}"
    copies = tr.weight_copies()
    w = p1["target_critic_1"]["_mlp.2.weight"]
    assert np.array_equal(copies["target_critic_1.w2"].cpu().numpy().view(np.uint32), w.view(np.uint32))


# --------------------------------------------------------------------------- #
# noise drawn on the device
# --------------------------------------------------------------------------- #
def _box_muller(seed, step, B, A, stream):
    """include/iqlhip.h, iqlhip_awac_train_steps: float64 Box-Muller on Philox block (row * 8 + column / 4, step lo,
    step hi, stream), words (x, y) / (z, w) one pair each."""
    from oracle import philox
    nq = (A + 3) // 4
    rows = np.repeat(np.arange(B, dtype=np.uint32), nq)
    quads = np.tile(np.arange(nq, dtype=np.uint32), B)
    x, y, z, w = philox.philox4x32_10(rows * np.uint32(8) + quads, np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32),
                                      np.uint32(stream), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((B, nq, 4), np.float64)
    for pair, (ua, ub) in enumerate(((x, y), (z, w))):
        u1 = (ua.astype(np.float64) + 1.0) / 4294967296.0
        u2 = ub.astype(np.float64) / 4294967296.0
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        out[:, :, 2 * pair] = (rad * np.cos(ang)).reshape(B, nq)
        out[:, :, 2 * pair + 1] = (rad * np.sin(ang)).reshape(B, nq)
    return out.reshape(B, 4 * nq)[:, :A]


def test_noise_drawn_on_the_device():
    case, seed = "s29_a8_b256_h256", 0x1234567887654321
    tr, buf, (S, A, B, H, lam, data, idx, _) = _trainer(case, seed=seed, keep_grads=False)
    twin, _, _ = _trainer(case, seed=1, keep_grads=False)
    idx_t = torch.from_numpy(idx).to(DEV)
    drawn = []
    for t in range(ac.STEPS):
        got = tr.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=None)
        e = tr.last_eps()
        want = twin.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=e[None].clone())
        assert torch.equal(got, want) and torch.equal(tr._params, twin._params) and torch.equal(tr._target, twin._target)
        assert torch.equal(tr._exp_avg, twin._exp_avg) and torch.equal(tr._exp_avg_sq, twin._exp_avg_sq)
        drawn.append(e.cpu().numpy())
    drawn = np.stack(drawn)  # [STEPS, 2, B, A]
    assert np.all(np.isfinite(drawn))
    worst, differ = 0.0, 0
    for t in range(ac.STEPS):
        for which, stream in ((0, 5), (1, 6)):
            want = _box_muller(seed, t, B, A, stream)
            w32 = want.astype(np.float32)
            unit = np.spacing(np.maximum(np.abs(w32), np.float32(1e-30)))
            err = np.abs(drawn[t, which].astype(np.float64) - w32.astype(np.float64)) / unit
            worst, differ = max(worst, float(err.max())), differ + int((drawn[t, which] != w32).sum())
    n = drawn.size
    mean, var = float(drawn.mean(dtype=np.float64)), float(drawn.var(dtype=np.float64))
    _say(f"device noise: largest |device - numpy float64 Box-Muller| {worst:.2f} fp32 spacings, {differ} of {n} "
         f"entries differ; mean {mean:+.4f} (bound {5 / np.sqrt(n):.4f}), var - 1 {var - 1:+.4f} "
         f"(bound {5 * np.sqrt(2 / n):.4f})")
    assert worst <= 1.0
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert not np.array_equal(drawn[0], drawn[1]) and not np.array_equal(drawn[1], drawn[2])
    assert all(not np.array_equal(drawn[t, 0], drawn[t, 1]) for t in range(ac.STEPS))


# --------------------------------------------------------------------------- #
# groups
# --------------------------------------------------------------------------- #
def _same_trainer(got, want, where):
    torch.cuda.synchronize()
    assert got.total_it == want.total_it, where
    for name in ("_params", "_target", "_exp_avg", "_exp_avg_sq"):
        assert torch.equal(getattr(got, name), getattr(want, name)), f"{where}: {name}"
    for (k, a), b in zip(got.state_dict().items(), want.state_dict().values()):
        assert all(torch.equal(x, y) for x, y in zip(a.values(), b.values())), f"{where}: {k}"


def test_group_lifecycle_matches_members_stepped_alone():
    from iqlpref_amd import awac
    S, A, H, K = 3, 1, 16, 3
    rng = np.random.default_rng(5)

    def inputs(k):
        torch.manual_seed(40 + k)
        named = lambda m: {"_mlp." + n: v.detach().numpy().copy() for n, v in m.state_dict().items()}
        p = {"actor": named(ac.mlp(S, H, A)), "critic_1": named(ac.mlp(S + A, H, 1)), "critic_2": named(ac.mlp(S + A, H, 1))}
        p["actor"]["_log_std"] = np.full(A, -0.3 * k, np.float32)
        return p

    def dataset(n):
        return {"observations": rng.standard_normal((n, S)).astype(np.float32),
                "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32), "rewards": rng.standard_normal(n).astype(np.float32),
                "next_observations": rng.standard_normal((n, S)).astype(np.float32),
                "terminals": (rng.uniform(size=n) < 0.3).astype(np.float32)}

    params = [inputs(k) for k in range(K)]
    bufs = []
    for k in range(K):
        d = dataset(40 + 7 * k)
        bufs.append(awac.ReplayBuffer(S, A, len(d["observations"]), DEV))
        bufs[-1].load_d4rl_dataset(d)
    build = lambda: [_build(S, A, H, p, 1.0, seed=11 + k, keep_grads=False) for k, p in enumerate(params)]
    members, twins = build(), build()
    group = awac.AWACGroup(members)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    handles = []
    for B in (1, 17):
        idx = [up(rng.integers(0, 40 + 7 * k, (ac.STEPS, B))) for k in range(K)]
        # member 0 injects its normals, the others draw theirs on the device from their own keys
        eps = [up(rng.standard_normal((ac.STEPS, 2, B, A)).astype(np.float32)), None, None]
        got = group.train_steps(bufs, ac.STEPS, B, indices=idx, eps=eps, return_losses=True)
        want = [t.train_steps(b, ac.STEPS, B, indices=i, eps=e) for t, b, i, e in zip(twins, bufs, idx, eps)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == (ac.STEPS, 2) and torch.equal(g, w), f"batch {B} member {k}"
            assert bool(torch.isfinite(g).all())
        assert all(t._group_owner is group and t._handle_batch == B for t in members)
        handles.append(group._group.value)
        for k, (m, t) in enumerate(zip(members, twins)):
            _same_trainer(m, t, f"batch {B} member {k}")
            assert torch.equal(m.last_eps(), t.last_eps())
    assert all(t.total_it == 2 * ac.STEPS for t in members) and None not in handles
    assert not torch.equal(members[0]._params, members[1]._params)

    group.close()
    assert all(t._group_owner is None and t._handle is not None for t in members)
    survivor = members[1]
    del group, members
    gc.collect()
    idx = up(rng.integers(0, 47, (1, 17)))
    got = survivor.train_steps(bufs[1], 1, 17, indices=idx)
    want = twins[1].train_steps(bufs[1], 1, 17, indices=idx)
    assert torch.equal(got, want)
    _same_trainer(survivor, twins[1], "the survivor")


def test_outside_the_envelope_is_refused_before_any_launch():
    from iqlpref_amd import awac
    adam = lambda m, **kw: torch.optim.Adam(m.parameters(), lr=3e-4, **kw)

    def mk(S, A, H, **kw):
        a, c1, c2 = awac.Actor(S, A, H).to(DEV), awac.Critic(S, A, H).to(DEV), awac.Critic(S, A, H).to(DEV)
        return awac.AdvantageWeightedActorCritic(a, adam(a, **kw), c1, adam(c1), c2, adam(c2))

    for S, A, H in ((129, 6, 64), (17, 33, 64), (17, 6, 24), (17, 6, 272)):
        with pytest.raises(NotImplementedError):
            mk(S, A, H)
    with pytest.raises(NotImplementedError):
        mk(17, 6, 64, weight_decay=1e-2)
    with pytest.raises(NotImplementedError):
        mk(17, 6, 64, betas=(0.8, 0.999))
    ok = mk(17, 6, 32)
    assert ok._handle is None  # nothing was created, nothing launched
    with pytest.raises(NotImplementedError):
        awac.AWACGroup([ok] * 17)
    host = torch.zeros((1, 16), dtype=torch.int64)
    buf = awac.ReplayBuffer(17, 6, 4, DEV)
    buf.load_d4rl_dataset({"observations": np.zeros((4, 17), np.float32), "actions": np.zeros((4, 6), np.float32),
                           "rewards": np.zeros(4, np.float32), "next_observations": np.zeros((4, 17), np.float32),
                           "terminals": np.zeros(4, np.float32)})
    with pytest.raises(ValueError, match="indices"):
        ok.train_steps(buf, 1, 16, indices=host)
    with pytest.raises(ValueError, match="eps"):
        ok.train_steps(buf, 1, 16, indices=host.to(DEV), eps=torch.zeros((1, 2, 16, 6)))
    assert ok._handle is None and ok.total_it == 0
