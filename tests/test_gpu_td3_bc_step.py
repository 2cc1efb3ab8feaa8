"""The TD3+BC step (csrc/td3_bc_step.hip: k_td3_critic_fwd_bwd / k_td3_critic_update and, on an actor step,
k_td3_actor_fwd / k_td3_actor_bwd / k_td3_actor_update) over its envelope.  -m gpu.

``TD3_BC.train_steps`` with injected indices and standard normals, 2 x policy_freq steps per case (at least 3: two
actor steps each), every step judged at the GPU's own parameters of the step before (the scheme of
tests/test_gpu_awac_step.py): the critic half is restated at what the GPU held BEFORE the step, the actor half at the
GPU's old actor and its NEW critic 1 (tdbc:365 reads the critic just updated), Adam from the GPU's own p0, m0, v0 and
gradient -- the actor's on its own step count --, the targets from the GPU's old targets and new networks.

Cases (S, A, B, H, max_action, policy_freq): (3, 1, 1, 16, 1, 2), (17, 6, 17, 256, 1, 2), (128, 32, 48, 128, 2, 2),
(45, 24, 64, 64, 1, 3), (29, 8, 256, 256, 1, 1) -- tests/td3_bc_cases.py.  Every dataset row that no index names holds
1e30 in every column, and the memory right behind each step's B indices names such rows; some terminals are 1.

Compared per step: the losses, every gradient, both Adam moments and every new parameter of what the step trains.
Bound per tensor: 4 x the largest |fp32 torch - float64 torch| of that tensor on the same inputs over eight summation
orders, floored at the tensor's fp32 rounding unit at its largest entry; for the (row, hidden unit) pairs of a
differentiated network whose float64 pre-activation is within 1e-5 of zero, what the pair can contribute to each
gradient entry is added to that entry's bound, and their share stays under 1 in 1,000.  Bit for bit: the forward and
transposed copies of all six networks against the new parameters and targets; on an actor step the three targets
against the numpy-float32 evaluation of tdbc:79 at the GPU's own values; on any other step the actor, its two moments,
its optimiser's step count and all three targets against their values before the step; the eps read back against the
eps injected.  No inf or nan anywhere.  Every ratio is printed (IQLTEST lines with -s).

An MI355X gave, as the largest error / bound over the five cases and their 3 to 6 steps: critic_loss 0.25, actor_loss
0.78 (the one-row case, whose bound is the loss's own rounding unit; 0.39 in the others), gradients 0.25, new parameters
0.26, exp_avg 0.25, exp_avg_sq 0.25; every copy and every target bit for bit; at most 14 pairs of a step near a kink
(6.1e-5 of them at most), no inf or nan.  (A first version of the step formed Adam's second moment from the fp32
constants of ``AdamCoef`` as AWAC does and had critic 2's last bias -- a one-entry tensor -- at 1.16 of its bound in step
1 of the 17-row case: csrc/step_math.h, ``adam_apply_v64``.)  The device's noise equalled the numpy restatement in all
6,144 entries (0.00 spacings), mean +0.0024 (bound 0.0638), var - 1 +0.0207 (bound 0.0902).

Noise drawn on the device (the (29, 8, 256, 256) case): a step with ``eps=None``, its eps read back, equals bit for
bit a twin stepped with those eps injected; the eps equal the numpy Box-Muller restatement on ``oracle.philox`` at
stream 7 within one fp32 spacing (tests/test_gpu_awac_step.py has why that is the bound) and differ between steps.

Group: three members with their own parameters, data and alpha stepped as one ``TD3BCGroup`` -- one with its
``total_it`` one ahead, so that members take their actor steps on different steps, one at policy_freq 3 -- at batch 1,
then at batch 17, where every member handle is rebuilt and the group with them, match twins stepped alone bit for bit.
Then the group is closed, two members are deleted and the survivor steps on like its twin.
"""
import gc

import numpy as np
import pytest
import torch

from tests import td3_bc_cases as tc

pytestmark = pytest.mark.gpu
DEV = tc.DEV
STREAM = 7


def _say(line):
    print("IQLTEST td3bc-step " + line)


def _trainer(case, **kw):
    from iqlpref_amd import td3_bc
    S, A, B, H, params, data, idx, eps, _ = tc.case_inputs(case)
    tr = tc.build_trainer(S, A, H, params, tc.hyper(case), **kw)
    buf = td3_bc.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_d4rl_dataset(data)
    return tr, buf, (S, A, B, H, data, idx, eps)


def _read(tr):
    torch.cuda.synchronize()
    p, m, v, step = {}, {}, {}, {}
    opts = dict(zip(tc.TRAINED, tr._optimizers))
    for n, mod in tr._modules().items():
        p[n] = {k: x.detach().cpu().numpy().copy() for k, x in mod.named_parameters()}
        if n not in opts:
            continue
        m[n], v[n], step[n] = {}, {}, set()
        for k, par in mod.named_parameters():
            st = opts[n].state.get(par) or {}
            m[n][k], v[n][k] = (st[x].detach().cpu().numpy().copy() if x in st else np.zeros(tuple(par.shape), np.float32)
                                for x in ("exp_avg", "exp_avg_sq"))
            step[n].add(float(st["step"]) if "step" in st else 0.0)
    return p, m, v, step


def _grads(tr):
    return {f"{n}.{k}": par.grad.detach().cpu().numpy().copy() for n in tc.TRAINED
            for k, par in getattr(tr, n).named_parameters()}


def _kink_extra(half, args, zs, g64):
    near = tc.near_kink(zs)
    n_near = sum(int(x.sum()) for x in near)
    extra = {k: 0.0 for k in g64}
    if n_near:
        on = half(*args, torch.float64, force=(near, 1.0))[1]
        off = half(*args, torch.float64, force=(near, 0.0))[1]
        extra = {k: np.abs(on[k] - off[k]) for k in g64}
    return n_near, sum(x.size for x in near), extra


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("case", list(tc.CASES))
def test_step_at_the_gpus_own_parameters(case):
    tr, buf, (S, A, B, H, data, idx, eps) = _trainer(case)
    hp = tc.hyper(case)
    idx_t, eps_t = torch.from_numpy(idx).to(DEV), torch.from_numpy(eps).to(DEV)
    failures, r16 = [], lambda x: -(-x // 16) * 16
    actor_it = 0
    for t in range(tc.n_steps(case)):
        p0, m0, v0, _ = _read(tr)
        # (a view of the index row: the poisoned indices lie right behind the B real ones in memory)
        losses = tr.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=eps_t[t:t + 1])
        p1, m1, v1, step1 = _read(tr)
        losses = losses.cpu().numpy()[0]
        grads = _grads(tr)
        acts = tc.is_actor_step(t + 1, hp["policy_freq"])
        actor_it += int(acts)
        assert tr.total_it == t + 1
        assert step1["critic_1"] == step1["critic_2"] == {float(t + 1)} and step1["actor"] == {float(actor_it)}
        assert _same_bits(tr.last_eps().cpu().numpy(), eps[t])
        batch = tc.batch_of(data, idx[t, :B])
        worst = {}

        def check(what, got, w64, w32=None, extra=0.0, gap=None):
            _, bound = tc.judge(got, w64, w32) if gap is None else tc.judge_gap(got, w64, gap)
            err = np.abs(np.asarray(got, np.float64) - np.asarray(w64, np.float64))
            ratio = float(np.max(err / (bound + extra))) if np.all(np.isfinite(err)) else np.inf
            worst[what] = ratio
            if not ratio <= 1:
                failures.append(f"step {t + 1} {what}: {ratio:.2f} of the bound {bound:.2e}")

        # 1. the critic half at the GPU's old parameters
        cnets = (p0["actor_target"], p0["critic_1"], p0["critic_2"], p0["critic_1_target"], p0["critic_2_target"])
        cargs = cnets + (batch, eps[t], hp)
        lc64, gc64, zc, _ = tc.critic_half(*cargs, torch.float64)
        lc_gap, gc_gap = tc.fp32_gap(tc.critic_half, cnets, (batch, eps[t], hp), {"critic_1": 1, "critic_2": 2}, lc64, gc64)
        near, pairs, extra = _kink_extra(tc.critic_half, cargs, zc, gc64)
        assert np.all(np.isfinite(losses))
        check("critic_loss", losses[0], lc64, gap=lc_gap)
        g64, ggap = dict(gc64), dict(gc_gap)
        trained = ["critic_1", "critic_2"]
        if acts:
            # 2. the actor half at the GPU's old actor and NEW critic 1
            anets = (p0["actor"], p1["critic_1"])
            aargs = anets + (batch, hp)
            la64, ga64, za, xa = tc.actor_half(*aargs, torch.float64)
            la_gap, ga_gap = tc.fp32_gap(tc.actor_half, anets, (batch, hp), {"actor": 0}, la64, ga64)
            near_a, pairs_a, extra_a = _kink_extra(tc.actor_half, aargs, za, ga64)
            near, pairs = near + near_a, pairs + pairs_a
            assert xa["mean_abs_q"] >= 1e-3
            check("actor_loss", losses[1], la64, gap=la_gap)
            g64.update(ga64), ggap.update(ga_gap), extra.update(extra_a)
            trained.append("actor")
        else:
            assert losses[1] == 0.0
        share = near / pairs
        assert share <= tc.KINK_CAP, f"{case} step {t + 1}: {share} of the pairs within {tc.KINK} of a kink"
        for k in g64:
            check("grad " + k, grads[k], g64[k], extra=extra[k], gap=ggap[k])
        # 3. the updates, from the GPU's own numbers (the actor's Adam on its own count)
        for n in trained:
            for k in p0[n]:
                g, t1 = grads[f"{n}.{k}"], actor_it if n == "actor" else t + 1
                want = tc.adam_step(p0[n][k], m0[n][k], v0[n][k], g, t1, torch.float64, lr=tc.LR)
                f32 = tc.adam_step(p0[n][k], m0[n][k], v0[n][k], g, t1, torch.float32, lr=tc.LR)
                for what, got, w64, w32 in zip(("parameter", "exp_avg", "exp_avg_sq"), (p1[n][k], m1[n][k], v1[n][k]), want, f32):
                    check(f"{what} {n}.{k}", got, w64, w32)
        # 4. the targets: tdbc:79 in numpy float32 at the GPU's own values on an actor step; untouched otherwise,
        #    as are the actor and its moments
        for n, tg in zip(tc.TRAINED, tc.TARGETS):
            for k in p0[tg]:
                want = tc.polyak32(p0[tg][k], p1[n][k], hp["tau"]) if acts else p0[tg][k]
                if not _same_bits(p1[tg][k], want):
                    failures.append(f"step {t + 1} {tg}.{k}: {int((p1[tg][k] != want).sum())} entries differ from "
                                    + ("tdbc:79" if acts else "the step before"))
        if not acts:
            for k in p0["actor"]:
                for what, a, b in (("parameter", p1, p0), ("exp_avg", m1, m0), ("exp_avg_sq", v1, v0)):
                    if not _same_bits(a["actor"][k], b["actor"][k]):
                        failures.append(f"step {t + 1} actor {what} {k} changed on a step without an actor update")
        # 5. the copies the next step reads: the new parameters bit for bit, zero padding
        copies = {k: v.cpu().numpy() for k, v in tr.weight_copies().items()}
        pad = lambda w, shape: np.pad(w, [(0, n_ - d) for n_, d in zip(shape, w.shape)])
        seen = set()
        for n in p1:
            for l, layer in enumerate(tc.LAYERS):
                w = p1[n][layer + ".weight"]
                full = pad(w, (r16(w.shape[0]), r16(w.shape[1])))
                for name, want in ((f"{n}.w{l + 1}", full), (f"{n}.w{l + 1}t", full.T)):
                    if name not in copies:
                        continue
                    seen.add(name)
                    if not _same_bits(copies[name], want):
                        failures.append(f"step {t + 1} copy {name}: {int((copies[name] != want).sum())} entries differ")
        assert seen == set(copies) and len(copies) == 18 + 7
        for n in p1:
            assert all(np.all(np.isfinite(x)) for x in p1[n].values()), f"{case} step {t + 1}: inf or nan in {n}"
        groups = {}
        for k, r in worst.items():
            key = k.split(" ")[0] if k.split(" ")[0] in ("grad", "parameter", "exp_avg", "exp_avg_sq") else k
            groups[key] = max(groups.get(key, 0.0), r)
        top = max((k for k in worst if k.startswith("grad ")), key=lambda k: worst[k])
        _say(f"{case} step {t + 1} ({'actor' if acts else 'critics only'}): error / bound: "
             + ", ".join(f"{k} {v:.3f}" for k, v in groups.items())
             + f"; worst gradient {top}; {near} pairs near a kink ({share:.1e})")
    assert not failures, f"{case}:\n  " + "\n  ".join(failures)


def test_train_on_an_explicit_batch_is_the_same_step():
    """``train(batch)`` (tdbc:324-380) = ``train_steps`` on the same rows, bit for bit; ``actor_loss`` is in the dict
    on actor steps only; the state dict has tdbc's seven keys and round-trips with rebuilt targets."""
    case = "s17_a6_b17_h256"
    tr_a, buf, (S, A, B, H, data, idx, eps) = _trainer(case, keep_grads=False)
    tr_b, _, _ = _trainer(case, keep_grads=False)
    for t in range(2):
        rows = torch.from_numpy(idx[t, :B]).to(DEV)
        e = torch.from_numpy(eps[t:t + 1]).to(DEV)
        la = tr_a.train_steps(buf, 1, B, indices=rows.view(1, B), eps=e).cpu().numpy()[0]
        out = tr_b.train([torch.from_numpy(x).to(DEV) for x in tc.batch_of(data, idx[t, :B])], eps=e[0])
        assert list(out) == (["critic_loss"] if t == 0 else ["critic_loss", "actor_loss"])
        assert out["critic_loss"] == float(la[0]) and out.get("actor_loss", 0.0) == float(la[1])
        assert torch.equal(tr_a._params, tr_b._params) and torch.equal(tr_a._target, tr_b._target)
    sd = tr_b.state_dict()
    assert list(sd) == ["critic_1", "critic_1_optimizer", "critic_2", "critic_2_optimizer", "actor", "actor_optimizer", "total_it"]
    assert list(sd["actor"]) == list(tc.NAMES) and sd["total_it"] == 2
    assert {float(s["step"]) for s in sd["actor_optimizer"]["state"].values()} == {1.0}
    assert {float(s["step"]) for s in sd["critic_1_optimizer"]["state"].values()} == {2.0}
    # a fresh trainer that loads it steps on like the one that wrote it, except that its targets are the networks
    tr_c, _, _ = _trainer(case, keep_grads=False)
    tr_c.load_state_dict(sd)
    assert tr_c.total_it == 2 and tr_c._actor_it == 1
    assert torch.equal(tr_c._params, tr_b._params) and torch.equal(tr_c._target, tr_c._params)
    assert torch.equal(tr_c._exp_avg, tr_b._exp_avg) and torch.equal(tr_c._exp_avg_sq, tr_b._exp_avg_sq)
    with torch.no_grad():
        tr_b._target.copy_(tr_b._params)
    tr_b.sync_weights()
    rows, e = torch.from_numpy(idx[2:4, :B]).to(DEV).contiguous(), torch.from_numpy(eps[2:4]).to(DEV)
    assert torch.equal(tr_c.train_steps(buf, 2, B, indices=rows, eps=e), tr_b.train_steps(buf, 2, B, indices=rows, eps=e))
    assert torch.equal(tr_c._params, tr_b._params) and torch.equal(tr_c._target, tr_b._target)
    assert torch.equal(tr_c._exp_avg_sq, tr_b._exp_avg_sq)


def test_targets_at_a_tau_whose_rounding_matters():
    """tdbc:79 multiplies by float32(1 - tau) of the Python double; at tau = 0.33 that is not float32(1 - float32(tau))."""
    tau = 0.33
    assert np.float32(1 - tau) != np.float32(1.0 - float(np.float32(tau)))
    case = "s17_a6_b17_h256"
    tr, buf, (S, A, B, H, data, idx, eps) = _trainer(case, keep_grads=False, tau=tau)
    tr.train_steps(buf, 1, B, indices=torch.from_numpy(idx[:1, :B]).to(DEV), eps=torch.from_numpy(eps[:1]).to(DEV))
    p0 = _read(tr)[0]
    tr.train_steps(buf, 1, B, indices=torch.from_numpy(idx[1:2, :B]).to(DEV), eps=torch.from_numpy(eps[1:2]).to(DEV))
    p1 = _read(tr)[0]
    for n, tg in zip(tc.TRAINED, tc.TARGETS):
        for k in p0[tg]:
            assert _same_bits(p1[tg][k], tc.polyak32(p0[tg][k], p1[n][k], tau)), f"{tg}.{k}"


# --------------------------------------------------------------------------- #
# noise drawn on the device
# --------------------------------------------------------------------------- #
def test_noise_drawn_on_the_device():
    case, seed = tc.NOISE_CASE, 0x1234567887654321
    tr, buf, (S, A, B, H, data, idx, _) = _trainer(case, seed=seed, keep_grads=False)
    twin, _, _ = _trainer(case, seed=1, keep_grads=False)
    idx_t = torch.from_numpy(idx).to(DEV)
    drawn = []
    steps = tc.n_steps(case)
    for t in range(steps):
        got = tr.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=None)
        e = tr.last_eps()
        want = twin.train_steps(buf, 1, B, indices=idx_t[t, :B].view(1, B), eps=e[None].clone())
        assert torch.equal(got, want) and torch.equal(tr._params, twin._params) and torch.equal(tr._target, twin._target)
        assert torch.equal(tr._exp_avg, twin._exp_avg) and torch.equal(tr._exp_avg_sq, twin._exp_avg_sq)
        drawn.append(e.cpu().numpy())
    drawn = np.stack(drawn)  # [steps, B, A]
    assert np.all(np.isfinite(drawn))
    worst, differ = 0.0, 0
    for t in range(steps):
        w32 = tc.box_muller(seed, t, B, A, STREAM).astype(np.float32)
        unit = np.spacing(np.maximum(np.abs(w32), np.float32(1e-30)))
        err = np.abs(drawn[t].astype(np.float64) - w32.astype(np.float64)) / unit
        worst, differ = max(worst, float(err.max())), differ + int((drawn[t] != w32).sum())
    n = drawn.size
    mean, var = float(drawn.mean(dtype=np.float64)), float(drawn.var(dtype=np.float64))
    _say(f"device noise: largest |device - numpy float64 Box-Muller| {worst:.2f} fp32 spacings, {differ} of {n} "
         f"entries differ; mean {mean:+.4f} (bound {5 / np.sqrt(n):.4f}), var - 1 {var - 1:+.4f} "
         f"(bound {5 * np.sqrt(2 / n):.4f})")
    assert worst <= 1.0
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert all(not np.array_equal(drawn[t], drawn[t + 1]) for t in range(steps - 1))


# --------------------------------------------------------------------------- #
# groups
# --------------------------------------------------------------------------- #
def _same_trainer(got, want, where):
    torch.cuda.synchronize()
    assert got.total_it == want.total_it and got._actor_it == want._actor_it, where
    for name in ("_params", "_target", "_exp_avg", "_exp_avg_sq"):
        assert torch.equal(getattr(got, name), getattr(want, name)), f"{where}: {name}"
    a, b = got.state_dict(), want.state_dict()
    for n in tc.TRAINED:
        assert all(torch.equal(x, y) for x, y in zip(a[n].values(), b[n].values())), f"{where}: {n}"
        sa, sb = a[n + "_optimizer"]["state"], b[n + "_optimizer"]["state"]
        assert [float(s["step"]) for s in sa.values()] == [float(s["step"]) for s in sb.values()], f"{where}: {n} steps"


def test_group_lifecycle_matches_members_stepped_alone():
    from iqlpref_amd import td3_bc
    S, A, H, K, STEPS = 3, 1, 16, 3, 6
    rng = np.random.default_rng(5)
    # own alpha, max_action and policy_freq each; member 1 starts one step ahead: actor steps on different steps
    over = [dict(alpha=2.5), dict(alpha=1.0, max_action=2.0, policy_noise=0.4, noise_clip=1.0), dict(alpha=4.0, policy_freq=3)]

    def inputs(k):
        torch.manual_seed(40 + k)
        named = lambda m: {"net." + n: v.detach().numpy().copy() for n, v in m.state_dict().items()}
        return {"actor": named(tc.mlp(S, H, A)), "critic_1": named(tc.mlp(S + A, H, 1)), "critic_2": named(tc.mlp(S + A, H, 1))}

    def dataset(n):
        return {"observations": rng.standard_normal((n, S)).astype(np.float32),
                "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32), "rewards": rng.standard_normal(n).astype(np.float32),
                "next_observations": rng.standard_normal((n, S)).astype(np.float32),
                "terminals": (rng.uniform(size=n) < 0.3).astype(np.float32)}

    params = [inputs(k) for k in range(K)]
    bufs = []
    for k in range(K):
        d = dataset(40 + 7 * k)
        bufs.append(td3_bc.ReplayBuffer(S, A, len(d["observations"]), DEV))
        bufs[-1].load_d4rl_dataset(d)
    hp = dict(tc.hyper("s3_a1_b1_h16"))

    def build():
        out = [tc.build_trainer(S, A, H, p, hp, seed=11 + k, keep_grads=False, **over[k]) for k, p in enumerate(params)]
        out[1].total_it = 1  # (as a checkpoint's total_it would set it; the handle is created with it)
        return out

    members, twins = build(), build()
    group = td3_bc.TD3BCGroup(members)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    handles = []
    for B in (1, 17):
        idx = [up(rng.integers(0, 40 + 7 * k, (STEPS, B))) for k in range(K)]
        # member 0 injects its normals, the others draw theirs on the device from their own keys
        eps = [up(rng.standard_normal((STEPS, B, A)).astype(np.float32)), None, None]
        got = group.train_steps(bufs, STEPS, B, indices=idx, eps=eps, return_losses=True)
        want = [t.train_steps(b, STEPS, B, indices=i, eps=e) for t, b, i, e in zip(twins, bufs, idx, eps)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == (STEPS, 2) and torch.equal(g, w), f"batch {B} member {k}"
            assert bool(torch.isfinite(g).all())
        # the actor_loss column is 0.0 exactly where the member's own count says so
        for k, g in enumerate(got):
            first = members[k].total_it - STEPS
            acts = [(first + i + 1) % members[k].policy_freq == 0 for i in range(STEPS)]
            assert [bool(x) for x in (g[:, 1] != 0).cpu()] == acts, f"batch {B} member {k}"
        assert all(t._group_owner is group and t._handle_batch == B for t in members)
        handles.append(group._group.value)
        for k, (m, t) in enumerate(zip(members, twins)):
            _same_trainer(m, t, f"batch {B} member {k}")
            assert torch.equal(m.last_eps(), t.last_eps())
    assert [t.total_it for t in members] == [2 * STEPS, 2 * STEPS + 1, 2 * STEPS] and None not in handles
    assert [t._actor_it for t in members] == [6, 6, 4]
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
