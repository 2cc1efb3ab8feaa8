"""Seed groups of the BB flavour on the GPU: short last batches in group launches.  -m gpu.

1. every member of a group stepped with per-member valid-row counts is byte-identical to the same trainer
   stepped alone with ``train_steps(n_valid=...)`` (tests/test_gpu_bb.py pins that lone path to the float64
   restatement and to the reference run), over every fp32 geometry a group launch of k_backward can take;
2. counts that all equal the batch change no bit; poisoned padding rows change nothing; graph replay equals
   plain launches and the cached graph is keyed on counts;
3. the K-way block index generator equals the host sampler for every member;
4. ``train(seeds_per_gpu=3)``: every seed byte-identical to ``train()`` of that seed alone;
5. groups on the general step and bf16 groups refuse counts before anything is launched.

The geometry of a group launch of k_backward (csrc/iql_step.hip: bwd_parts_per_wg, launch_backward), with
R = batch x members rows per launch and P = layer2_parts(H) = 4 / 2 / 1 for H = 256 / 128 / 64:
    PW = 2 (never PRE)   iff R >= 512 and P even and H >= 128
    PRE (PW = 1)         iff not PW = 2 and R < 1024
    PW = 1 without PRE   iff not PW = 2 and R >= 1024
"""
import os

import numpy as np
import pytest
import torch

from tests import bb_env
from tests import test_gpu_bb as one  # the lone-trainer helpers: the same nets, buffers and tensors

pytestmark = pytest.mark.gpu
DEV = one.DEV
S, A, N = one.S, one.A, one.N
B = bb_env.BATCH
LOSSES = one.LOSSES
NVS = (1, 7, 15, 16, 17, 31, B)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bb_train_run.npz")))


@pytest.fixture(scope="module")
def bb():
    from iqlpref_amd import custom_offline_bb
    return custom_offline_bb


@pytest.fixture(scope="module")
def dataset(golden, bb):
    return bb.BBDataset({k[5:]: v for k, v in golden.items() if k.startswith("data/")})


def _transitions(seed, poison_from=None):
    """Standard-normal transitions (as test_gpu_bb.py's short_case); rows from ``poison_from`` on hold 1e4."""
    rng = np.random.default_rng(seed)
    d = {"observations": rng.standard_normal((N, S)).astype(np.float32),
         "actions": np.stack([rng.uniform(0, 0.8, N), rng.uniform(-1, 1, N)], 1).astype(np.float32),
         "rewards": rng.standard_normal(N).astype(np.float32),
         "next_observations": rng.standard_normal((N, S)).astype(np.float32),
         "terminals": (rng.uniform(size=N) < 0.1).astype(np.float32)}
    if poison_from is not None:
        for v in d.values():
            v[poison_from:] = 1.0e4
    return d


def _buffer(bb, transitions):
    buf = bb.ReplayBuffer(S, A, N, DEV)
    buf.load_dataset(transitions)
    return buf


def _state(tr, losses):
    """Everything a step writes: losses, parameters (log_std among them), Adam moments, target nets."""
    out = one._tensors(tr)
    out["losses"] = losses.cpu().numpy().copy()
    out["log_std"] = tr.actor.log_std.detach().cpu().numpy().copy()
    return out


def _same(got, want, what):
    for k in want:
        assert np.isfinite(want[k]).all(), (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _counts(nv, batch):
    return None if nv is None else torch.tensor([batch, nv, batch], dtype=torch.int32, device=DEV)


def _plan(K, batch, seed):
    """Per member: indices of three steps (valid entries from rows [0, PAD0), the padding entries of the short
    step from [PAD0, N)), its count for the middle step (None for one member: no counts at all) and its seed."""
    rng = np.random.default_rng(seed)
    nvs = [NVS[(k + 1) % len(NVS)] for k in range(K)]  # 7, 15, 16, 17, 31, B, 1, 7, ...
    nvs = [batch if nv == B else nv for nv in nvs]  # (B stands for the whole batch, whatever its size)
    nvs[K // 2] = None
    plan = []
    for k in range(K):
        idx = rng.integers(0, one.PAD0, (3, batch))
        if nvs[k] is not None:
            idx[1, nvs[k]:] = rng.integers(one.PAD0, N, batch - nvs[k])
        plan.append((torch.from_numpy(idx).to(DEV), nvs[k], 100 + 7 * k))
    return plan


def _lone(bb, dataset, buf, plan, hidden, batch):
    out = []
    for idx, nv, seed in plan:
        tr = one._trainer(bb, dataset, seed=seed, t_max=1000, hidden=hidden)
        out.append(_state(tr, tr.train_steps(buf, 3, batch, indices=idx, n_valid=_counts(nv, batch), graph_unroll=0)))
    return out


def _group(bb, dataset, buf, plan, hidden, batch, mode, graph_unroll=0):
    import iqlpref_amd as ia
    trs = [one._trainer(bb, dataset, seed=seed, t_max=1000, hidden=hidden) for _, _, seed in plan]
    group = ia.SeedGroup(trs, mode=mode)
    losses = group.train_steps(buf, 3, batch, indices=[p[0] for p in plan], n_valid=[_counts(p[1], batch) for p in plan],
                               return_losses=True, graph_unroll=graph_unroll)
    group.synchronize()
    counts = group.launch_counts() if mode == "group" else None
    out = [_state(tr, l) for tr, l in zip(trs, losses)]
    group.close()
    return out, counts


# (H, batch, K, mode): the geometry each case hits is in its id
CASES = [
    pytest.param(256, 32, 2, "group", id="H256-B32-K2-PRE-PW1"),
    pytest.param(256, 32, 2, "split", id="H256-B32-K2-split"),
    pytest.param(256, 32, 2, "streams", id="H256-B32-K2-streams"),
    pytest.param(128, 32, 3, "group", id="H128-B32-K3-oddK"),
    pytest.param(256, 32, 16, "group", id="H256-B32-K16-PW2"),
    pytest.param(64, 64, 16, "group", id="H64-B64-K16-PW1-noPRE"),
]


@pytest.mark.parametrize("hidden,batch,K,mode", CASES)
def test_members_equal_lone_trainers(bb, dataset, hidden, batch, K, mode):
    buf = _buffer(bb, _transitions(5))
    plan = _plan(K, batch, seed=hidden + K)
    nvs = [p[1] for p in plan]
    assert nvs.count(None) == 1 and len({nv for nv in nvs if nv is not None}) >= min(K - 1, 2)
    assert all(nv is None or 1 <= nv <= batch for nv in nvs)
    want = _lone(bb, dataset, buf, plan, hidden, batch)
    got, counts = _group(bb, dataset, buf, plan, hidden, batch, mode)
    if mode == "group":
        assert counts == (3, 0)
    for k in range(K):
        _same(got[k], want[k], f"member {k} (n_valid {nvs[k]})")
    # a short step is not a whole one: the counts reached the kernels
    short = next(k for k, nv in enumerate(nvs) if nv is not None and nv < batch)
    whole = _lone(bb, dataset, buf, [(plan[short][0], None, plan[short][2])], hidden, batch)[0]
    assert got[short]["losses"][1].tobytes() != whole["losses"][1].tobytes()
    assert got[short]["losses"][0].tobytes() == whole["losses"][0].tobytes()


def test_every_count_value_in_one_group(bb, dataset):
    """All of 1, 7, 15, 16, 17, 31, B side by side (K = 7, H = 256)."""
    buf = _buffer(bb, _transitions(5))
    rng = np.random.default_rng(3)
    plan = []
    for k, nv in enumerate(NVS):
        idx = rng.integers(0, one.PAD0, (3, B))
        idx[1, nv:] = rng.integers(one.PAD0, N, B - nv)
        plan.append((torch.from_numpy(idx).to(DEV), nv, 40 + k))
    want = _lone(bb, dataset, buf, plan, 256, B)
    got, _ = _group(bb, dataset, buf, plan, 256, B, "group")
    for k, nv in enumerate(NVS):
        _same(got[k], want[k], f"n_valid {nv}")


def test_whole_batch_counts_change_no_bit(bb, dataset):
    import iqlpref_amd as ia
    buf = _buffer(bb, _transitions(5))
    rng = np.random.default_rng(8)
    idx = [torch.from_numpy(rng.integers(0, N, (3, B))).to(DEV) for _ in range(3)]
    runs = []
    for valid in (torch.full((3,), B, dtype=torch.int32, device=DEV), None):  # ONE tensor shared by all members
        trs = [one._trainer(bb, dataset, seed=60 + k, t_max=1000) for k in range(3)]
        group = ia.SeedGroup(trs, mode="group")
        kw = {} if valid is None else {"n_valid": valid}
        losses = group.train_steps(buf, 3, B, indices=idx, return_losses=True, graph_unroll=0, **kw)
        group.synchronize()
        runs.append([_state(tr, l) for tr, l in zip(trs, losses)])
        group.close()
    for k in range(3):
        _same(runs[0][k], runs[1][k], f"member {k}")


def test_padding_rows_leak_nowhere(bb, dataset):
    """K = 3: the rows the padding entries point at hold 1e4 everywhere in one run; not one bit differs."""
    plan = _plan(3, B, seed=1)
    plan = [(idx, nv if nv is not None else 17, seed) for idx, nv, seed in plan]  # every member has a short step
    assert all(nv < B for _, nv, _ in plan)
    clean, _ = _group(bb, dataset, _buffer(bb, _transitions(5)), plan, 256, B, "group")
    dirty, _ = _group(bb, dataset, _buffer(bb, _transitions(5, poison_from=one.PAD0)), plan, 256, B, "group")
    for k in range(3):
        _same(dirty[k], clean[k], f"member {k}")


def test_graph_replay_and_the_graph_cache_is_keyed_on_counts(bb, dataset):
    """graph_unroll = 3 with counts, then a second call on the SAME group without counts, then counts again; and
    on a fresh group the other way round, where a graph cached for the plain call would ignore the counts of the
    next.  Every call equals plain launches, and launch_counts() shows the replays."""
    import iqlpref_amd as ia
    buf = _buffer(bb, _transitions(5))
    plan = _plan(3, B, seed=2)
    counted = ([p[0] for p in plan], [_counts(p[1], B) for p in plan])
    rng = np.random.default_rng(12)
    plain = ([torch.from_numpy(rng.integers(0, N, (3, B))).to(DEV) for _ in plan], None)
    for order in ((counted, plain, counted), (plain, counted)):
        runs = {}
        for unroll in (0, 3):
            trs = [one._trainer(bb, dataset, seed=p[2], t_max=1000) for p in plan]
            group = ia.SeedGroup(trs, mode="group")
            calls = []
            for i, v in order:
                losses = group.train_steps(buf, 3, B, indices=i, n_valid=v, return_losses=True, graph_unroll=unroll)
                group.synchronize()
                calls.append([_state(tr, l) for tr, l in zip(trs, losses)])
            assert group.launch_counts() == ((0, len(order)) if unroll else (3 * len(order), 0))
            runs[unroll] = calls
            group.close()
        for c in range(len(order)):
            for k in range(3):
                _same(runs[3][c][k], runs[0][c][k], f"call {c} member {k}")
        if order[0] is counted:  # the first call against lone trainers
            want = _lone(bb, dataset, buf, plan, 256, B)
            for k in range(3):
                _same(runs[3][0][k], want[k], f"member {k} against the lone trainer")


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("n_rows,t0", [(167, 0), (167, 5), (167, 11), (160, 3), (7, 2)])
def test_group_index_generator_equals_host_sampler(bb, n_rows, t0, K):
    gen = torch.Generator().manual_seed(n_rows + K)
    samplers = [bb.BlockEpochSampler(n_rows, B, generator=gen) for _ in range(K)]
    if K > 1 and n_rows >= 2 * B:
        assert len({tuple(s.perm.tolist()) for s in samplers}) > 1  # distinct permutations
    idx, valid = bb.BlockEpochSamplerGroup(samplers).device_indices(t0, 14, DEV)
    assert len(idx) == K and valid.dtype == torch.int32 and tuple(valid.shape) == (14,)
    for k, s in enumerate(samplers):
        want_idx, want_valid = s.host_indices(t0, 14)
        assert idx[k].dtype == torch.int64 and idx[k].is_contiguous()
        np.testing.assert_array_equal(idx[k].cpu().numpy(), want_idx)
        np.testing.assert_array_equal(valid.cpu().numpy(), want_valid)
        lone_idx, lone_valid = s.device_indices(t0, 14, DEV)
        assert torch.equal(lone_idx, idx[k]) and torch.equal(lone_valid, valid)


def test_a_sampler_group_of_one_is_its_sampler(bb):
    """37 rows in batches of 8 (4 blocks and 5 rows left over), steps 3 .. 11: the short slot twice, the epoch
    wrap, and the one-sampler launch behind the group's return shape."""
    sampler = bb.BlockEpochSampler(37, 8, generator=torch.Generator().manual_seed(37))
    idx, valid = bb.BlockEpochSamplerGroup([sampler]).device_indices(3, 9, DEV)
    lone_idx, lone_valid = sampler.device_indices(3, 9, DEV)
    want_idx, want_valid = sampler.host_indices(3, 9)
    assert isinstance(idx, list) and len(idx) == 1 and want_valid.tolist() == [8, 5, 8, 8, 8, 8, 5, 8, 8]
    assert torch.equal(idx[0], lone_idx) and torch.equal(valid, lone_valid)
    assert idx[0].dtype == torch.int64 and valid.dtype == torch.int32
    np.testing.assert_array_equal(idx[0].cpu().numpy(), want_idx)
    np.testing.assert_array_equal(valid.cpu().numpy(), want_valid)


def _train(bb, golden, tmp_path, **kw):
    records = []
    seeds = []
    real_eval = bb.bb_run_eval_IQL

    def spy(**ekw):
        seeds.append(ekw["seed"])
        return real_eval(**dict(ekw, max_horizon=20))

    config = bb.TrainConfig(update_steps=12, eval_every=6, batch_size=B, normalize_state=True, normalize_reward=True,
                            eval_episodes=1, eval_seed=4, checkpoints_path=str(tmp_path), train_seed=kw.pop("train_seed"))
    bb.bb_run_eval_IQL = spy
    try:
        out = bb.train(config, {k[5:]: v for k, v in golden.items() if k.startswith("data/")}, bb_env.numpy_reward,
                       bb_env.MOVE_STATS, logger=lambda d, step: records.append((int(step), dict(d))), device=DEV,
                       chunk=4, **kw)
    finally:
        bb.bb_run_eval_IQL = real_eval
    return out, records, seeds, config


def _flat(x, prefix=""):
    if isinstance(x, dict):
        for k, v in x.items():
            yield from _flat(v, f"{prefix}/{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _flat(v, f"{prefix}/{i}")
    else:
        yield prefix, (x.detach().cpu().numpy().tobytes() if isinstance(x, torch.Tensor) else x)


def test_train_three_seeds_per_gpu(golden, bb, tmp_path):
    s0 = int(golden["train_seed"])
    perms = [golden["perm"], np.array([4, 2, 0, 3, 1]), np.array([1, 3, 4, 0, 2])]
    trainers, records, eval_seeds, config = _train(bb, golden, tmp_path / "group", train_seed=s0, seeds_per_gpu=3,
                                                   perm=perms)
    assert isinstance(trainers, list) and len(trainers) == 3
    assert all(set(r) - {"seed"} and "seed" in r for _, r in records)
    assert eval_seeds == [4 + 5] * 3 + [4 + 11] * 3  # eval_seed + step, per member
    for k, tr in enumerate(trainers):
        seed = s0 + k
        mine = [(step, {n: v for n, v in r.items() if n != "seed"}) for step, r in records if r["seed"] == seed]
        lone, lone_records, _, _ = _train(bb, golden, tmp_path / f"lone{k}", train_seed=seed, perm=perms[k])
        assert [(s, list(r)) for s, r in mine] == [(s, list(r)) for s, r in lone_records]
        for (_, a), (_, b) in zip(mine, lone_records):  # losses, evaluation returns, best score and step
            for n in a:
                assert np.float64(a[n]).tobytes() == np.float64(b[n]).tobytes(), (seed, n)
        got, want = dict(_flat(tr.state_dict())), dict(_flat(lone.state_dict()))
        assert got.keys() == want.keys()
        for n in want:
            assert got[n] == want[n], (seed, n)
        assert tr.total_it == 12 and tr.actor.training
        files = sorted(os.listdir(os.path.join(config.checkpoints_path, f"seed_{seed}")))
        assert files == ["best_model.pt", "checkpoint_11.pt", "checkpoint_5.pt"]
        if k == 0:
            losses = np.asarray([[r[n] for n in LOSSES] for _, r in mine if "value_loss" in r])
            print(f"member 0 loss rel error vs the reference {np.abs(losses / golden['losses'] - 1).max():.2e}")
            np.testing.assert_allclose(losses, golden["losses"], rtol=one.TOL)
    assert sorted(os.listdir(config.checkpoints_path)) == ["config.yaml"] + [f"seed_{s0 + k}" for k in range(3)]


# --------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------- #
def _refused(group, trs, buf, match):
    idx = [torch.zeros((2, B), dtype=torch.int64, device=DEV) for _ in trs]
    before = [one._tensors(t) for t in trs]
    counts = group.launch_counts()
    with pytest.raises(NotImplementedError, match=match):
        group.train_steps(buf, 2, B, indices=idx, n_valid=torch.tensor([B, 7], dtype=torch.int32, device=DEV))
    assert group.launch_counts() == counts and all(t.total_it == 0 and t.launch_counts() == (0, 0) for t in trs)
    for b, t in zip(before, trs):
        a = one._tensors(t)
        for k in b:
            assert a[k].tobytes() == b[k].tobytes(), k
    group.train_steps(buf, 2, B, indices=idx)  # the same call without counts runs
    group.synchronize()
    assert all(t.total_it == 2 for t in trs) and sum(group.launch_counts()) > counts[0] + counts[1]
    group.close()


def test_general_group_refuses_counts_before_any_launch(bb, dataset):
    import iqlpref_amd as ia
    trs = [one._trainer(bb, dataset, seed=2 + k, t_max=100, hidden=96) for k in range(2)]
    group = ia.SeedGroup(trs, mode="general")
    _refused(group, trs, _buffer(bb, dataset.transitions()), "valid-row counts")


def test_bf16_group_refuses_counts_before_any_launch(bb, dataset):
    import iqlpref_amd as ia
    trs = []
    for k in range(2):
        torch.manual_seed(2 + k)
        q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), ia.GaussianPolicy(S, A, 1.0).to(DEV)
        trs.append(ia.ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), q,
                                        torch.optim.Adam(q.parameters(), lr=3e-4), v,
                                        torch.optim.Adam(v.parameters(), lr=3e-4), device=DEV, precision="bf16",
                                        seed=2 + k))
    group = ia.SeedGroup(trs, mode="group")
    _refused(group, trs, _buffer(bb, dataset.transitions()), "fp32")


def test_the_library_refuses_what_the_python_check_refuses(bb, dataset):
    """iqlhip_group_train_steps_valid itself: IQLHIP_ERR_UNSUPPORTED for a general-step group, nothing launched."""
    import ctypes as C
    import iqlpref_amd as ia
    from iqlpref_amd import _lib
    trs = [one._trainer(bb, dataset, seed=2 + k, t_max=100, hidden=96) for k in range(2)]
    group = ia.SeedGroup(trs, mode="general")
    buf = _buffer(bb, dataset.transitions())
    group._ensure_group(B)
    idx = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    valid = torch.tensor([B, 7], dtype=torch.int32, device=DEV)
    views = (_lib.ReplayView * 2)(buf.view(), buf.view())
    arr = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)
    rc = _lib.load().iqlhip_group_train_steps_valid(group._group, views, 2, arr(idx), arr(valid), None, None, 0,
                                                    _lib.stream_ptr())
    assert rc == _lib.ERR_UNSUPPORTED and b"valid-row counts" in _lib.load().iqlhip_last_error()
    assert group.launch_counts() == (0, 0)
    group.close()


def test_count_dtype_and_shape_are_checked(bb, dataset):
    import iqlpref_amd as ia
    buf = _buffer(bb, dataset.transitions())
    idx = [torch.zeros((2, B), dtype=torch.int64, device=DEV) for _ in range(2)]
    for mode in ("group", "split", "streams"):
        trs = [one._trainer(bb, dataset, seed=2 + k, t_max=100) for k in range(2)]
        group = ia.SeedGroup(trs, mode=mode)
        good = torch.tensor([B, 7], dtype=torch.int32, device=DEV)
        for bad in (good.to(torch.int64), torch.tensor([B, 7, B], dtype=torch.int32, device=DEV), good.cpu(),
                    [good], [good, good, good], [good, good.to(torch.int64)]):
            with pytest.raises(ValueError):
                group.train_steps(buf, 2, B, indices=idx, n_valid=bad)
        assert all(t.total_it == 0 for t in trs)
        group.close()
