"""iqlhip_mlp_set_forward (one launch for M MLPs with weights of their own) against M separate
iqlhip_mlp_forward calls, bit for bit; the set as a snapshot; posthoc.evaluate_many and posthoc.run with real
policies against the sequential loop that calls policy_actions per step.  -m gpu.

The sampled table covers every M of {1, 2, 5, 33}, every R of {1, 15, 16, 17, 64, 65, 130} (one row, one M
tile short of a row, one M tile, one more row, one 64-row tile, one more row, three tiles), inputs 1 / 3 /
45 / 128, hidden widths 1 / 17 / 64 / 255 / 256, outputs 1 / 2 / 24 / 32 (the k-split narrow last layer)
and 64 / 256 (the main path), 1 / 2 / 3 / 8 layers, relu and tanh hidden layers, none and tanh outputs, two
codes of the flax table (k_mlp_set<2>) and both weight layouts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import fake_envs, helpers
from tests.fake_envs import FakeGymEnv, FakeGymnasiumEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = helpers.ACT_FLAX_BASE
TOL = 2e-5  # tests/test_gpu_mlp_envelope.py: rtol = atol for fp32 forwards of up to four layers
SENTINEL = -77.25
PAD_X, PAD_OUT, TAIL_ROWS = 3, 5, 2

# (dims, hidden_act, out_act, w_in_out, M, R)
CASES = [
    ([45, 256, 256, 24], 0, 1, 0, 1, 1), ([45, 256, 256, 24], 0, 1, 0, 2, 16), ([45, 256, 256, 24], 0, 1, 0, 5, 17),
    ([45, 256, 256, 24], 0, 1, 1, 33, 1), ([45, 256, 256, 24], 0, 1, 0, 5, 130), ([45, 256, 256, 24], 1, 1, 0, 2, 65),
    ([45, 255, 255, 24], 0, 1, 0, 5, 15), ([45, 255, 24], 1, 0, 1, 2, 64), ([3, 17, 2], 0, 0, 0, 33, 17),
    ([3, 17, 17, 1], 1, 1, 1, 5, 65), ([1, 1, 1], 0, 0, 0, 2, 1), ([1, 1], 0, 0, 0, 5, 15), ([1, 64, 1], 0, 1, 1, 1, 130),
    ([128, 64, 32], 0, 0, 0, 2, 17), ([128, 256, 32], 1, 0, 0, 5, 16), ([128, 32], 0, 1, 1, 33, 15),
    ([128, 24], 0, 0, 0, 1, 64), ([3, 2], 0, 1, 0, 2, 130), ([45, 1], 0, 0, 1, 33, 16),
    ([45, 64, 64, 64, 64, 64, 64, 64, 24], 0, 1, 0, 2, 17), ([3, 17, 17, 17, 17, 17, 17, 17, 2], 1, 0, 1, 5, 1),
    ([128, 255, 255, 255, 255, 255, 255, 255, 32], 0, 0, 0, 1, 65), ([45, 256, 256, 256], 0, 1, 0, 2, 15),
    ([45, 64, 64], 0, 0, 1, 5, 64), ([3, 256, 64], 1, 1, 0, 2, 130), ([128, 256], 0, 0, 0, 5, 17),
    ([45, 64, 24], T + 6, 0, 0, 2, 1), ([45, 64, 24], T + 6, T + 0, 1, 5, 16), ([3, 17, 1], T + 3, 1, 0, 33, 15),
    ([45, 255, 255, 32], T + 0, T + 7, 0, 2, 65), ([128, 64, 256], T + 6, 0, 0, 1, 130), ([8, 16, 64], T + 6, T + 0, 1, 5, 17),
    ([45, 256, 24], 0, T + 1, 0, 2, 64), ([1, 17, 2], 0, 1, 0, 1, 15), ([3, 1, 24], 0, 0, 0, 1, 16),
    ([45, 17, 32], 1, 1, 0, 33, 64), ([128, 1, 1], 0, 0, 1, 2, 65), ([1, 256, 256, 2], 0, 1, 0, 33, 130),
    ([3, 64, 255, 1], 0, 0, 0, 1, 17), ([45, 256, 256, 24], 0, 1, 0, 33, 16),
]


def test_the_table_covers_what_it_says():
    dims = [c[0] for c in CASES]
    assert {c[4] for c in CASES} == {1, 2, 5, 33} and {c[5] for c in CASES} == {1, 15, 16, 17, 64, 65, 130}
    assert {d[0] for d in dims} >= {1, 3, 45, 128} and {d[-1] for d in dims} >= {1, 2, 24, 32, 64, 256}
    assert {w for d in dims for w in d[1:-1]} >= {1, 17, 64, 255, 256}
    assert {len(d) - 1 for d in dims} == {1, 2, 3, 8} and {c[3] for c in CASES} == {0, 1}
    assert {c[1] for c in CASES} >= {0, 1, T + 6, T + 3} and {c[2] for c in CASES} >= {0, 1, T + 0, T + 7}
    assert 35 <= len(CASES) <= 45


def _id(c):
    return "x".join(map(str, c[0])) + f"-a{c[1]}.{c[2]}-io{c[3]}-M{c[4]}-R{c[5]}"


@pytest.fixture(scope="module")
def lib():
    from iqlpref_amd import _lib
    return _lib.load()


def _members(dims, hidden, out, io, M, seed):
    """M distinct members: numpy weights [in, out], their device tensors in the layout asked for, descriptors."""
    from iqlpref_amd.iql import mlp_desc
    rng = np.random.default_rng(seed)
    host, descs, keep = [], [], []
    for _ in range(M):
        ws, bs = helpers.mlp_weights_for(rng, dims)
        tw = [torch.from_numpy(np.ascontiguousarray(w if io else w.T)).to(DEV) for w in ws]
        tb = [torch.from_numpy(b).to(DEV) for b in bs]
        d, k = mlp_desc(tw, tb, w_in_out=bool(io), hidden_act=hidden, out_act=out)
        host.append((ws, bs)), descs.append(d), keep.append((tw, tb, k))
    return host, descs, keep


def _create(lib, descs):
    from iqlpref_amd import _lib
    arr = (C.POINTER(_lib.MlpDesc) * len(descs))(*[C.pointer(d) for d in descs])
    handle = C.c_void_p()
    _lib.check(lib.iqlhip_mlp_set_create(arr, len(descs), C.byref(handle), _lib.stream_ptr()))
    return handle


def _solo(lib, d, x, n, x_stride, n_out):
    from iqlpref_amd import _lib
    out = torch.full((n, n_out), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(lib.iqlhip_mlp_forward(C.byref(d), C.c_void_p(x.data_ptr()), n, x_stride, _lib.ptr(out), n_out,
                                      _lib.stream_ptr()))
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_set_forward_carries_the_bits_of_separate_forwards(lib, case):
    from iqlpref_amd import _lib
    dims, hidden, out_act, io, M, R = case
    n_in, n_out = dims[0], dims[-1]
    host, descs, keep = _members(dims, hidden, out_act, io, M, seed=sum(dims) + 7 * M + R)
    xs, os_ = n_in + PAD_X, n_out + PAD_OUT
    rng = np.random.default_rng(R + 31 * M)
    x_np = rng.standard_normal((M, R, xs)).astype(np.float32)
    x = torch.from_numpy(x_np).to(DEV)
    out = torch.full((M * R + TAIL_ROWS, os_), SENTINEL, dtype=torch.float32, device=DEV)
    handle = _create(lib, descs)
    try:
        _lib.check(lib.iqlhip_mlp_set_forward(handle, _lib.ptr(x), R, xs, _lib.ptr(out), os_, _lib.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        assert lib.iqlhip_mlp_set_destroy(handle) == 0
    # exactly M R rows and n_out columns are written
    assert torch.all(out[M * R:] == SENTINEL) and torch.all(out[:M * R, n_out:] == SENTINEL)
    got = out[:M * R, :n_out].reshape(M, R, n_out)
    assert torch.isfinite(got).all()
    rows = sorted({r for r in (0, 14, 15, 16, 63, 64, R - 1) if r < R})
    for m in range(M):
        # the R rows of member m in one call
        assert torch.equal(got[m], _solo(lib, descs[m], x[m], R, xs, n_out)), f"member {m}, R-row call"
        # ... and one row at a time, as the sequential program forwards them
        for r in rows:
            assert torch.equal(got[m, r:r + 1], _solo(lib, descs[m], x[m, r], 1, xs, n_out)), f"member {m}, row {r}"
    if M > 1:  # the members' weights are distinct, and so are their outputs
        assert not torch.equal(got[0], _solo(lib, descs[1], x[0], R, xs, n_out))
    if len(dims) - 1 <= 4:  # one independent check: the fp64 forward, at the envelope test's tolerance
        for m in (0, M - 1):
            want = helpers.mlp_forward_ref(*host[m], x_np[m, :, :n_in], hidden, out_act)
            err = np.abs(got[m].cpu().numpy() - want).max()
            print(f"{_id(case)} member {m}: max |err| = {err:.3e}")
            np.testing.assert_allclose(got[m].cpu().numpy(), want, rtol=TOL, atol=TOL)


def test_the_set_is_a_snapshot(lib):
    from iqlpref_amd import _lib
    dims, M, R = [45, 64, 24], 3, 5
    host, descs, keep = _members(dims, 0, 1, 0, M, seed=5)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((M, R, 45)).astype(np.float32)).to(DEV)

    def forward(handle):
        out = torch.empty((M, R, 24), dtype=torch.float32, device=DEV)
        _lib.check(lib.iqlhip_mlp_set_forward(handle, _lib.ptr(x), R, 45, _lib.ptr(out), 24, _lib.stream_ptr()))
        return out
    handle = _create(lib, descs)
    before = forward(handle)
    for tw, tb, k in keep:  # overwrite the sources (the descriptors point at these very tensors)
        for t in k:
            t.mul_(-0.5).add_(0.25)
    torch.cuda.synchronize()
    assert torch.equal(forward(handle), before)
    assert lib.iqlhip_mlp_set_destroy(handle) == 0
    handle = _create(lib, descs)  # a new set sees the new weights
    after = forward(handle)
    assert lib.iqlhip_mlp_set_destroy(handle) == 0
    assert not torch.equal(after, before)
    for m in range(M):
        assert torch.equal(after[m], _solo(lib, descs[m], x[m], R, 45, 24))


def test_r_zero_and_short_strides_write_nothing(lib):
    from iqlpref_amd import _lib
    host, descs, keep = _members([8, 16, 4], 0, 0, 0, 2, seed=9)
    x = torch.zeros((2, 4, 8), dtype=torch.float32, device=DEV)
    out = torch.full((2, 4, 4), SENTINEL, dtype=torch.float32, device=DEV)
    handle = _create(lib, descs)
    try:
        for R, xs, os_ in ((0, 8, 4), (-1, 8, 4), (4, 7, 4), (4, 8, 3)):
            rc = lib.iqlhip_mlp_set_forward(handle, _lib.ptr(x), R, xs, _lib.ptr(out), os_, _lib.stream_ptr())
            assert rc == _lib.ERR_INVALID, (R, xs, os_)
        assert lib.iqlhip_mlp_set_forward(handle, None, 4, 8, _lib.ptr(out), 4, None) == _lib.ERR_INVALID
        assert lib.iqlhip_mlp_set_forward(handle, _lib.ptr(x), 4, 8, None, 4, None) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert torch.all(out == SENTINEL)
    finally:
        assert lib.iqlhip_mlp_set_destroy(handle) == 0


# --------------------------------------------------------------------------- #
# the Python layer
# --------------------------------------------------------------------------- #
NAME, S, A = "posthoc-11-3", 11, 3
EPISODES, SEED = 6, 123


@pytest.fixture(autouse=True)
def _dims(monkeypatch):
    monkeypatch.setitem(fake_envs.DIMS, NAME, (S, A))


class SpacedGymnasiumEnv(FakeGymnasiumEnv):
    """With the spaces posthoc.run reads the dimensions and the action bound from."""

    def __init__(self, name):
        super().__init__(name)
        self.observation_space, self.action_space = fake_envs._Box(self.S, np.inf), fake_envs._Box(self.A, 1.0)


def _policies(kind, width, n=3, dropout=0.1):
    import iqlpref_amd as ia
    cls = ia.GaussianPolicy if kind == "gaussian" else ia.DeterministicPolicy
    out = []
    for i in range(n):
        torch.manual_seed(1000 + i + width)
        out.append(cls(S, A, 1.0, hidden_dim=width, n_hidden=2, dropout=dropout).to(DEV))
    return out


def _sequential(actor, mode, mean, std):
    """The two reference loops with policy_actions as ``actor.act``."""
    import iqlpref_amd as ia
    actor.eval()

    def act(state):
        return ia.policy_actions(actor, np.asarray(state).reshape(1, -1), 1.0, DEV).flatten()
    out = []
    if mode == "reset":
        env = ia.wrap_env(FakeGymnasiumEnv(NAME), state_mean=mean, state_std=std)
        for i in range(EPISODES):
            (state, _), done, total = env.reset(seed=SEED + i), False, 0.0
            while not done:
                state, reward, terminated, truncated, _ = env.step(act(state))
                done = terminated or truncated
                total += reward
            out.append(total)
    else:
        env = ia.wrap_env(FakeGymEnv(NAME), state_mean=mean, state_std=std)
        env.seed(SEED)
        for _ in range(EPISODES):
            state, done, total = env.reset(), False, 0.0
            while not done:
                state, reward, done, _ = env.step(act(state))
                total += reward
            out.append(total)
    return np.asarray(out)


@pytest.mark.parametrize("kind,width", (("gaussian", 64), ("deterministic", 64), ("gaussian", 300)))
def test_evaluate_many_equals_the_sequential_program(kind, width):
    from iqlpref_amd import posthoc
    actors = _policies(kind, width)
    mean, std = np.linspace(-0.3, 0.3, S), np.linspace(0.7, 1.3, S)
    want = {mode: np.stack([_sequential(a, mode, mean, std) for a in actors]) for mode in ("reset", "chain")}
    assert len({tuple(r) for r in want["reset"]}) == len(actors)  # distinct weights, distinct returns
    actors[0].train(), actors[1].eval(), actors[2].train()
    for mode, env in (("reset", FakeGymnasiumEnv), ("chain", FakeGymEnv)):
        got = posthoc.evaluate_many(functools.partial(env, NAME), actors, EPISODES, SEED, episode_seeding=mode,
                                    lanes=4, state_mean=mean, state_std=std, device=DEV)
        np.testing.assert_array_equal(got.view(np.uint64), want[mode].view(np.uint64), err_msg=mode)
        assert [a.training for a in actors] == [True, False, True]
    # the reference's signature: one actor on an environment the caller wrapped
    import iqlpref_amd as ia
    env = ia.wrap_env(FakeGymnasiumEnv(NAME), state_mean=mean, state_std=std)
    one = posthoc.evaluate(env, actors[1], EPISODES, SEED, DEV)
    np.testing.assert_array_equal(one.view(np.uint64), want["reset"][1].view(np.uint64))


def test_policy_actions_many_and_a_mixed_group():
    import iqlpref_amd as ia
    from iqlpref_amd import posthoc
    actors = _policies("gaussian", 64)
    obs = np.random.default_rng(3).standard_normal((3, 5, S))
    actor_set = posthoc.MlpSet([a.net for a in actors], DEV)
    got = posthoc.policy_actions_many(actor_set, obs, 1.0)
    for m, a in enumerate(actors):
        a.eval()
        np.testing.assert_array_equal(got[m].view(np.uint32), ia.policy_actions(a, obs[m], 1.0, DEV).view(np.uint32))
    actor_set.close()
    with pytest.raises(RuntimeError, match="closed"):
        actor_set.forward(torch.zeros((3, 1, S), device=DEV))
    with pytest.raises(NotImplementedError, match="300 > 256"):
        posthoc.MlpSet([a.net for a in _policies("gaussian", 300, n=1)], DEV)
    with pytest.raises(ValueError, match="differs"):
        posthoc.MlpSet([actors[0].net, _policies("gaussian", 32, n=1)[0].net], DEV)
    # actors of two shapes in one call: two sets behind one result
    mixed = [actors[0], _policies("gaussian", 32, n=1)[0], actors[2]]
    got = posthoc.evaluate_many(functools.partial(FakeGymnasiumEnv, NAME), mixed, 3, SEED, lanes=2, device=DEV)
    for m, a in enumerate(mixed):
        solo = posthoc.evaluate_many(functools.partial(FakeGymnasiumEnv, NAME), [a], 3, SEED, lanes=1, device=DEV)
        np.testing.assert_array_equal(got[m], solo[0])


def test_run_writes_the_rows_of_single_evaluations(tmp_path):
    import iqlpref_amd as ia
    from iqlpref_amd import posthoc
    actors = _policies("gaussian", 64, n=4)
    run_dir = tmp_path / "pen" / "cloned-v2-ab12cd34"
    os.makedirs(run_dir)
    paths = []
    for t, a in zip((4999, 9999, 14999, 19999), actors):
        paths.append(str(run_dir / f"checkpoint_{t}.pt"))
        torch.save({"actor": a.state_dict(), "total_it": t + 1}, paths[-1])
    spec = {"project": "IQL-eval", "program": "evaluation/minari/iql_eval.py", "method": "grid",
            "parameters": {"eval_csv": {"value": str(tmp_path / "grid.csv")}, "dataset_id": {"value": NAME},
                           "eval_episodes": {"value": EPISODES}, "eval_seed": {"value": SEED},
                           "actor_path": {"values": paths}}}
    observations = np.random.default_rng(8).standard_normal((200, S)).astype(np.float32)
    make = functools.partial(SpacedGymnasiumEnv, NAME)
    configs = posthoc.expand_eval_sweep(spec)
    logs = []
    scores = posthoc.run(configs, make_env=make, dataset={"observations": observations}, lanes=3, device=DEV,
                         log=logs.append)
    assert len(scores) == 4 and len(logs) == 1 and "4 checkpoints" in logs[0]
    mean, std = ia.compute_mean_std(observations, eps=1e-3)
    for p, a in zip(paths, actors):
        loaded = posthoc.load_actor(p, S, A, 1.0, False, DEV)
        assert not loaded.training and loaded.net._dims == [S, 64, 64, A] and loaded.net._dropout is not None
        env = ia.wrap_env(FakeGymnasiumEnv(NAME), state_mean=mean, state_std=std)
        single = posthoc.evaluate(env, loaded, EPISODES, SEED, DEV)
        posthoc.write_mean_row(str(tmp_path / "single.csv"), NAME, p, single)
    grid, single = open(tmp_path / "grid.csv").read(), open(tmp_path / "single.csv").read()
    assert grid == single and len(grid.splitlines()) == 5
    assert [line.split(",")[1:3] for line in grid.splitlines()[1:]] == [["ab12cd34", str(t)]
                                                                        for t in (4999, 9999, 14999, 19999)]
    with pytest.raises(ValueError, match="11 -> 3"):
        posthoc.load_actor(paths[0], S + 1, A, 1.0, False, DEV)
    # the d4rl program loads with strict=False: a Gaussian checkpoint as a deterministic policy (log_std ignored)
    with pytest.raises(RuntimeError, match="log_std"):
        posthoc.load_actor(paths[0], S, A, 1.0, True, DEV)
    lenient = posthoc.load_actor(paths[0], S, A, 1.0, True, DEV, strict=False)
    assert isinstance(lenient, ia.DeterministicPolicy)
    assert torch.equal(lenient.net.linears()[0].weight, actors[0].net.linears()[0].weight)
    # a file that holds more than tensors and plain containers is not unpickled
    torch.save({"actor": actors[0].state_dict(), "extra": SpacedGymnasiumEnv}, str(run_dir / "checkpoint_0.pt"))
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|global"):
        posthoc.load_actor(str(run_dir / "checkpoint_0.pt"), S, A, 1.0, False, DEV)
