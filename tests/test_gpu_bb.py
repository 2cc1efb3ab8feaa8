"""The BB flavour (iqlpref_amd/custom_offline_bb.py) on the GPU.  -m gpu.

1. short batches (iqlhip_train_steps_valid) against a float64 torch restatement of the step on the valid
   rows only (tests/bb_env.py), n_valid in {1, 7, 15, 16, 17, 31, 32}, one short step between two whole
   ones; n_valid == 32 equals the call without counts bit for bit; poisoned padding rows change nothing;
   graph replay equals plain launches;
2. the block index generator equals the host sampler;
3. train_epoch_steps over the 12 steps of tests/golden/bb_train_run.npz (a run of the reference's own
   iql_bb.py) in one call and split at step 5: the reference's losses and parameters, and bit-identical
   to each other;
4. act() on the recorded evaluation states;
5. train() end to end;
6. the general layer-wise step and bf16 trainers refuse counts before anything is launched.

Tolerances, as tests/test_gpu_step.py applies the project's fp32 bound of 2e-5 to reference arrays:
* losses: rtol 2e-5 (its TOL["fp32"]).  Measured: <= 2.3e-6 against the restatement, 1.6e-6 against the
  reference's 12 steps.
* parameters and target: rtol = atol = 2e-5, the project's form for fp32 arrays (test_gpu_mlp_envelope.py,
  test_gpu_train.py).  An entry-wise bound relative to a tensor's LARGEST entry does not fit a parameter
  after Adam steps: for an entry whose gradient is near adam_eps the update lr g / (|g| + eps) moves by
  lr / eps = 3e4 times the gradient's fp32 rounding error, whatever the kernel does -- measured 1.8e-6 on
  an entry of q2's 256 x 256 layer after three WHOLE batches on the unchanged path (2.9e-5 of the largest
  entry 0.063), 3.0e-6 with a one-row step between them.  atol 2e-5 is 7 % of one lr = 3e-4 step.
* Adam moments: largest error <= 1e-4 of the tensor's largest entry, test_gpu_step.py's MOMENT_TOL for
  fp32 (an absolute 2e-5 would be empty for exp_avg_sq entries of 1e-6).  Adam's step does not depend on
  the gradient's scale, so it is the moments and the losses that would show a wrong divisor (32 for 7 is a
  factor 4.6).  Measured against the reference's 12 steps: 2.9e-5 in the worst tensor.
"""
import os

import numpy as np
import pytest
import torch

from tests import bb_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
LOSSES = ("value_loss", "q_loss", "actor_loss")
S, A, B, N = bb_env.STATE_DIM, bb_env.ACTION_DIM, bb_env.BATCH, bb_env.N_ROWS
PAD0 = 128  # rows [PAD0, 160) are referenced by padding entries only: the poison variant overwrites them


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


def _trainer(bb, dataset, seed, t_max, hidden=256):
    import iqlpref_amd as ia
    torch.manual_seed(seed)
    q, v = ia.TwinQ(S, A, hidden).to(DEV), ia.ValueFunction(S, hidden).to(DEV)
    actor = bb.GaussianPolicy(S, A, dataset.max_actions().to(DEV), dataset.min_actions().to(DEV), hidden).to(DEV)
    ao = torch.optim.Adam(actor.parameters(), lr=3e-4)
    return bb.ImplicitQLearning(
        dataset.max_actions(), dataset.min_actions(), actor, ao, torch.optim.lr_scheduler.CosineAnnealingLR(ao, t_max),
        q, torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4), device=DEV,
        seed=seed)


def _buffer(bb, transitions):
    buf = bb.ReplayBuffer(S, A, N, DEV)
    buf.load_dataset(transitions)
    return buf


def _tensors(tr):
    """Everything a step writes, as host arrays: parameters, target, Adam moments."""
    torch.cuda.synchronize()
    return {"params": tr._params.cpu().numpy().copy(), "target": tr._target.cpu().numpy().copy(),
            "exp_avg": tr._exp_avg.cpu().numpy().copy(), "exp_avg_sq": tr._exp_avg_sq.cpu().numpy().copy()}


def _net_params(tr):
    out = {}
    for name, mlp in (("q1", tr.qf.q1), ("q2", tr.qf.q2), ("v", tr.vf.v), ("actor", tr.actor.net)):
        out[name] = [t.detach().cpu().numpy().copy() for l in mlp.linears() for t in (l.weight, l.bias)]
    return out


MOMENT_TOL = 1e-4  # of a moment tensor's largest entry (test_gpu_step.py, fp32)


def _close(got, want, what, moment=False):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{what}: max error {err:.3e} of largest entry {scale:.3e} = {err / (scale + 1e-300):.2e}")
    if moment:
        assert err <= MOMENT_TOL * scale, what
    else:
        np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL, err_msg=what)


# --------------------------------------------------------------------------- #
# 1. short batches
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def short_case(bb, dataset):
    """Indices of three steps -- valid entries from rows [0, PAD0), padding entries of the short step from
    [PAD0, 160) -- and the clean and the poisoned transitions.

    The inputs are standard-normal in every state column (as test_gpu_custom_train.py's buffers), not the
    fixture's dataset: that one keeps its last four columns raw (day runs to 180), the untrained nets then
    put out |q|, |v| of 5-20, and a value loss of 0.05 is a mean of squared differences of such numbers --
    an fp32 forward (relative error ~1e-6 per output) is then 20-50 times that off in the advantage and
    twice that in the loss, beyond 2e-5 against ANY float64 restatement whatever the kernel does (measured:
    step 0, a whole batch on the unchanged path, 1e-7; the step after a one-row step 3.3e-5 on a value loss
    of 0.050).  With O(1) outputs the bound measures the kernel."""
    rng = np.random.default_rng(5)
    clean = {"observations": rng.standard_normal((N, S)).astype(np.float32),
             "actions": np.stack([rng.uniform(0, 0.8, N), rng.uniform(-1, 1, N)], 1).astype(np.float32),
             "rewards": rng.standard_normal(N).astype(np.float32),
             "next_observations": rng.standard_normal((N, S)).astype(np.float32),
             "terminals": (rng.uniform(size=N) < 0.1).astype(np.float32)}
    poisoned = {k: v.copy() for k, v in clean.items()}
    for k, v in poisoned.items():
        v[PAD0:160] = 1.0e4  # large and finite: a leak would move the results, not merely add NaN
    idx = rng.integers(0, PAD0, (3, B))
    pad = PAD0 + rng.permutation(32)
    return dict(clean=clean, poisoned=poisoned, idx=idx, pad=pad)


def _run_short(bb, dataset, case, nv, *, poisoned=False, counts=True, graph_unroll=0):
    tr = _trainer(bb, dataset, seed=11, t_max=1000)
    init = _net_params(tr), tr.actor.log_std.detach().cpu().numpy().copy()
    buf = _buffer(bb, case["poisoned" if poisoned else "clean"])
    idx = case["idx"].copy()
    idx[1, nv:] = case["pad"][nv:]
    valid = torch.tensor([B, nv, B], dtype=torch.int32, device=DEV) if counts else None
    losses = tr.train_steps(buf, 3, B, indices=torch.from_numpy(idx).to(DEV), n_valid=valid,
                            graph_unroll=graph_unroll).cpu().numpy()
    assert tr.launch_counts() == ((0, 1) if graph_unroll else (3, 0))
    return tr, init, idx, losses


@pytest.mark.parametrize("nv", [1, 7, 15, 16, 17, 31, 32])
def test_short_batch_against_restatement(bb, dataset, short_case, nv):
    tr, (params, log_std), idx, losses = _run_short(bb, dataset, short_case, nv)
    assert tr.step_kind(B) == "tuned"
    ref = bb_env.StepRestatement(params, log_std, t_max=1000)
    d = short_case["clean"]
    want = []
    for t, n in enumerate((B, nv, B)):
        rows = idx[t, :n]
        want.append(ref.train(d["observations"][rows], d["actions"][rows], d["rewards"][rows],
                              d["next_observations"][rows], 1.0 - d["terminals"][rows]))
    print(f"n_valid {nv}: loss rel error {np.abs(losses / np.asarray(want) - 1).max():.2e}")
    np.testing.assert_allclose(losses, want, rtol=TOL)
    got = _net_params(tr)
    m_got = {n: ([], []) for n in bb_env.NETS}
    for name, mlp in (("q1", tr.qf.q1), ("q2", tr.qf.q2), ("v", tr.vf.v), ("actor", tr.actor.net)):
        opt = {"q1": tr.q_optimizer, "q2": tr.q_optimizer, "v": tr.v_optimizer, "actor": tr.actor_optimizer}[name]
        leaves = [t for l in mlp.linears() for t in (l.weight, l.bias)] + ([tr.actor.log_std] if name == "actor" else [])
        for p in leaves:
            m_got[name][0].append(opt.state[p]["exp_avg"].cpu().numpy())
            m_got[name][1].append(opt.state[p]["exp_avg_sq"].cpu().numpy())
    for name in bb_env.NETS:
        for i, (g, w) in enumerate(zip(got[name], ref.p[name])):
            _close(g, w.detach().numpy(), f"n_valid {nv} {name} tensor {i}")
        m_want, v_want = ref.moments(name)
        for i, (g, w) in enumerate(zip(m_got[name][0], m_want)):
            _close(g, w, f"n_valid {nv} {name} exp_avg {i}", moment=True)
        for i, (g, w) in enumerate(zip(m_got[name][1], v_want)):
            _close(g, w, f"n_valid {nv} {name} exp_avg_sq {i}", moment=True)
    _close(tr.actor.log_std.detach().cpu().numpy(), ref.log_std.detach().numpy(), f"n_valid {nv} log_std")
    for name, mlp in (("q1", tr.q_target.q1), ("q2", tr.q_target.q2)):
        tg = [t.detach().cpu().numpy() for l in mlp.linears() for t in (l.weight, l.bias)]
        for i, (g, w) in enumerate(zip(tg, ref.target[name])):
            _close(g, w.numpy(), f"n_valid {nv} target {name} tensor {i}")


def test_whole_batch_counts_change_no_bit(bb, dataset, short_case):
    with_counts = _run_short(bb, dataset, short_case, 32)
    without = _run_short(bb, dataset, short_case, 32, counts=False)
    assert with_counts[3].tobytes() == without[3].tobytes()
    a, b = _tensors(with_counts[0]), _tensors(without[0])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("nv", [1, 7, 17, 31])
def test_padding_rows_leak_nowhere(bb, dataset, short_case, nv):
    """The rows the padding entries point at hold 1e4 everywhere in one run: not one bit differs."""
    clean = _run_short(bb, dataset, short_case, nv)
    dirty = _run_short(bb, dataset, short_case, nv, poisoned=True)
    assert np.isfinite(clean[3]).all() and clean[3].tobytes() == dirty[3].tobytes()
    a, b = _tensors(clean[0]), _tensors(dirty[0])
    for k in a:
        assert np.isfinite(a[k]).all() and a[k].tobytes() == b[k].tobytes(), k


def test_short_batch_under_graph_replay(bb, dataset, short_case):
    plain = _run_short(bb, dataset, short_case, 7)
    graph = _run_short(bb, dataset, short_case, 7, graph_unroll=3)
    assert plain[3].tobytes() == graph[3].tobytes()
    a, b = _tensors(plain[0]), _tensors(graph[0])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------------------- #
# 2. block index generator
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n_rows,t0", [(167, 0), (167, 5), (167, 6), (167, 11), (160, 0), (160, 3), (7, 2)])
def test_block_indices_equal_host_sampler(bb, n_rows, t0):
    s = bb.BlockEpochSampler(n_rows, B, generator=torch.Generator().manual_seed(n_rows))
    idx, valid = s.device_indices(t0, 14, DEV)
    want_idx, want_valid = s.host_indices(t0, 14)
    assert idx.dtype == torch.int64 and valid.dtype == torch.int32
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(valid.cpu().numpy(), want_valid)
    assert 0 <= int(idx.min()) and int(idx.max()) < n_rows


# --------------------------------------------------------------------------- #
# 3. run parity with the reference
# --------------------------------------------------------------------------- #
def _golden_tensors(golden, prefix):
    return {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}


def _check_against_golden(sd_nets, want, what):
    for net, sd in sd_nets.items():
        for k, v in sd.items():
            v = v.detach().cpu().numpy()
            assert abs(v.astype(np.float64).sum() - want[f"{net}/{k}/sum"]) <= TOL * np.abs(v).max() * v.size, (what, net, k)
            if f"{net}/{k}/full" in want:
                _close(v, want[f"{net}/{k}/full"], f"{what} {net}/{k}")
            else:
                _close(v[0], want[f"{net}/{k}/row0"], f"{what} {net}/{k} row 0")


def _nets(tr):
    return {"qf": tr.qf.state_dict(), "vf": tr.vf.state_dict(), "actor": tr.actor.state_dict(),
            "q_target": tr.q_target.state_dict()}


def test_epoch_steps_replay_the_reference(golden, bb, dataset):
    sampler = bb.BlockEpochSampler(N, B, perm=golden["perm"])
    runs = []
    for split in ((12,), (5, 7)):
        tr = _trainer(bb, dataset, seed=int(golden["train_seed"]), t_max=12)
        if len(split) == 1:  # the nets the reference built under the same torch seed, bit for bit
            for net, sd in _nets(tr).items():
                for k, v in sd.items():
                    assert float(v.cpu().double().sum()) == golden[f"init/{net}/{k}/sum"], (net, k)
        buf = _buffer(bb, dataset.transitions())
        losses, t = [], 0
        for n in split:
            losses.append(tr.train_epoch_steps(buf, sampler, t, n))
            t += n
        runs.append((torch.cat(losses).cpu().numpy(), _tensors(tr), tr))
    (l1, t1, tr), (l2, t2, _) = runs
    assert l1.tobytes() == l2.tobytes()
    for k in t1:
        assert t1[k].tobytes() == t2[k].tobytes(), k
    print(f"loss rel error vs the reference {np.abs(l1 / golden['losses'] - 1).max():.2e}")
    np.testing.assert_allclose(l1, golden["losses"], rtol=TOL)
    _check_against_golden(_nets(tr), _golden_tensors(golden, "step11/"), "step 11")
    sd = tr.state_dict()
    assert set(sd) == {"qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer", "actor_lr_scheduler"}
    for opt in ("q_optimizer", "v_optimizer", "actor_optimizer"):
        for i, st in sd[opt]["state"].items():
            assert float(st["step"]) == golden[f"final/{opt}/{i}/step"] == 12.0
            for k in ("exp_avg", "exp_avg_sq"):
                v = st[k].cpu().numpy()
                pre = f"final/{opt}/{i}/{k}"
                _close(v if f"{pre}/full" in golden else v[0], golden.get(f"{pre}/full", golden.get(f"{pre}/row0")),
                       f"{opt} {i} {k}", moment=True)
    assert sd["actor_lr_scheduler"]["last_epoch"] == 12


def test_epoch_steps_parameters_step_by_step(golden, bb, dataset):
    """One step per call: the parameters after EACH of the 12 steps, the tail batches (steps 5 and 11)
    included."""
    sampler = bb.BlockEpochSampler(N, B, perm=golden["perm"])
    tr = _trainer(bb, dataset, seed=int(golden["train_seed"]), t_max=12)
    buf = _buffer(bb, dataset.transitions())
    for t in range(12):
        loss = tr.train_epoch_steps(buf, sampler, t, 1).cpu().numpy()[0]
        np.testing.assert_allclose(loss, golden["losses"][t], rtol=TOL, err_msg=f"step {t}")
        _check_against_golden(_nets(tr), _golden_tensors(golden, f"step{t}/"), f"step {t}")


# --------------------------------------------------------------------------- #
# 4. the actor
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("policy", ["gaussian", "deterministic"])
def test_act_on_recorded_states(golden, bb, dataset, policy):
    cls = bb.GaussianPolicy if policy == "gaussian" else bb.DeterministicPolicy
    actor = cls(S, A, dataset.max_actions().to(DEV), dataset.min_actions().to(DEV), hidden_dim=16)
    sd = {k[len("eval/actor/"):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("eval/actor/")}
    if policy == "deterministic":
        sd.pop("log_std")
    actor.load_state_dict(sd)
    actor.to(DEV).eval()
    got = np.stack([actor.act(s, DEV) for s in golden["eval/states"]])
    assert got.dtype == np.float32 and got.shape == golden["eval/actions"].shape
    np.testing.assert_allclose(got, golden["eval/actions"], rtol=TOL, atol=TOL)
    lo, hi = dataset.min_actions().numpy(), dataset.max_actions().numpy()
    assert (got[:, 0] == lo[0]).any() and (got[:, 0] == hi[0]).any() and (got[:, 0] >= lo[0]).all() \
        and (got[:, 0] <= hi[0]).all()
    assert ((got[:, 0] > lo[0]) & (got[:, 0] < hi[0])).any()


# --------------------------------------------------------------------------- #
# 5. train()
# --------------------------------------------------------------------------- #
def test_train_end_to_end(golden, bb, tmp_path):
    config = bb.TrainConfig(update_steps=12, eval_every=6, batch_size=B, normalize_state=True, normalize_reward=True,
                            eval_episodes=2, train_seed=int(golden["train_seed"]), eval_seed=4,
                            checkpoints_path=str(tmp_path))
    records = []
    seeds = []
    real_eval = bb.bb_run_eval_IQL

    def spy(**kw):
        seeds.append(kw["seed"])
        return real_eval(**dict(kw, max_horizon=40))

    bb.bb_run_eval_IQL = spy
    try:
        tr = bb.train(config, {k[5:]: v for k, v in golden.items() if k.startswith("data/")}, bb_env.numpy_reward,
                      bb_env.MOVE_STATS, logger=lambda d, step: records.extend((int(step), k, float(v)) for k, v in d.items()),
                      perm=golden["perm"], device=DEV, chunk=4)
    finally:
        bb.bb_run_eval_IQL = real_eval
    want = []
    for t in range(12):
        want += [(t, k) for k in LOSSES]
        if t in (5, 11):
            want += [(t, k) for k in ("evaluation_return", "best_score_so_far", "best_step_so_far")]
    assert [(s, k) for s, k, _ in records] == want
    assert seeds == [4 + 5, 4 + 11]  # eval_seed + step
    losses = np.asarray([v for _, k, v in records if k in LOSSES]).reshape(12, 3)
    np.testing.assert_allclose(losses, golden["losses"], rtol=TOL)
    vals = {(s, k): v for s, k, v in records}
    assert vals[(5, "best_step_so_far")] == 5 and vals[(5, "best_score_so_far")] == vals[(5, "evaluation_return")]
    assert vals[(11, "best_score_so_far")] == max(vals[(5, "evaluation_return")], vals[(11, "evaluation_return")])
    files = sorted(os.listdir(config.checkpoints_path))
    assert files == ["best_model.pt", "checkpoint_11.pt", "checkpoint_5.pt", "config.yaml"]
    sd = torch.load(os.path.join(config.checkpoints_path, "checkpoint_11.pt"), weights_only=True)
    assert set(sd) == {"qf", "q_optimizer", "vf", "v_optimizer", "actor", "actor_optimizer", "actor_lr_scheduler"}
    assert sd["actor_lr_scheduler"]["last_epoch"] == 12 and tr.total_it == 12
    assert tr.actor.training and tr.launch_counts()[0] == 12


# --------------------------------------------------------------------------- #
# 6. where counts are not supported
# --------------------------------------------------------------------------- #
def test_general_step_refuses_counts_before_any_launch(bb, dataset):
    tr = _trainer(bb, dataset, seed=2, t_max=100, hidden=96)
    assert tr.step_kind(B) == "general"
    buf = _buffer(bb, dataset.transitions())
    before = _tensors(tr)
    idx = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="valid-row counts"):
        tr.train_steps(buf, 2, B, indices=idx, n_valid=torch.tensor([B, 7], dtype=torch.int32, device=DEV))
    assert tr.launch_counts() == (0, 0) and tr.total_it == 0
    after = _tensors(tr)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    tr.train_steps(buf, 2, B, indices=idx)  # the same call without counts runs
    assert tr.total_it == 2


def test_bf16_refuses_counts_before_any_launch(bb, dataset):
    import iqlpref_amd as ia
    torch.manual_seed(2)
    q, v, actor = ia.TwinQ(S, A).to(DEV), ia.ValueFunction(S).to(DEV), ia.GaussianPolicy(S, A, 1.0).to(DEV)
    tr = ia.ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), q,
                              torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                              device=DEV, precision="bf16", seed=2)
    buf = _buffer(bb, dataset.transitions())
    idx = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        tr.train_steps(buf, 2, B, indices=idx, n_valid=torch.tensor([B, 7], dtype=torch.int32, device=DEV))
    assert tr.launch_counts() == (0, 0) and tr.total_it == 0


def test_count_dtype_is_checked(bb, dataset):
    buf = _buffer(bb, dataset.transitions())
    idx = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        _trainer(bb, dataset, seed=2, t_max=100).train_steps(
            buf, 2, B, indices=idx, n_valid=torch.tensor([B, 7], dtype=torch.int64, device=DEV))
