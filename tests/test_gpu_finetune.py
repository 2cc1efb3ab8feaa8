"""Online fine-tuning (iqlpref_amd.finetune, csrc/online.hip) on the GPU.  -m gpu.

1. iqlhip_replay_append: byte for byte what iqlhip_replay_pack writes into the same rows;
2. iqlhip_np_randint_growing: bit for bit numpy's RandomState.randint called step by step, state included;
3. iqlhip_explore_action against a float64 numpy restatement at the fp32 bound 2e-5;
4. finetune.train() replays tests/golden/finetune_run.npz -- two runs of the reference's own train() on the
   CPU (make_finetune_fixture.py) -- record for record, on an environment that plays the recording back;
5. the refusals leave everything as it was.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib
from iqlpref_amd import custom_offline as co
from oracle import philox
from tests import finetune_env as fe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_BOUND = 2e-5  # the project's fp32 bound (exact-fp32 MFMA against float64)


def _ft():
    from iqlpref_amd import finetune
    return finetune


# --------------------------------------------------------------------------- #
# append
# --------------------------------------------------------------------------- #
S_, A_ = 5, 3


def _transitions(n, seed):
    rng = np.random.default_rng(seed)
    return {"observations": rng.standard_normal((n, S_)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (n, A_)).astype(np.float32),
            "rewards": rng.standard_normal(n).astype(np.float32),
            "next_observations": rng.standard_normal((n, S_)).astype(np.float32),
            "terminals": (rng.uniform(size=n) < 0.3).astype(np.float32)}


def _pack_into(rows, first, d, sel):
    """iqlhip_replay_pack of the transitions ``sel`` of ``d`` into rows[first ...]."""
    lib = _lib.load()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x[sel])).to(DEV)
    t = [up(d[k]) for k in ("observations", "actions", "rewards", "next_observations", "terminals")]
    with torch.cuda.device(DEV):
        _lib.check(lib.iqlhip_replay_pack(_lib.ptr(rows), rows.shape[1], S_, A_, first, len(sel),
                                          *[_lib.ptr(x) for x in t], _lib.stream_ptr()))
    torch.cuda.synchronize()


def _expected_ring(cap, loaded, new):
    stride = _lib.load().iqlhip_replay_row_stride(S_, A_)
    rows = torch.zeros((cap, stride), dtype=torch.float32, device=DEV)
    if len(loaded["rewards"]):
        _pack_into(rows, 0, loaded, list(range(len(loaded["rewards"]))))
    p = len(loaded["rewards"])
    for i in range(len(new["rewards"])):
        _pack_into(rows, (p + i) % cap, new, [i])
    return rows


@pytest.mark.parametrize("how", ["one_at_a_time", "one_call"])
def test_append_wraps_and_equals_pack(how):
    ft = _ft()
    loaded, new = _transitions(37, 1), _transitions(7, 2)
    buf = ft.ReplayBuffer(S_, A_, 40, DEV)
    buf.load_d4rl_dataset({k: v.copy() for k, v in loaded.items()})
    assert (buf._pointer, buf._size) == (37, 37)
    gen0 = buf.view().generation
    if how == "one_at_a_time":
        for i in range(7):
            buf.add_transition(new["observations"][i], new["actions"][i], float(new["rewards"][i]),
                               new["next_observations"][i], bool(new["terminals"][i]))
    else:
        up = lambda k: torch.from_numpy(new[k]).to(DEV)
        buf.append_device(up("observations"), up("actions"), up("rewards"), up("next_observations"), up("terminals"))
    torch.cuda.synchronize()
    assert (buf._pointer, buf._size) == (4, 40)
    assert buf.view().generation != gen0 and buf.view().n_rows == 40
    want = _expected_ring(40, loaded, new)
    got = buf._rows.cpu().numpy()
    assert got.tobytes() == want.cpu().numpy().tobytes()
    # rows the appends did not address are what the load wrote
    only_loaded = _expected_ring(40, loaded, _transitions(0, 0))
    assert got[4:37].tobytes() == only_loaded.cpu().numpy()[4:37].tobytes()
    np.testing.assert_array_equal(buf._states.cpu().numpy()[:4], new["observations"][3:])
    np.testing.assert_array_equal(buf._next_states.cpu().numpy()[37:], new["next_observations"][:3])


def test_append_capacity_one():
    ft = _ft()
    new = _transitions(2, 3)
    buf = ft.ReplayBuffer(S_, A_, 1, DEV)
    for i in range(2):
        buf.add_transition(new["observations"][i], new["actions"][i], float(new["rewards"][i]),
                           new["next_observations"][i], bool(new["terminals"][i]))
        torch.cuda.synchronize()
        assert (buf._pointer, buf._size) == (0, 1)
        want = _expected_ring(1, _transitions(0, 0), {k: v[i:i + 1] for k, v in new.items()})
        assert buf._rows.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def _small_trainer(ft, S, A, *, deterministic=False, n_hidden=2, hidden=64, seed=5, dropout=None, precision="fp32"):
    import iqlpref_amd as ia
    torch.manual_seed(seed)
    q = ia.TwinQ(S, A, hidden, n_hidden).to(DEV)
    v = ia.ValueFunction(S, hidden, n_hidden).to(DEV)
    pol = ia.DeterministicPolicy if deterministic else ia.GaussianPolicy
    actor = pol(S, A, 1.5, hidden, n_hidden, dropout=dropout).to(DEV)
    return ft.ImplicitQLearning(1.5, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), q,
                                torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                                max_steps=10, device=DEV, seed=seed, precision=precision)


def test_sample_after_append_sees_the_new_row():
    """A 3-row ring holding 2 rows: a step, then a transition goes in, and both the sampler and the next step
    (on injected indices that all hit the new row) see it; the view's size and generation moved.  That a batch
    staged before an append is not used is test_append_invalidates_the_staged_batch's to show."""
    ft = _ft()
    loaded, new = _transitions(2, 4), _transitions(1, 5)
    all3 = {k: np.concatenate([loaded[k], new[k]]) for k in loaded}
    idx0 = torch.zeros((1, 16), dtype=torch.int64, device=DEV)
    idx2 = torch.full((1, 16), 2, dtype=torch.int64, device=DEV)
    out = []
    for grown in (True, False):
        tr = _small_trainer(ft, S_, A_)
        buf = ft.ReplayBuffer(S_, A_, 3, DEV)
        buf.load_d4rl_dataset({k: v.copy() for k, v in (loaded if grown else all3).items()})
        first = tr.train_steps(buf, 1, 16, indices=idx0)
        if grown:
            gen = buf.view().generation
            buf.add_transition(new["observations"][0], new["actions"][0], float(new["rewards"][0]),
                               new["next_observations"][0], bool(new["terminals"][0]))
            assert buf.view().generation != gen and buf.view().n_rows == 3
            s, a, r, s2, d = buf.sample(16, indices=idx2[0])
            np.testing.assert_array_equal(s.cpu().numpy(), np.repeat(new["observations"], 16, 0))
            np.testing.assert_array_equal(a.cpu().numpy(), np.repeat(new["actions"], 16, 0))
            np.testing.assert_array_equal(r.cpu().numpy()[:, 0], np.repeat(new["rewards"], 16))
            np.testing.assert_array_equal(s2.cpu().numpy(), np.repeat(new["next_observations"], 16, 0))
            np.testing.assert_array_equal(d.cpu().numpy()[:, 0], np.repeat(new["terminals"], 16))
        second = tr.train_steps(buf, 1, 16, indices=idx2)
        out.append(torch.cat([first, second]).cpu())
    assert torch.equal(out[0], out[1])


def test_append_invalidates_the_staged_batch():
    """A full 3-row ring stepped with device-drawn indices and no loss output -- the calls that continue one
    another on the batch the previous step staged.  An append overwrites row 0 (same rows, same size: only the
    view's generation tells the library), and the next step must train on the new row: it equals a step on
    injected copies of the same indices, which always gathers afresh."""
    ft = _ft()
    loaded, new = _transitions(2, 4), _transitions(2, 5)
    new["observations"][1] += 50.0  # (the row that replaces row 0 is far from the old one)
    add = lambda buf, i: buf.add_transition(new["observations"][i], new["actions"][i], float(new["rewards"][i]),
                                            new["next_observations"][i], bool(new["terminals"][i]))
    idx1 = torch.from_numpy(philox.sample_indices(5, 1, 16, 3)[None]).to(DEV)
    assert (idx1 == 0).any()  # step 1 reads the rewritten row
    runs = {}
    for how in ("continued", "injected", "control_continued", "control_injected"):
        tr = _small_trainer(ft, S_, A_, seed=5)
        buf = ft.ReplayBuffer(S_, A_, 3, DEV)
        buf.load_d4rl_dataset({k: v.copy() for k, v in loaded.items()})
        add(buf, 0)  # full: pointer back at row 0
        assert (buf._pointer, buf._size) == (0, 3)
        tr.train_steps(buf, 1, 16, return_losses=False)  # step 0, stages step 1's batch
        if not how.startswith("control"):
            add(buf, 1)
        if how.endswith("continued"):
            tr.train_steps(buf, 1, 16, return_losses=False)
        else:
            tr.train_steps(buf, 1, 16, indices=idx1, return_losses=False)
        torch.cuda.synchronize()
        runs[how] = torch.cat([p.detach().reshape(-1).clone() for p in tr.actor.parameters()] +
                              [p.detach().reshape(-1).clone() for p in tr.qf.parameters()])
    # the control pins the restated indices: without an append both ways are the same step
    assert torch.equal(runs["control_continued"], runs["control_injected"])
    assert not torch.equal(runs["continued"], runs["control_continued"])  # the new row mattered
    assert torch.equal(runs["continued"], runs["injected"])


# --------------------------------------------------------------------------- #
# growing draw
# --------------------------------------------------------------------------- #
def _grow_device(rss, hi0, cap, growth, n, B):
    lib = _lib.load()
    K = len(rss)
    state = torch.from_numpy(np.stack([co.pack_np_state(r.get_state()) for r in rss]).view(np.int32)).to(DEV)
    outs = [torch.full((n, B), -7, dtype=torch.int64, device=DEV) for _ in range(K)]
    with torch.cuda.device(DEV):
        _lib.check(lib.iqlhip_np_randint_growing(_lib.ptr(state), (C.c_int64 * K)(*hi0), (C.c_int64 * K)(*cap), growth,
                                                 K, B, n, (C.c_void_p * K)(*[o.data_ptr() for o in outs]),
                                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], state.cpu().numpy().view(np.uint32)


def _grow_host(rs, hi0, cap, growth, n, B):
    return np.stack([rs.randint(0, min(hi0 + t * growth, cap), size=B) for t in range(n)])


GROW_CASES = {  # (hi0, cap, growth, n_steps, B)
    "mask_changes_at_256": (250, 10 ** 6, 1, 20, 16),
    "first_step_draws_nothing": (1, 10 ** 6, 1, 12, 16),
    "cap_reached_mid_call": (60, 70, 1, 25, 16),
    "three_rounds_of_624": (300, 10 ** 6, 1, 6, 256),
    "stands_at_one": (1, 1, 1, 3, 16),
}


@pytest.mark.parametrize("case", sorted(GROW_CASES))
@pytest.mark.parametrize("start", ["fresh", "mid_key"])
def test_growing_draw_matches_numpy(case, start):
    hi0, cap, growth, n, B = GROW_CASES[case]

    def gen():
        rs = np.random.RandomState(11)
        if start == "mid_key":
            rs.randint(0, 2 ** 32, size=300)
        return rs
    (got,), state = _grow_device([gen()], [hi0], [cap], growth, n, B)
    host = gen()
    want = _grow_host(host, hi0, cap, growth, n, B)
    np.testing.assert_array_equal(got, want)
    ws = co.pack_np_state(host.get_state())
    assert int(state[0][624]) == int(ws[624])
    np.testing.assert_array_equal(state[0][:624], ws[:624])


def test_growing_draw_without_growth_is_np_randint():
    lib = _lib.load()
    n, B, hi = 9, 100, 496113
    (got,), state = _grow_device([np.random.RandomState(3)], [hi], [hi], 0, n, B)
    st2 = torch.from_numpy(co.pack_np_state(np.random.RandomState(3).get_state())[None].view(np.int32)).to(DEV)
    out = torch.empty((n, B), dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.iqlhip_np_randint(_lib.ptr(st2), (C.c_int64 * 1)(hi), 1, B, n, (C.c_void_p * 1)(out.data_ptr()),
                                         _lib.stream_ptr()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, out.cpu().numpy())
    np.testing.assert_array_equal(state[0], st2.cpu().numpy().view(np.uint32)[0])
    host = np.random.RandomState(3)
    np.testing.assert_array_equal(got, _grow_host(host, hi, hi, 0, n, B))


def test_growing_draw_three_streams():
    hi0, cap, n, B = [250, 1, 5000], [300, 8, 5003], 20, 16
    rss = [np.random.RandomState(40 + k) for k in range(3)]
    got, state = _grow_device(rss, hi0, cap, 1, n, B)
    for k in range(3):
        host = np.random.RandomState(40 + k)
        np.testing.assert_array_equal(got[k], _grow_host(host, hi0[k], cap[k], 1, n, B), err_msg=f"stream {k}")
        np.testing.assert_array_equal(state[k], co.pack_np_state(host.get_state()), err_msg=f"state {k}")


def test_growing_index_stream_advances_the_generator():
    ft = _ft()
    rs, host = np.random.RandomState(8), np.random.RandomState(8)
    rs.standard_normal()  # a cached gaussian that no draw may touch
    host.standard_normal()
    (idx,) = ft.GrowingIndexStream(DEV).draw(51, 80, 40, 16, generators=[rs])
    np.testing.assert_array_equal(idx.cpu().numpy(), _grow_host(host, 51, 80, 1, 40, 16))
    a, b = rs.get_state(), host.get_state()
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2:] == b[2:]


# --------------------------------------------------------------------------- #
# exploration action
# --------------------------------------------------------------------------- #
def _actor_f64(tr, states, keeps=None, p=0.0):
    """The actor's forward in float64 from the live parameters; ``keeps``: per hidden layer keep masks."""
    lin = tr.actor.net.linears()
    x = np.asarray(states, np.float64)
    for l, m in enumerate(lin):
        x = x @ m.weight.detach().cpu().double().numpy().T + m.bias.detach().cpu().double().numpy()
        if l < len(lin) - 1:
            x = np.maximum(x, 0.0)
            if keeps is not None:
                x = x * keeps[l] * np.float64(np.float32(1.0) / np.float32(1.0 - p))
    return np.tanh(x)


def _explore_f64(tr, states, eps, expl_noise, noise_clip, deterministic, **kw):
    out = _actor_f64(tr, states, **kw)
    eps = np.asarray(eps, np.float64)
    if deterministic:
        a = out + np.clip(np.float64(np.float32(expl_noise)) * eps, -np.float64(np.float32(noise_clip)),
                          np.float64(np.float32(noise_clip)))
    else:
        ls = np.clip(tr.actor.log_std.detach().cpu().double().numpy(), -20.0, 2.0)
        a = out + np.exp(ls) * eps
    return np.clip(1.5 * a, -1.5, 1.5)


@pytest.mark.parametrize("rows", [1, 25])
@pytest.mark.parametrize("shape", ["tuned", "general"])
@pytest.mark.parametrize("deterministic", [False, True], ids=["gaussian", "deterministic"])
def test_explore_action_matches_float64(deterministic, shape, rows):
    ft = _ft()
    S, A = 11, 3
    n_hidden, hidden = (2, 64) if shape == "tuned" else (3, 40)
    tr = _small_trainer(ft, S, A, deterministic=deterministic, n_hidden=n_hidden, hidden=hidden)
    assert tr.step_kind(16) == shape
    if not deterministic:
        with torch.no_grad():
            tr.actor.log_std.copy_(torch.tensor([-0.7, 0.2, 3.0]))  # (the last one beyond LOG_STD_MAX)
    rng = np.random.default_rng(rows)
    states = rng.standard_normal((rows, S)).astype(np.float32)
    eps = rng.standard_normal((rows, A)).astype(np.float32)
    eps[0, 0] = 40.0  # far enough to hit the noise clip and the action clamp
    if rows > 1:
        eps[1] = -40.0
    noise, clip = (0.3, 0.25) if deterministic else (0.03, 0.5)
    got = tr.explore_action(states, eps, expl_noise=noise, noise_clip=clip).cpu().numpy()
    want = _explore_f64(tr, states, eps, noise, clip, deterministic)
    err = np.abs(got - want).max()
    print(f"explore_action {shape} rows={rows}: max |err| = {err:.3e}")
    assert got.shape == (rows, A) and err <= FP32_BOUND
    if deterministic:  # the clip held the noise: the action is out +- clip, scaled
        out = _actor_f64(tr, states)
        assert abs(got[0, 0] - min(1.5 * (out[0, 0] + clip), 1.5)) <= FP32_BOUND
    else:
        assert got[0, 0] == 1.5 and (rows == 1 or (got[1] == -1.5).all())  # the clamp at max_action
    # the weights are live: one training step moves the action
    buf = ft.ReplayBuffer(S, A, 64, DEV)
    d = {"observations": rng.standard_normal((64, S)).astype(np.float32),
         "actions": rng.uniform(-1, 1, (64, A)).astype(np.float32), "rewards": rng.standard_normal(64).astype(np.float32),
         "next_observations": rng.standard_normal((64, S)).astype(np.float32), "terminals": np.zeros(64, np.float32)}
    buf.load_d4rl_dataset(d)
    tr.train_steps(buf, 1, 16)
    after = tr.explore_action(states, eps, expl_noise=noise, noise_clip=clip).cpu().numpy()
    assert not np.array_equal(after, got)
    assert np.abs(after - _explore_f64(tr, states, eps, noise, clip, deterministic)).max() <= FP32_BOUND


def _philox_normals(seed, call, rows, A):
    """The standard normals iqlhip_explore_action draws itself (include/iqlhip.h), in float64."""
    nq = (A + 3) // 4
    r = philox.philox4x32_10(np.repeat(np.arange(rows, dtype=np.uint32), nq), np.uint32(call),
                             np.tile(np.arange(nq, dtype=np.uint32), rows), np.uint32(4), seed & 0xFFFFFFFF, seed >> 32)
    x, y, z, w = [v.astype(np.float64) for v in r]
    out = np.empty((rows * nq, 4))
    for k, (ua, ub) in enumerate(((x, y), (z, w))):
        rad, ang = np.sqrt(-2.0 * np.log((ua + 1.0) / 2.0 ** 32)), 2.0 * np.pi * ub / 2.0 ** 32
        out[:, 2 * k], out[:, 2 * k + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(rows, nq * 4)[:, :A]


@pytest.mark.parametrize("deterministic", [False, True], ids=["gaussian", "deterministic"])
def test_explore_action_draws_its_own_noise(deterministic):
    ft = _ft()
    S, A, rows = 11, 6, 25
    tr = _small_trainer(ft, S, A, deterministic=deterministic, seed=9)
    states = np.random.default_rng(0).standard_normal((rows, S)).astype(np.float32)
    for call in range(2):  # a fresh block of noise per call
        got = tr.explore_action(states, None, expl_noise=0.2, noise_clip=0.5).cpu().numpy()
        eps = _philox_normals(9, call, rows, A)
        want = _explore_f64(tr, states, eps.astype(np.float32), 0.2, 0.5, deterministic)
        assert np.abs(got - want).max() <= FP32_BOUND, f"call {call}"


def test_explore_action_with_actor_dropout_drops_units():
    """The reference never takes the actor out of train mode for the exploring forward (finetune/iql.py:681;
    only eval_actor switches, and switches back): with actor_dropout the forward drops hidden units."""
    ft = _ft()
    S, A, rows, p = 11, 3, 25, 0.25
    tr = _small_trainer(ft, S, A, dropout=p, seed=13)
    rng = np.random.default_rng(1)
    states, eps = rng.standard_normal((rows, S)).astype(np.float32), rng.standard_normal((rows, A)).astype(np.float32)
    for call in range(2):
        got = tr.explore_action(states, eps, expl_noise=0.03, noise_clip=0.5).cpu().numpy()
        keeps = [philox.mlp_dropout_keep(13, call, l, rows, 64, p).astype(np.float64) for l in range(2)]
        want = _explore_f64(tr, states, eps, 0.03, 0.5, False, keeps=keeps, p=p)
        assert np.abs(got - want).max() <= FP32_BOUND, f"call {call}"


# --------------------------------------------------------------------------- #
# the reference's run, record for record
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "finetune_run.npz")))


INT_KEYS = ("offline_iter", "online_iter", "train/episode_length", "train/is_success", "eval/success_rate")


def _check_nets(sd, g, prefix, exact):
    """Every parameter tensor against what the fixture kept of it (make_finetune_fixture.sample_of: the whole
    tensor up to 4096 elements, else every 61st element): the same bits, or each element within the fp32 bound."""
    for net in ("qf", "vf", "actor"):
        for k, v in sd[net].items():
            flat = v.detach().cpu().reshape(-1).numpy()
            got, want = (flat if flat.size <= 4096 else flat[::61]), g[f"{prefix}/{net}/{k}"]
            assert got.shape == want.shape, f"{prefix}/{net}/{k}"
            if exact:
                np.testing.assert_array_equal(got, want, err_msg=f"{prefix}/{net}/{k}")
            else:
                np.testing.assert_allclose(got, want, rtol=0, atol=FP32_BOUND, err_msg=f"{prefix}/{net}/{k}")


@pytest.mark.parametrize("name", ["gauss", "det"])
@pytest.mark.parametrize("online_chunk", [256, 7])
def test_replays_reference_finetune(name, online_chunk, golden, tmp_path):
    ft = _ft()
    g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    c = {k[len("common/"):]: int(v) for k, v in golden.items() if k.startswith("common/")}
    env_name, det = str(g["env_name"]), bool(g["deterministic"])
    env, eval_env = fe.ReplayEnv(env_name, g, "env"), fe.ReplayEnv(env_name, g, "eval_env")
    dataset = {k[len("dataset/"):]: v.copy() for k, v in g.items() if k.startswith("dataset/")}
    config = ft.TrainConfig(device=DEV, env=env_name, seed=int(g["seed"]), eval_seed=c["eval_seed"],
                            eval_freq=c["eval_freq"], n_episodes=c["n_episodes"],
                            offline_iterations=c["offline_iterations"], online_iterations=c["online_iterations"],
                            checkpoints_path=str(tmp_path), buffer_size=c["buffer_size"], batch_size=c["batch_size"],
                            iql_deterministic=det, normalize_reward=bool(g["normalize_reward"]))
    records, saves, idx_seen, lrs, box = [], [], [], [], {}
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        box[os.path.basename(path)] = {n: {k: v.clone() for k, v in obj[n].items()} for n in ("qf", "vf", "actor")}
        box[os.path.basename(path) + "/meta"] = (obj["total_it"], obj["actor_lr_schedule"]["last_epoch"])
        real_save(obj, path)

    def on_start(trainer, buf):
        _check_nets({"qf": trainer.qf.state_dict(), "vf": trainer.vf.state_dict(), "actor": trainer.actor.state_dict()},
                    g, "init", exact=True)
        real_steps = trainer.train_steps

        def train_steps(rb, n, B, *, indices=None, **kw):
            idx_seen.append(indices.cpu().numpy().copy())
            lrs.extend(ft.cosine_rate(3e-4, trainer.total_it + i, trainer._max_steps) for i in range(n))
            assert trainer.actor_optimizer.param_groups[0]["lr"] == lrs[-n]  # the host bookkeeping's rate
            return real_steps(rb, n, B, indices=indices, **kw)
        trainer.train_steps = train_steps
        box["buf"] = buf

    torch.save = save
    try:
        trainer = ft.train(config, env, eval_env, dataset, device=DEV,
                           logger=lambda d, step: records.extend((int(step), k, float(v)) for k, v in d.items()),
                           online_chunk=online_chunk, exploration_noise=lambda tick: g["eps"][tick], on_start=on_start)
    finally:
        torch.save = real_save
    torch.cuda.synchronize()
    assert env.exhausted() and eval_env.exhausted()
    assert env.seeds == g["env/seeds"].tolist() and eval_env.seeds == g["eval_env/seeds"].tolist()

    # exactly: indices, numpy's generator, the buffer, log keys and steps, integer and boolean entries, saves
    np.testing.assert_array_equal(np.concatenate(idx_seen), g["idx"])
    st = np.random.get_state()
    np.testing.assert_array_equal(st[1], g["np_key"])
    assert st[2] == g["np_pos"]
    buf = box["buf"]
    assert (buf._pointer, buf._size) == (int(g["buf_pointer"]), int(g["buf_size"]))
    np.testing.assert_array_equal(buf._states.cpu().numpy(), g["buf_states"])
    np.testing.assert_array_equal(buf._rewards.cpu().numpy(), g["buf_rewards"])
    np.testing.assert_array_equal(buf._next_states.cpu().numpy(), g["buf_next_states"])
    np.testing.assert_array_equal(buf._dones.cpu().numpy(), g["buf_dones"])
    keys = np.asarray([r[1] for r in records])
    vals = np.asarray([r[2] for r in records], np.float64)
    np.testing.assert_array_equal(keys, g["rec_key"])
    np.testing.assert_array_equal([r[0] for r in records], g["rec_step"])
    exact = np.isin(keys, INT_KEYS)
    np.testing.assert_array_equal(vals[exact], g["rec_value"][exact])
    np.testing.assert_array_equal([s[0] for s in saves], g["save_step"])
    np.testing.assert_array_equal([s[1] for s in saves], g["save_name"])

    # within the fp32 bound: proposed actions (exploring and evaluating), losses, parameters at checkpoints;
    # the buffer's action columns are those proposed actions
    act_err = np.abs(np.asarray(env.actions) - g["env/actions"]).max()
    eval_err = np.abs(np.asarray(eval_env.actions) - g["eval_env/actions"]).max()
    loss = np.isin(keys, ("value_loss", "q_loss", "actor_loss"))
    rel = np.abs(vals[loss] - g["rec_value"][loss]) / np.maximum(np.abs(g["rec_value"][loss]), 1e-30)
    print(f"{name}: actions {act_err:.3e}, eval actions {eval_err:.3e}, losses rel {rel.max():.3e}")
    assert act_err <= FP32_BOUND and eval_err <= FP32_BOUND
    np.testing.assert_allclose(buf._actions.cpu().numpy(), g["buf_actions"], rtol=0, atol=FP32_BOUND)
    # (losses: the bound relative to the value -- the q losses of the scaled-reward run are ~2e4, whose fp32
    # spacing alone is 2e-3; the atol covers value losses of ~1e-4, as in test_gpu_custom_train.py)
    np.testing.assert_allclose(vals[loss], g["rec_value"][loss], rtol=FP32_BOUND, atol=2e-8)
    np.testing.assert_allclose(np.asarray(lrs), g["actor_lr"], rtol=0, atol=4 * 6.02e-18)  # (test_finetune_host.py)
    rest = ~loss & ~exact  # returns, scores and regrets: functions of the replayed rewards alone
    np.testing.assert_allclose(vals[rest], g["rec_value"][rest], rtol=1e-12, atol=1e-12)
    for fname in g["save_name"].tolist():
        _check_nets(box[fname], g, f"ckpt/{fname}", exact=False)
        assert box[fname + "/meta"] == (int(g[f"ckpt/{fname}/total_it"]), int(g[f"ckpt/{fname}/last_epoch"]))
        assert os.path.exists(os.path.join(config.checkpoints_path, fname))
    assert trainer.total_it == c["offline_iterations"] + c["online_iterations"]


# --------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------- #
def test_refusals_leave_everything_as_it_was():
    ft = _ft()
    lib = _lib.load()
    # a bf16 trainer: the Python method and the entry point itself
    tr = _small_trainer(ft, S_, A_, precision="bf16")
    states = torch.zeros((2, S_), device=DEV)
    with pytest.raises(NotImplementedError):
        tr.explore_action(states)
    tr._ensure_handle(16)
    out = torch.full((2, A_), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.iqlhip_explore_action(tr._handle, _lib.ptr(states), 2, None, 0.03, 0.5, 1.5, 0, _lib.ptr(out),
                                       _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and (out == -7.0).all()
    assert tr._explore_calls == 0
    # more transitions than the ring holds
    loaded = _transitions(3, 6)
    buf = ft.ReplayBuffer(S_, A_, 4, DEV)
    buf.load_d4rl_dataset({k: v.copy() for k, v in loaded.items()})
    before, gen = buf._rows.clone(), buf.view().generation
    five = _transitions(5, 7)
    up = lambda k: torch.from_numpy(five[k]).to(DEV)
    with pytest.raises(ValueError):
        buf.append_device(up("observations"), up("actions"), up("rewards"), up("next_observations"), up("terminals"))
    t = [up(k) for k in ("observations", "actions", "rewards", "next_observations", "terminals")]
    with torch.cuda.device(DEV):
        rc = lib.iqlhip_replay_append(_lib.ptr(buf._rows), buf._stride, S_, A_, 4, 3, 5, *[_lib.ptr(x) for x in t],
                                      _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID
    assert torch.equal(buf._rows, before) and (buf._pointer, buf._size) == (3, 3) and buf.view().generation == gen
    # a bound below 1
    rs = np.random.RandomState(2)
    key, pos = rs.get_state()[1].copy(), rs.get_state()[2]
    with pytest.raises(ValueError):
        ft.GrowingIndexStream(DEV).draw(0, 10, 4, 16, generators=[rs])
    assert rs.get_state()[2] == pos and np.array_equal(rs.get_state()[1], key)
    state = torch.from_numpy(co.pack_np_state(rs.get_state())[None].view(np.int32)).to(DEV)
    keep = state.clone()
    o = torch.full((4, 16), -7, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.iqlhip_np_randint_growing(_lib.ptr(state), (C.c_int64 * 1)(0), (C.c_int64 * 1)(10), 1, 1, 16, 4,
                                           (C.c_void_p * 1)(o.data_ptr()), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and torch.equal(state, keep) and (o == -7).all()
    # the offline buffer still has no add_transition
    import iqlpref_amd as ia
    with pytest.raises(NotImplementedError):
        ia.ReplayBuffer(S_, A_, 4, DEV).add_transition()
