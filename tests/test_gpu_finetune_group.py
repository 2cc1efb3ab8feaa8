"""K seeds per GPU for the fine-tune flavour, on the device.  Nothing here has a tolerance:

1. iqlhip_explore_action_group: every member's row has the bits of that member's own iqlhip_explore_action call,
   over both summation orders of the stand-alone MLP kernels, both policies, dropout, drawn and given noise;
2. iqlhip_replay_append_group: K rings byte for byte what add_transition leaves in twin rings;
3. refusals change nothing;
4. finetune.train(seeds_per_gpu=3) is three runs of finetune.train, member for member;
5. the one loop of finetune.train launches the solo calls for one seed and the grouped ones for K > 1, and hands
   the caller of one seed what it always got.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib
from tests import finetune_env as fe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_ACTION = 1.5


def _ft():
    from iqlpref_amd import finetune
    return finetune


def _transitions(n, seed, S, A):
    rng = np.random.default_rng(seed)
    return {"observations": rng.standard_normal((n, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "rewards": rng.standard_normal(n).astype(np.float32),
            "next_observations": rng.standard_normal((n, S)).astype(np.float32),
            "terminals": (rng.uniform(size=n) < 0.3).astype(np.float32)}


def _trainer(ft, S, A, *, deterministic, n_hidden, hidden, seed, dropout=None, precision="fp32"):
    """A trainer whose nets are initialised on the device (16 members of 6 x 1024 in no time)."""
    import iqlpref_amd as ia
    torch.manual_seed(seed)
    with torch.device(DEV):
        q = ia.TwinQ(S, A, hidden, n_hidden)
        v = ia.ValueFunction(S, hidden, n_hidden)
        pol = ia.DeterministicPolicy if deterministic else ia.GaussianPolicy
        actor = pol(S, A, MAX_ACTION, hidden, n_hidden, dropout=dropout)
    return ft.ImplicitQLearning(MAX_ACTION, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), q,
                                torch.optim.Adam(q.parameters(), lr=3e-4), v, torch.optim.Adam(v.parameters(), lr=3e-4),
                                max_steps=10, device=DEV, seed=seed, precision=precision)


def _warm(ft, trainers, S, A):
    """One or two training steps each, so that the weights are the live masters and differ per member."""
    buf = ft.ReplayBuffer(S, A, 64, DEV)
    buf.load_d4rl_dataset(_transitions(64, 11, S, A))
    for k, tr in enumerate(trainers):
        tr.train_steps(buf, 1 + k % 2, 16, return_losses=False)
    torch.cuda.synchronize()


def _solo_rows(trainers, states, eps, **kw):
    return torch.cat([tr.explore_action(states[k:k + 1], None if eps is None else eps[k:k + 1], **kw)
                      for k, tr in enumerate(trainers)])


def _check_group_equals_solo(ft, trainers, seed):
    """Two consecutive calls, given and drawn noise: the group's rows against the members' own calls at the
    same call numbers."""
    K, S, A = len(trainers), trainers[0]._state_dim, trainers[0]._action_dim
    g = torch.Generator().manual_seed(seed)
    kw = dict(expl_noise=0.3, noise_clip=0.5)
    for given in (True, False):
        for _ in range(2):
            states = torch.randn((K, S), generator=g).to(DEV)
            eps = torch.randn((K, A), generator=g).to(DEV) if given else None
            calls = [tr._explore_calls for tr in trainers]
            got = ft.explore_actions(trainers, states, eps, **kw)
            assert [tr._explore_calls for tr in trainers] == [c + 1 for c in calls]
            for tr, c in zip(trainers, calls):
                tr._explore_calls = c
            want = _solo_rows(trainers, states, eps, **kw)
            torch.cuda.synchronize()
            assert got.shape == (K, A) and got.dtype == torch.float32
            for k in range(K):
                assert torch.equal(got[k], want[k]), \
                    f"member {k} of {K} (eps {'given' if given else 'drawn'}, call {calls[k]}): {got[k]} != {want[k]}"
            assert (got.abs() <= MAX_ACTION).all()


# (S, A, n_hidden, hidden)
SHAPES = {
    "tuned_unaligned_first_layer": (5, 3, 2, 64),
    "output_nk3_two_tiles": (16, 17, 1, 40),
    "deep3_w96": (29, 8, 3, 96),
    "narrow_edge_A32": (96, 32, 2, 256),
    "first_wide_width": (5, 3, 2, 264),
    "top_of_envelope": (17, 6, 6, 1024),
}


@pytest.mark.parametrize("deterministic", [False, True], ids=["gaussian", "deterministic"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_act_rows_equal_the_members_own_calls(shape, deterministic):
    """16 members of one shape, the odd ones with actor_dropout = 0.1; groups of 1 (with and without dropout),
    3 and 16 of them."""
    ft = _ft()
    S, A, n_hidden, hidden = SHAPES[shape]
    trainers = [_trainer(ft, S, A, deterministic=deterministic, n_hidden=n_hidden, hidden=hidden, seed=100 + k,
                         dropout=0.1 if k % 2 else None) for k in range(16)]
    _warm(ft, trainers, S, A)
    for members in ([0], [1], [2, 3, 4], list(range(16))):
        _check_group_equals_solo(ft, [trainers[k] for k in members], seed=len(members))
    # the dropout masks are live: a member with dropout acts differently from call to call on one state
    s = torch.ones((1, S), device=DEV)
    e = torch.zeros((1, A), device=DEV)
    a0 = ft.explore_actions([trainers[1]], s, e, expl_noise=0.3, noise_clip=0.5)
    a1 = ft.explore_actions([trainers[1]], s, e, expl_noise=0.3, noise_clip=0.5)
    assert not torch.equal(a0, a1)


def test_act_mixed_group():
    """Depths 1 and 3, widths on both summation orders, Gaussian beside deterministic, dropout beside none."""
    ft = _ft()
    S, A = 11, 5
    spec = [(1, 40, False, None), (3, 96, True, None), (2, 264, False, 0.1), (3, 64, True, 0.1), (1, 1024, False, None)]
    trainers = [_trainer(ft, S, A, deterministic=det, n_hidden=nh, hidden=h, seed=7 + k, dropout=p)
                for k, (nh, h, det, p) in enumerate(spec)]
    _warm(ft, trainers, S, A)
    _check_group_equals_solo(ft, trainers, seed=3)
    _check_group_equals_solo(ft, trainers[::-1], seed=4)


# --------------------------------------------------------------------------- #
# append
# --------------------------------------------------------------------------- #
S_, A_ = 5, 3
CAPS, LOADED = (1, 7, 40), (0, 6, 39)  # every pointer on its ring's last row: the next append wraps


def _rings(ft):
    bufs = []
    for cap, n in zip(CAPS, LOADED):
        b = ft.ReplayBuffer(S_, A_, cap, DEV)
        if n:
            b.load_d4rl_dataset(_transitions(n, 20 + cap, S_, A_))
        bufs.append(b)
    return bufs


def test_append_group_equals_add_transition():
    ft = _ft()
    bufs, twins = _rings(ft), _rings(ft)
    assert [b._pointer for b in bufs] == [0, 6, 39]
    for rnd in range(3):
        new = _transitions(3, 30 + rnd, S_, A_)
        gens = [b.view().generation for b in bufs]
        ft.add_transitions(bufs, new["observations"], new["actions"], new["rewards"], new["next_observations"],
                           new["terminals"])
        for k, tw in enumerate(twins):
            tw.add_transition(new["observations"][k], new["actions"][k], float(new["rewards"][k]),
                              new["next_observations"][k], bool(new["terminals"][k]))
        torch.cuda.synchronize()
        for k, (b, tw) in enumerate(zip(bufs, twins)):
            assert (b._pointer, b._size) == (tw._pointer, tw._size), (rnd, k)
            assert b._rows.cpu().numpy().tobytes() == tw._rows.cpu().numpy().tobytes(), (rnd, k)  # the whole matrix
            assert b.view().generation != gens[k] and b.view().n_rows == tw._size
    assert [(b._pointer, b._size) for b in bufs] == [(0, 1), (2, 7), (2, 40)]


def test_sample_and_step_see_the_group_append():
    """test_gpu_finetune.py's two solo checks with the append made by add_transitions: the sampler and the next
    step see the new row, and a batch staged before the append is not used."""
    from oracle import philox
    ft = _ft()
    loaded, new = _transitions(2, 4, S_, A_), _transitions(2, 5, S_, A_)
    new["observations"][1] += 50.0
    other_new = _transitions(2, 6, S_, A_)

    def add(buf, other, i):
        pick = lambda name: [new[name][i], other_new[name][i]]
        ft.add_transitions([buf, other], pick("observations"), pick("actions"), pick("rewards"),
                           pick("next_observations"), pick("terminals"))

    idx1 = torch.from_numpy(philox.sample_indices(5, 1, 16, 3)[None]).to(DEV)
    assert (idx1 == 0).any()
    runs = {}
    for how in ("continued", "injected", "control_continued", "control_injected"):
        tr = _trainer(ft, S_, A_, deterministic=False, n_hidden=2, hidden=64, seed=5)
        buf, other = ft.ReplayBuffer(S_, A_, 3, DEV), ft.ReplayBuffer(S_, A_, 9, DEV)
        buf.load_d4rl_dataset({k: v.copy() for k, v in loaded.items()})
        other.load_d4rl_dataset(_transitions(4, 8, S_, A_))
        add(buf, other, 0)
        assert (buf._pointer, buf._size) == (0, 3) and (other._pointer, other._size) == (5, 5)
        s, a, r, s2, d = buf.sample(16, indices=torch.full((16,), 2, dtype=torch.int64, device=DEV))
        np.testing.assert_array_equal(s.cpu().numpy(), np.repeat(new["observations"][:1], 16, 0))
        np.testing.assert_array_equal(a.cpu().numpy(), np.repeat(new["actions"][:1], 16, 0))
        np.testing.assert_array_equal(r.cpu().numpy()[:, 0], np.repeat(new["rewards"][:1], 16))
        np.testing.assert_array_equal(s2.cpu().numpy(), np.repeat(new["next_observations"][:1], 16, 0))
        np.testing.assert_array_equal(d.cpu().numpy()[:, 0], np.repeat(new["terminals"][:1], 16))
        tr.train_steps(buf, 1, 16, return_losses=False)  # step 0, stages step 1's batch
        if not how.startswith("control"):
            gen = buf.view().generation
            add(buf, other, 1)
            assert buf.view().generation != gen
        if how.endswith("continued"):
            tr.train_steps(buf, 1, 16, return_losses=False)
        else:
            tr.train_steps(buf, 1, 16, indices=idx1, return_losses=False)
        torch.cuda.synchronize()
        runs[how] = torch.cat([p.detach().reshape(-1).clone() for p in tr.actor.parameters()] +
                              [p.detach().reshape(-1).clone() for p in tr.qf.parameters()])
    assert torch.equal(runs["control_continued"], runs["control_injected"])
    assert not torch.equal(runs["continued"], runs["control_continued"])  # the new row mattered
    assert torch.equal(runs["continued"], runs["injected"])


# --------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------- #
def test_refusals_leave_everything_as_it_was():
    ft = _ft()
    lib = _lib.load()
    kw = dict(deterministic=False, n_hidden=2, hidden=64)
    good = _trainer(ft, S_, A_, seed=1, **kw)
    bf16 = _trainer(ft, S_, A_, seed=2, precision="bf16", **kw)
    wider = _trainer(ft, S_ + 1, A_, seed=3, **kw)
    for tr in (good, bf16, wider):
        tr._ensure_handle(16)

    def raw(trainers, states):
        out = torch.full((len(trainers), A_), -7.0, device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.iqlhip_explore_action_group((C.c_void_p * len(trainers))(*[t._handle.value for t in trainers]),
                                                 len(trainers), _lib.ptr(states), states.shape[1], None, 0.03, 0.5,
                                                 MAX_ACTION, (C.c_uint32 * len(trainers))(), _lib.ptr(out),
                                                 _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    # a bf16 member
    states = torch.zeros((2, S_), device=DEV)
    with pytest.raises(NotImplementedError):
        ft.explore_actions([good, bf16], states, expl_noise=0.03, noise_clip=0.5)
    rc, out = raw([good, bf16], states)
    assert rc == _lib.ERR_UNSUPPORTED and (out == -7.0).all()
    # members of different S
    with pytest.raises(ValueError):
        ft.explore_actions([good, wider], torch.zeros((2, S_ + 1), device=DEV), expl_noise=0.03, noise_clip=0.5)
    rc, out = raw([good, wider], torch.zeros((2, S_ + 1), device=DEV))
    assert rc == _lib.ERR_INVALID and (out == -7.0).all()
    assert good._explore_calls == bf16._explore_calls == wider._explore_calls == 0

    # a full ring beside one with room: neither is written
    room, full = ft.ReplayBuffer(S_, A_, 8, DEV), ft.ReplayBuffer(S_, A_, 4, DEV)
    room.load_d4rl_dataset(_transitions(3, 6, S_, A_))
    full.load_d4rl_dataset(_transitions(4, 7, S_, A_))  # (a dataset that filled the buffer: fref:173)
    before = [b._rows.clone() for b in (room, full)]
    gens = [b.view().generation for b in (room, full)]
    new = _transitions(2, 9, S_, A_)
    with pytest.raises(IndexError):
        ft.add_transitions([room, full], new["observations"], new["actions"], new["rewards"],
                           new["next_observations"], new["terminals"])
    stage = torch.ones((2, 2 * S_ + A_ + 2), device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.iqlhip_replay_append_group((C.c_void_p * 2)(room._rows.data_ptr(), full._rows.data_ptr()), room._stride,
                                            S_, A_, (C.c_int64 * 2)(8, 4), (C.c_int64 * 2)(3, 4), 2, _lib.ptr(stage),
                                            _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID
    for b, rows, gen, at in zip((room, full), before, gens, ((3, 3), (4, 4))):
        assert torch.equal(b._rows, rows) and (b._pointer, b._size) == at and b.view().generation == gen


# --------------------------------------------------------------------------- #
# train(seeds_per_gpu=3) against three runs of train()
# --------------------------------------------------------------------------- #
def _same(a, b, path="state_dict"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}/{i}")
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    else:
        assert a == b or (a != a and b != b), path


def _run(ft, name, det, seed, K, tmp_path, monkeypatch):
    """One finetune.train call; returns per member what the comparison needs."""
    config = ft.TrainConfig(device=DEV, env=name, seed=seed, eval_seed=3, eval_freq=25, n_episodes=2,
                            offline_iterations=40, online_iterations=60, checkpoints_path=str(tmp_path / f"K{K}_{seed}"),
                            buffer_size=320, batch_size=32, iql_deterministic=det)
    envs = [fe.RecordingEnv(fe.FinetuneEnv(name)) for _ in range(K)]
    eval_envs = [fe.RecordingEnv(fe.FinetuneEnv(name)) for _ in range(K)]
    dataset = fe.make_dataset(name, 300, 17)
    records, box = [], {}
    real_draw = ft.GrowingIndexStream.draw

    def draw(self, hi0, cap, n_steps, batch_size, growth=1, generators=None):
        box["gens"] = generators
        return real_draw(self, hi0, cap, n_steps, batch_size, growth, generators)

    monkeypatch.setattr(ft.GrowingIndexStream, "draw", draw)
    logger = lambda d, step: records.append((int(step), dict(d)))
    on_start = lambda tr, buf: box.update(buf=buf)
    if K == 1:
        trainers = [ft.train(config, envs[0], eval_envs[0], dataset, device=DEV, logger=logger, online_chunk=7,
                             on_start=on_start)]
        bufs, gen_states = [box["buf"]], [np.random.get_state()]
        ckpts = [config.checkpoints_path]
        assert box["gens"] is None
    else:
        trainers = ft.train(config, envs, lambda k: eval_envs[k], dataset, device=DEV, logger=logger, online_chunk=7,
                            on_start=on_start, seeds_per_gpu=K)
        bufs, gen_states = box["buf"], [g.get_state() for g in box["gens"]]
        ckpts = [os.path.join(config.checkpoints_path, f"seed_{seed + k}") for k in range(K)]
    torch.cuda.synchronize()
    out = []
    for k in range(K):
        recs = records if K == 1 else [(s, {n: v for n, v in d.items() if n != "seed"}) for s, d in records
                                       if d["seed"] == seed + k]
        out.append({"sd": trainers[k].state_dict(), "rows": bufs[k]._rows.clone(),
                    "ring": (bufs[k]._pointer, bufs[k]._size), "tape": envs[k].tape("env"),
                    "eval_tape": eval_envs[k].tape("eval"), "records": recs, "gen": gen_states[k],
                    "ckpts": sorted(os.listdir(ckpts[k]))})
    if K > 1:
        assert all("seed" in d for _, d in records)
    return out


@pytest.mark.parametrize("name,det", [("antmaze-finetune-v0", False), ("cheetah-finetune-v0", True)],
                         ids=["gaussian_goal", "deterministic"])
def test_train_three_seeds_equals_three_runs(name, det, tmp_path, monkeypatch):
    ft = _ft()
    K, seed = 3, 40
    group = _run(ft, name, det, seed, K, tmp_path, monkeypatch)
    for k in range(K):
        solo = _run(ft, name, det, seed + k, 1, tmp_path, monkeypatch)[0]
        m = group[k]
        who = f"member {k} (seed {seed + k})"
        for key in solo["tape"]:  # what the environment handed out and the actions it was given
            np.testing.assert_array_equal(m["tape"][key], solo["tape"][key], err_msg=f"{who}: {key}")
        for key in solo["eval_tape"]:
            np.testing.assert_array_equal(m["eval_tape"][key], solo["eval_tape"][key], err_msg=f"{who}: {key}")
        assert m["sd"]["explore_calls"] == solo["sd"]["explore_calls"] == 60, who
        _same(m["sd"], solo["sd"], who)
        assert m["ring"] == solo["ring"] == (40, 320), who  # 300 + 60 rows through a ring of 320
        assert torch.equal(m["rows"], solo["rows"]), who
        assert len(m["records"]) == len(solo["records"]), who
        for i, ((s0, d0), (s1, d1)) in enumerate(zip(m["records"], solo["records"])):
            assert s0 == s1 and list(d0) == list(d1), f"{who}: record {i}"
            for n in d0:
                assert np.array_equal(d0[n], d1[n], equal_nan=True), f"{who}: record {i} at step {s0}, {n}"
        assert m["gen"][0] == solo["gen"][0] and m["gen"][2:] == solo["gen"][2:], who
        np.testing.assert_array_equal(m["gen"][1], solo["gen"][1], err_msg=who)
        want = sorted(f"checkpoint_{t}.pt" for t in (24, 49, 74, 99))
        assert m["ckpts"] == want and [f for f in solo["ckpts"] if f.endswith(".pt")] == want, who
    # the members are runs of their own: they differ from one another
    assert not torch.equal(group[0]["rows"], group[1]["rows"])


# --------------------------------------------------------------------------- #
# one loop: what one seed and what a group call in it, and what the caller of one seed is handed
# --------------------------------------------------------------------------- #
def _small_run(ft, name, K, tmp_path, **hooks):
    """A run of one offline chunk (4 steps), three online index chunks of 5 / 5 / 2 ticks, evaluations after
    steps 7 and 15, and a ring that wraps (40 + 12 > 48).  Returns (config, envs, what train returned, records)."""
    config = ft.TrainConfig(device=DEV, env=name, seed=40, eval_seed=3, eval_freq=8, n_episodes=1, offline_iterations=4,
                            online_iterations=12, checkpoints_path=str(tmp_path / f"K{K}"), buffer_size=48, batch_size=32)
    envs = [fe.RecordingEnv(fe.FinetuneEnv(name)) for _ in range(K)]
    eval_envs = [fe.RecordingEnv(fe.FinetuneEnv(name)) for _ in range(K)]
    records = []
    solo = K == 1
    got = ft.train(config, envs[0] if solo else envs, eval_envs[0] if solo else eval_envs, fe.make_dataset(name, 40, 17),
                   device=DEV, logger=lambda d, step: records.append((int(step), dict(d))), online_chunk=5,
                   seeds_per_gpu=K, **hooks)
    torch.cuda.synchronize()
    return config, envs, got, records


@pytest.mark.parametrize("name", ["antmaze-finetune-v0", "cheetah-finetune-v0"], ids=["goal", "plain"])
def test_one_seed_takes_the_solo_calls_and_a_group_the_grouped_ones(name, tmp_path, monkeypatch):
    ft = _ft()
    from iqlpref_amd import multi
    calls = {}

    def spy(owner, attr, key):
        real = getattr(owner, attr)
        calls[key] = 0

        def counted(*args, **kw):
            calls[key] += 1
            return real(*args, **kw)
        monkeypatch.setattr(owner, attr, counted)

    spy(ft, "explore_actions", "explore_actions")
    spy(ft, "add_transitions", "add_transitions")
    spy(ft.ImplicitQLearning, "explore_action", "explore_action")
    spy(ft.ReplayBuffer, "add_transition", "add_transition")
    spy(ft.ImplicitQLearning, "train_steps", "train_steps")
    spy(multi.SeedGroup, "__init__", "SeedGroup")
    spy(multi.SeedGroup, "train_steps", "SeedGroup.train_steps")

    _small_run(ft, name, 1, tmp_path)
    solo = dict(calls)
    assert solo["explore_action"] == 12 and solo["add_transition"] == 12
    assert solo["train_steps"] == 1 + 12  # one offline chunk, one call per tick
    assert solo["explore_actions"] == 0 and solo["add_transitions"] == 0
    assert solo["SeedGroup"] == 0 and solo["SeedGroup.train_steps"] == 0

    for key in calls:
        calls[key] = 0
    _small_run(ft, name, 3, tmp_path)
    assert calls["explore_action"] == 0 and calls["add_transition"] == 0
    assert calls["explore_actions"] == 12 and calls["add_transitions"] == 12
    assert calls["SeedGroup"] == 1 and calls["SeedGroup.train_steps"] == 1 + 12


@pytest.mark.parametrize("name", ["antmaze-finetune-v0", "cheetah-finetune-v0"], ids=["goal", "plain"])
def test_one_seed_keeps_its_call_shapes(name, tmp_path, monkeypatch):
    ft = _ft()
    real_rank_seed = ft.D.rank_seed
    monkeypatch.setattr(ft.D, "rank_seed", lambda seed, *a, **kw: real_rank_seed(seed, *a, **kw) + 1000)
    want = ["checkpoint_15.pt", "checkpoint_7.pt"]
    box = {}
    config, envs, got, records = _small_run(ft, name, 1, tmp_path, on_start=lambda tr, buf: box.update(tr=tr, buf=buf))
    assert envs[0].seeds[0] == config.seed  # no rank_seed for one seed
    assert isinstance(box["tr"], ft.ImplicitQLearning) and isinstance(box["buf"], ft.ReplayBuffer)
    assert got is box["tr"]
    assert records and not any("seed" in d for _, d in records)
    assert sorted(f for f in os.listdir(config.checkpoints_path) if f.endswith(".pt")) == want

    config, envs, got, records = _small_run(ft, name, 2, tmp_path, on_start=lambda tr, buf: box.update(tr=tr, buf=buf))
    assert isinstance(got, list) and got == box["tr"] and len(box["buf"]) == 2
    for k in range(2):
        s = config.seed + 1000 + k
        assert envs[k].seeds[0] == s
        assert sorted(os.listdir(os.path.join(config.checkpoints_path, f"seed_{s}"))) == want
    assert {d["seed"] for _, d in records} == {config.seed + 1000, config.seed + 1001}
    assert not [f for f in os.listdir(config.checkpoints_path) if f.endswith(".pt")]
