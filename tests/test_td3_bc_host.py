"""tdbc (algorithms/offline/td3_bc.py) without a GPU: the torch restatement of tests/td3_bc_cases.py against
tests/golden/td3_bc_step.npz (the reference's own ``train``) in fp32 -- torch on both sides, one thread -- and at the
float64 gap; what the step cases must have (kink shares, clipped noise, a' at and inside +-max_action, mean|q|); the
mirrored surface; the envelope refusals of the layout call; ``train()``'s bookkeeping on a stub stepper, the
recorder's row-to-record rule included; and the choices make_td3_bc_fixture.py committed."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib, _offline_loop, td3_bc
from tests import helpers, minari_cases as mc, offline_bc_env as obe, td3_bc_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step(golden_dir):
    return mc.load(golden_dir, "td3_bc_step.npz")


@pytest.fixture(scope="module")
def run(golden_dir):
    return mc.load(golden_dir, "td3_bc_run.npz")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _restated(case, dtype):
    """The case's chained steps of the restatement in ``dtype``: per step (losses, grads, p, m, v)."""
    S, A, B, H, params, data, idx, eps, _ = tc.case_inputs(case)
    hp = tc.hyper(case)
    np_t = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    p = {n: {k: v.astype(np_t) for k, v in params[n].items()} for n in params}
    m = {n: {k: np.zeros_like(v) for k, v in p[n].items()} for n in tc.TRAINED}
    v = {n: {k: np.zeros_like(x) for k, x in p[n].items()} for n in tc.TRAINED}
    out, actor_it = [], 0

    def adam(n, grads, t1):
        for k in p[n]:
            p[n][k], m[n][k], v[n][k] = tc.adam_step(p[n][k], m[n][k], v[n][k], grads[f"{n}.{k}"], t1, dtype, lr=tc.LR)

    for t in range(tc.n_steps(case)):
        batch = tc.batch_of(data, idx[t, :B])
        lc, gc, _, _ = tc.critic_half(p["actor_target"], p["critic_1"], p["critic_2"], p["critic_1_target"],
                                      p["critic_2_target"], batch, eps[t], hp, dtype)
        adam("critic_1", gc, t + 1), adam("critic_2", gc, t + 1)
        losses, grads = {"critic_loss": lc}, dict(gc)
        if tc.is_actor_step(t + 1, hp["policy_freq"]):
            la, ga, _, _ = tc.actor_half(p["actor"], p["critic_1"], batch, hp, dtype)
            actor_it += 1
            adam("actor", ga, actor_it)
            losses["actor_loss"] = la
            grads.update(ga)
            for n, tg in zip(tc.TRAINED, tc.TARGETS):
                if dtype is torch.float32:
                    p[tg] = {k: tc.polyak32(p[tg][k], p[n][k], tc.TAU) for k in p[tg]}
                else:
                    p[tg] = {k: (1 - tc.TAU) * p[tg][k] + tc.TAU * p[n][k] for k in p[tg]}
        flat = lambda d: {f"{n}.{k}": x.copy() for n in d for k, x in d[n].items()}
        out.append((losses, grads, flat(p), flat(m), flat(v)))
    return out


def test_restatement_is_the_references_train(step):
    """The reference's own losses and gradients lie within ``judge_gap`` of the float64 restatement (4 x the
    restatement's fp32 / float64 gap, floored at the rounding unit).  Torch on both sides and one thread: the fp32
    restatement gives the reference's bits, asserted on every loss and on every tensor stored whole; the float64 sum
    of every tensor, stored for all steps, is met within 1e-12 relative.  The log dict has ``actor_loss`` on actor
    steps only, and each optimiser counts its own steps."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for case in step["cases"]:
            case = str(case)
            r32, r64 = _restated(case, torch.float32), _restated(case, torch.float64)
            for t in range(tc.n_steps(case)):
                pre = f"{case}/{t}"
                losses, grads, p, m, v = r32[t]
                assert [str(k) for k in step[f"{pre}/keys"]] == list(losses), pre
                for k in losses:
                    gap = abs(losses[k] - r64[t][0][k])
                    ratio, _ = tc.judge_gap(step[f"{pre}/{k}"], r64[t][0][k], gap)
                    assert ratio <= 1, (pre, k, ratio)
                    assert np.float32(losses[k]) == np.float32(step[f"{pre}/{k}"]), (pre, k)
                for what, ours, ours64 in (("grad", grads, r64[t][1]), ("param", p, r64[t][2]), ("exp_avg", m, r64[t][3]),
                                           ("exp_avg_sq", v, r64[t][4])):
                    for name, x in ours.items():
                        key = f"{pre}/{what}/{name}"
                        if key + "/sum" not in step:  # (no state yet, or a gradient tdbc never applies)
                            continue
                        np.testing.assert_allclose(x.astype(np.float64).sum(), step[key + "/sum"], rtol=1e-12, atol=1e-300, err_msg=key)
                        if key in step:
                            assert np.array_equal(bits(x), bits(step[key])), key
                            ratio, _ = tc.judge(step[key], ours64[name], x)
                            assert ratio <= 1, (key, ratio)
                # the actor's optimiser counts its own steps (tdbc:373)
                acts = (t + 1) // tc.CASES[case][5]
                if acts:
                    assert float(step[f"{pre}/step/actor.net.0.weight"]) == acts
                assert float(step[f"{pre}/step/critic_1.net.0.weight"]) == t + 1
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("case", list(tc.CASES))
def test_cases_keep_their_conditions(case):
    """From the float64 restatement alone, so that the GPU test cannot pass by luck: in every step at most KINK_CAP
    of the (row, unit) pairs of the differentiated networks within KINK of zero; except in the one-row case between
    5 % and 95 % of the noise entries clipped at noise_clip; at least one a' at +-max_action and at least one inside;
    mean|q| at least 1e-3 in every actor step; two actor steps."""
    hp, B = tc.hyper(case), tc.CASES[case][2]
    traj = tc.f64_trajectory(case)
    assert len(traj) == tc.n_steps(case) >= 3
    assert sum(o["actor_loss"] is not None for o in traj) >= 2
    raw = np.stack([o["critic"]["raw"] for o in traj])
    noise = np.stack([o["critic"]["noise"] for o in traj])
    a2 = np.stack([o["critic"]["next_action"] for o in traj])
    clipped = np.abs(raw) > hp["noise_clip"]
    assert np.array_equal(np.abs(noise[clipped]), np.full(int(clipped.sum()), hp["noise_clip"]))
    if B > 1:
        assert 0.05 <= clipped.mean() <= 0.95, (case, clipped.mean())
    at_edge = np.abs(a2) == hp["max_action"]
    assert at_edge.any() and not at_edge.all(), case
    assert np.all(np.abs(a2) <= hp["max_action"])
    for t, o in enumerate(traj):
        assert o["share"] <= tc.KINK_CAP, (case, t, o["share"])
        assert np.isfinite(o["critic_loss"])
        assert (o["actor"] is not None) == tc.is_actor_step(t + 1, hp["policy_freq"])
        if o["actor"] is not None:
            assert o["actor"]["mean_abs_q"] >= 1e-3 and np.isfinite(o["actor_loss"]), (case, t)


def test_permuted_orders_are_the_same_restatement():
    case = "s17_a6_b17_h256"
    S, A, B, H, params, data, idx, eps, _ = tc.case_inputs(case)
    hp = tc.hyper(case)
    batch = tc.batch_of(data, idx[0, :B])
    nets = tuple(params[n] for n in ("actor_target", "critic_1", "critic_2", "critic_1_target", "critic_2_target"))
    rest = (batch, eps[0], hp)
    l64, g64, _, _ = tc.critic_half(*nets, *rest, torch.float64)
    rng = np.random.default_rng(3)
    perms = [[rng.permutation(H) for _ in range(2)] for _ in nets]
    l2, g2 = tc.critic_half(*[tc.permute_hidden(n, pm) for n, pm in zip(nets, perms)], *rest, torch.float64)[:2]
    assert abs(l2 - l64) <= 1e-13 * abs(l64)
    for prefix, i in (("critic_1", 1), ("critic_2", 2)):
        own = tc.unpermute_grads({k[len(prefix) + 1:]: v for k, v in g2.items() if k.startswith(prefix + ".")}, perms[i])
        for k, v in own.items():
            assert np.max(np.abs(v - g64[f"{prefix}.{k}"])) <= 1e-13 * max(1.0, np.abs(v).max()), (prefix, k)
    trained = {"critic_1": 1, "critic_2": 2}
    l1, g1 = tc.fp32_gap(tc.critic_half, nets, rest, trained, l64, g64, orders=1)
    l8, g8 = tc.fp32_gap(tc.critic_half, nets, rest, trained, l64, g64)
    l32, g32, _, _ = tc.critic_half(*nets, *rest, torch.float32)
    assert l1 == abs(l32 - l64) and l8 >= l1
    for k in g64:
        assert np.array_equal(g1[k], np.abs(g32[k].astype(np.float64) - g64[k])) and np.all(g8[k] >= g1[k]), k
    anets = (params["actor"], params["critic_1"])
    la64, ga64, _, _ = tc.actor_half(*anets, batch, hp, torch.float64)
    la2, ga2 = tc.actor_half(*[tc.permute_hidden(n, pm) for n, pm in zip(anets, perms)], batch, hp, torch.float64)[:2]
    own = tc.unpermute_grads({k[6:]: v for k, v in ga2.items()}, perms[0])
    assert abs(la2 - la64) <= 1e-13 * abs(la64)
    assert all(np.max(np.abs(v - ga64["actor." + k])) <= 1e-12 * max(1.0, np.abs(v).max()) for k, v in own.items())


def test_cases_are_what_the_issue_lists():
    assert sorted(v[:6] for v in tc.CASES.values()) == sorted([(3, 1, 1, 16, 1.0, 2), (17, 6, 17, 256, 1.0, 2),
                                                               (128, 32, 48, 128, 2.0, 2), (45, 24, 64, 64, 1.0, 3),
                                                               (29, 8, 256, 256, 1.0, 1)])
    for case in tc.CASES:
        S, A, B, H, params, data, idx, eps, poison = tc.case_inputs(case)
        named = set(idx[:, :B].reshape(-1).tolist())
        assert all(np.all(data[k][sorted(set(range(len(data["rewards"]))) - named)] == tc.POISON)
                   for k in ("observations", "actions", "next_observations", "rewards"))
        assert not np.any(data["observations"][sorted(named)] == tc.POISON)
        assert set(idx[:, B:].reshape(-1).tolist()) <= set(poison.tolist())
        assert eps.shape == (tc.n_steps(case), B, A) and eps.dtype == np.float32
        assert data["terminals"][sorted(named)].max() == 1.0 or B == 1


def test_config_fields_and_defaults(tmp_path):
    want = [("project", "CORL"), ("group", "TD3_BC-D4RL"), ("name", None), ("env", "halfcheetah-medium-expert-v2"),
            ("alpha", 2.5), ("discount", 0.99), ("expl_noise", 0.1), ("tau", 0.005), ("policy_noise", 0.2),
            ("noise_clip", 0.5), ("policy_freq", 2), ("max_timesteps", 1_000_000), ("buffer_size", 2_000_000),
            ("batch_size", 256), ("normalize", True), ("normalize_reward", False), ("eval_freq", 5000), ("n_episodes", 10),
            ("checkpoints_path", None), ("load_model", ""), ("seed", 0), ("device", "cuda")]
    c = td3_bc.TrainConfig()
    assert [f.name for f in dataclasses.fields(c)] == [k for k, _ in want]
    assert all(getattr(c, k) == v for k, v in want if k != "name")
    assert c.name.startswith("TD3_BC-halfcheetah-medium-expert-v2-") and len(c.name.split("-")[-1]) == 8
    path = tmp_path / "c.yaml"
    path.write_text("env: hopper-medium-v2\nalpha: 1e-1\nnormalize: false\npolicy_freq: 3\n")
    c = td3_bc.load_config(str(path), tau="0.01", checkpoints_path=str(tmp_path))
    assert (c.env, c.alpha, c.normalize, c.policy_freq, c.tau) == ("hopper-medium-v2", 0.1, False, 3, 0.01)
    assert c.checkpoints_path == os.path.join(str(tmp_path), c.name)
    with pytest.raises(ValueError, match="unknown"):
        td3_bc.load_config(None, awac_lambda="1")


def test_modules_have_the_references_names(run):
    actor, critic = td3_bc.Actor(17, 6, 1.0), td3_bc.Critic(17, 6)
    whole = str(run["run/whole"])
    assert list(actor.state_dict()) == [str(k) for k in run[f"run/{whole}/actor/names"]] == list(tc.NAMES)
    assert list(critic.state_dict()) == [str(k) for k in run[f"run/{whole}/critic_1/names"]]
    assert [str(k) for k in run[f"run/{whole}/keys"]] == ["critic_1", "critic_1_optimizer", "critic_2", "critic_2_optimizer",
                                                          "actor", "actor_optimizer", "total_it"]
    assert tuple(actor.net[0].weight.shape) == (256, 17) and tuple(critic.net[4].weight.shape) == (1, 256)
    small = td3_bc.Actor(17, 6, 2.0, 32)
    assert td3_bc._net_dims(small, (td3_bc.Critic(17, 6, 32), td3_bc.Critic(17, 6, 32))) == (17, 6, 32)
    with pytest.raises(NotImplementedError):
        td3_bc._net_dims(small, (td3_bc.Critic(17, 6, 32), td3_bc.Critic(17, 6, 48)))
    with pytest.raises(TypeError):
        td3_bc._net_dims(torch.nn.Linear(3, 3), (critic, critic))
    # soft_update is tdbc:77-79
    a, b = td3_bc.Critic(3, 1, 16), td3_bc.Critic(3, 1, 16)
    want = [tc.polyak32(x.detach().numpy(), y.detach().numpy(), tc.TAU) for x, y in zip(a.parameters(), b.parameters())]
    td3_bc.soft_update(a, b, tc.TAU)
    assert all(np.array_equal(bits(x.detach().numpy()), bits(w)) for x, w in zip(a.parameters(), want))
    assert td3_bc._actor_steps(0, 5, 2) == 2 and td3_bc._actor_steps(1, 5, 2) == 3 and td3_bc._actor_steps(4, 1, 3) == 0


def test_new_entry_points_are_bound_as_declared():
    with open(os.path.join(ROOT, "include", "iqlhip.h")) as f:
        header = helpers.parse_c_header(f.read())
    new = {f"iqlhip_td3bc_{n}" for n in ("arena_layout", "create", "destroy", "sync_weights", "set_step", "set_lr",
                                          "train_steps", "copy_out", "group_create", "group_destroy", "group_train_steps")}
    assert new <= set(header["functions"]) and new <= set(_lib.SYMBOLS)
    for n in new:
        assert len(_lib.SYMBOLS[n][1]) == len(header["functions"][n][1]), n
    assert _lib.ABI_VERSION == 6  # entry points were added, nothing changed


def test_envelope_is_refused_by_the_layout_call():
    """The layout call touches no device: precision, depth, width and dims are refused there, before anything is
    uploaded, and ``train()`` asks it first."""
    import ctypes as C
    lib = _lib.load()
    offs, n = (C.c_int64 * 18)(), C.c_int64()
    call = lambda cfg: lib.iqlhip_td3bc_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n))
    for H in range(16, 257, 16):
        assert call(td3_bc._config(17, 6, H, 256)) == 0
    assert call(td3_bc._config(128, 32, 256, 1)) == 0 and call(td3_bc._config(1, 1, 16, 65536)) == 0

    def create(cfg, policy_freq=2):
        h = C.c_void_p()
        ar = _lib.Arenas(1, 1, 1, 1, None)  # (never dereferenced: the config is refused first)
        return lib.iqlhip_td3bc_create(C.byref(h), C.byref(cfg), 5e-3, 0.2, 0.5, 1.0, 2.5, policy_freq, C.byref(ar))

    for field, value in (("precision", _lib.PREC_BF16), ("hidden_dim", 8), ("hidden_dim", 24), ("hidden_dim", 272),
                         ("n_hidden", 3), ("n_hidden", 0), ("n_hidden", 1), ("dropout_p", 0.1), ("state_dim", 129),
                         ("action_dim", 33), ("batch_size", 65537)):
        cfg = td3_bc._config(17, 6, 64, 64)
        setattr(cfg, field, value)
        assert call(cfg) == _lib.ERR_UNSUPPORTED, field
        assert create(cfg) == _lib.ERR_UNSUPPORTED, field
    assert create(td3_bc._config(17, 6, 64, 64), policy_freq=0) == _lib.ERR_UNSUPPORTED
    assert call(td3_bc._config(17, 6, 64, 0)) == _lib.ERR_INVALID
    # the layout: 18 tensors in order, each on a 128-byte line
    assert call(td3_bc._config(17, 6, 32, 64)) == 0
    o = list(offs)
    sizes = [32 * 17, 32, 32 * 32, 32, 6 * 32, 6] + 2 * [32 * 23, 32, 32 * 32, 32, 32, 1]
    assert o[0] == 0 and all(x % 32 == 0 for x in o)
    assert all(b == a + -(-s // 32) * 32 for a, b, s in zip(o, o[1:] + [n.value], sizes))
    with pytest.raises(NotImplementedError):
        td3_bc.check_envelope(17, 6, 40)
    with pytest.raises(NotImplementedError):
        td3_bc.check_envelope(17, 6, 64, policy_freq=0)
    with pytest.raises(NotImplementedError):
        td3_bc.train(td3_bc.TrainConfig(batch_size=4), obe.make_dataset(11), obe.OfflineBCEnv(), device="cpu", hidden_dim=40)


# --------------------------------------------------------------------------- #
# train(): bookkeeping on a stub stepper (no device)
# --------------------------------------------------------------------------- #
class _Buffer:
    made = []

    def __init__(self, state_dim, action_dim, buffer_size, device):
        self.n = None
        _Buffer.made.append(self)

    def load_d4rl_dataset(self, data):
        self.n, self.data = data["observations"].shape[0], {k: np.array(v) for k, v in data.items()}

    def index_bound(self):
        return self.n

    def draw_indices(self, batch_size, n_batches=None, rng=None):
        gen = np.random if rng is None else rng
        return np.stack([gen.randint(0, self.n, size=batch_size) for _ in range(n_batches)])


class _Actor:
    mode = "train"

    def eval(self):
        self.mode = "eval"

    def train(self):
        self.mode = "train"

    def act(self, state, device):
        assert self.mode == "eval"
        return np.zeros(6)


class _Trainer:
    def __init__(self, total_it=0):
        self.actor, self.total_it, self._dev = _Actor(), total_it, "cpu"

    def state_dict(self):
        return {"total_it": self.total_it}

    def load_state_dict(self, sd):
        self.total_it = sd["total_it"]


class _Stepper:
    seen = []

    def __init__(self, trainers):
        self.trainers = trainers

    def train_steps(self, buf, n, B, *, indices, eps=None, return_losses=False):
        out = []
        for k, (tr, idx) in enumerate(zip(self.trainers, indices)):
            assert tuple(idx.shape) == (n, B)
            _Stepper.seen.append(None if eps is None else eps[k].clone())
            base = torch.arange(tr.total_it, tr.total_it + n, dtype=torch.float32)
            out.append(torch.stack([base, torch.zeros(n)], 1))  # an actor_loss of 0.0 on EVERY step: no sentinel decides
            tr.total_it += n
        return out

    def synchronize(self):
        pass

    def close(self):
        pass


def _stub_train(monkeypatch, tmp_path, noise="device", seeds_per_gpu=1, **config_kw):
    _Buffer.made.clear(), _Stepper.seen.clear()
    monkeypatch.setattr(td3_bc, "ReplayBuffer", _Buffer)
    monkeypatch.setattr(td3_bc, "_build_trainer", lambda *a, **k: _Trainer())
    monkeypatch.setattr(td3_bc, "stepper", lambda trainers: _Stepper(trainers))
    kw = dict(env=obe.ENV, max_timesteps=7, eval_freq=3, batch_size=4, n_episodes=2, seed=6, checkpoints_path=str(tmp_path))
    kw.update(config_kw)
    config = td3_bc.TrainConfig(**kw)
    records = []
    dataset = obe.make_dataset(11)
    out = td3_bc.train(config, dataset, obe.OfflineBCEnv(), logger=lambda d, step: records.append((step, dict(d))),
                       sampler="host", noise=noise, device="cpu", chunk=2, seeds_per_gpu=seeds_per_gpu, hidden_dim=32)
    return config, records, out, dataset


def test_train_bookkeeping_on_a_stub_stepper(monkeypatch, tmp_path):
    config, records, trainer, dataset = _stub_train(monkeypatch, tmp_path)
    # records at the ONE-based total_it (tdbc:499); actor_loss where total_it % 2 == 0 only -- the stub's column is 0.0
    # on every step, so the rule is the step count's --; the score right behind the step that ends a period
    keys = [(s, list(d)) for s, d in records]
    c, ca = ["critic_loss"], ["critic_loss", "actor_loss"]
    assert keys == [(1, c), (2, ca), (3, c), (3, ["d4rl_normalized_score"]), (4, ca), (5, c), (6, ca),
                    (6, ["d4rl_normalized_score"]), (7, c)]
    assert [d["critic_loss"] for s, d in records if "critic_loss" in d] == [float(i) for i in range(7)]
    # checkpoint names are zero-based (tdbc:523)
    assert sorted(os.listdir(config.checkpoints_path)) == ["checkpoint_2.pt", "checkpoint_5.pt", "config.yaml"]
    assert torch.load(os.path.join(config.checkpoints_path, "checkpoint_5.pt"))["total_it"] == 6
    assert trainer.total_it == 7 and trainer.actor.mode == "train"
    # the score is tdbc:510-511's: get_normalized_score of the MEAN return, x 100, evaluated on config.seed
    env = td3_bc.wrap_env(obe.OfflineBCEnv(), 0.0, 1.0)
    scores = td3_bc.eval_actor(env, _Actor(), "cpu", 2, config.seed)
    want = env.get_normalized_score(scores.mean()) * 100.0
    assert [d["d4rl_normalized_score"] for s, d in records if "d4rl_normalized_score" in d] == [want, want]
    # the buffer got the z-scored dataset, rewards untouched, the dict rewritten in place
    raw = obe.make_dataset(11)
    mean, std = td3_bc.compute_mean_std(raw["observations"], eps=1e-3)
    np.testing.assert_array_equal(_Buffer.made[0].data["observations"], (raw["observations"] - mean) / std)
    np.testing.assert_array_equal(_Buffer.made[0].data["rewards"], raw["rewards"])
    assert np.array_equal(dataset["observations"], _Buffer.made[0].data["observations"])
    assert all(e is None for e in _Stepper.seen)  # noise="device": nothing injected


def test_normalize_off_and_policy_freq_3(monkeypatch, tmp_path):
    config, records, _, _ = _stub_train(monkeypatch, tmp_path, normalize=False, normalize_reward=True, policy_freq=3)
    raw = obe.make_dataset(11)
    np.testing.assert_array_equal(_Buffer.made[0].data["observations"], raw["observations"])
    td3_bc.modify_reward(raw, obe.ENV)
    np.testing.assert_array_equal(_Buffer.made[0].data["rewards"], raw["rewards"])
    assert [s for s, d in records if "actor_loss" in d] == [3, 6]
    assert [s for s, d in records if "critic_loss" in d] == list(range(1, 8))


def test_load_model_moves_the_step_offset(monkeypatch, tmp_path):
    """tdbc:487-490, 499: a loaded trainer goes on counting where the checkpoint stood, and the records follow."""
    ckpt = tmp_path / "start.pt"
    torch.save({"total_it": 11}, str(ckpt))
    config, records, trainer, _ = _stub_train(monkeypatch, tmp_path / "run", load_model=str(ckpt))
    assert trainer.total_it == 18
    assert [s for s, d in records if "critic_loss" in d] == list(range(12, 19))
    assert [s for s, d in records if "actor_loss" in d] == [12, 14, 16, 18]
    assert [s for s, d in records if "d4rl_normalized_score" in d] == [14, 17]
    assert sorted(os.listdir(config.checkpoints_path)) == ["checkpoint_2.pt", "checkpoint_5.pt", "config.yaml"]


def test_records_rule_under_the_loop_itself():
    """``_offline_loop.Records.loss_record``: the default is ``dict(zip(loss_names, row))``; TD3+BC's drops actor_loss
    by the step count."""
    base = _offline_loop.Records()
    assert base.loss_record(0, [1.0, 2.0, 3.0], 5) == {"value_loss": 1.0, "q_loss": 2.0, "actor_loss": 3.0}
    rec = td3_bc._Records(None, policy_freq=3, first_it=4)
    assert rec.step_offset == 5
    assert rec.loss_record(0, [1.0, 7.0], 0) == {"critic_loss": 1.0}            # total_it 5
    assert rec.loss_record(0, [1.0, 0.0], 1) == {"critic_loss": 1.0, "actor_loss": 0.0}  # total_it 6: by count, not by value


def test_group_records_carry_their_seed_and_no_other_key(monkeypatch, tmp_path):
    config, records, trainers, _ = _stub_train(monkeypatch, tmp_path, seeds_per_gpu=2)
    seeds = [config.seed, config.seed + 1]
    assert len(trainers) == 2 and sorted(os.listdir(config.checkpoints_path)) == ["config.yaml", "seed_6", "seed_7"]
    allowed = set(td3_bc.LOSS_NAMES) | {"d4rl_normalized_score", "seed"}
    assert all(set(d) <= allowed and d["seed"] in seeds for s, d in records)
    for seed in seeds:
        mine = [(s, [k for k in d if k != "seed"]) for s, d in records if d["seed"] == seed]
        assert [s for s, k in mine if "critic_loss" in k] == list(range(1, 8))
        assert [(s, k) for s, k in mine if k == ["d4rl_normalized_score"]] == [(3, ["d4rl_normalized_score"]), (6, ["d4rl_normalized_score"])]


def test_train_hands_recorded_noise_to_the_steps(monkeypatch, tmp_path):
    eps = np.random.default_rng(0).standard_normal((7, 4, 6)).astype(np.float32)
    _stub_train(monkeypatch, tmp_path, noise=eps)
    assert np.array_equal(torch.cat(_Stepper.seen).numpy(), eps)
    with pytest.raises(ValueError, match="shape"):
        _stub_train(monkeypatch, tmp_path / "c", noise=eps[:, :1])


def test_train_checks_its_arguments_first():
    with pytest.raises(ValueError, match="sampler"):
        td3_bc.train(td3_bc.TrainConfig(), {}, None, sampler="philox")
    with pytest.raises(ValueError, match="seeds_per_gpu"):
        td3_bc.train(td3_bc.TrainConfig(), {}, None, seeds_per_gpu=17)
    with pytest.raises(ValueError, match="noise"):
        td3_bc.train(td3_bc.TrainConfig(), obe.make_dataset(11), obe.OfflineBCEnv(), noise="host", device="cpu", hidden_dim=32)


def test_fixture_run_is_what_the_generator_would_choose_again(run):
    """The recorded seed is the first candidate that kept both margins, the candidates before it did not, and the
    stored fractions of the float64 twin stay under 1 for twice the recorded length."""
    steps, every = int(run["common/max_timesteps"]), int(run["common/eval_freq"])
    cand, ok = run["run/candidates"].tolist(), run["run/candidate_ok"].tolist()
    assert cand == list(range(int(run["common/first_seed"]), int(run["run/seed"]) + 1)) and ok == [False] * (len(ok) - 1) + [True]
    assert run["run/f64_critic_gap_of_bound"].shape == (2 * steps,) and run["run/f64_critic_gap_of_bound"].max() < 1
    assert run["run/f64_actor_gap_of_bound"].shape == (steps,) and run["run/f64_actor_gap_of_bound"].max() < 1
    assert run["run/f64_eval_gap_of_bound"].shape == (2 * steps // every,) and run["run/f64_eval_gap_of_bound"].max() < 1
    assert float(run["run/kink_margin"]) > 1 and float(run["common/kink_sigmas"]) == 4.0
    assert run["run/eps"].shape == (steps, int(run["common/batch_size"]), 6) and run["run/eps"].dtype == np.float32
    assert run["run/eval_returns"].shape == (steps // every, int(run["common/n_episodes"]))
    assert [str(n) for n in run["run/save_name"]] == [f"checkpoint_{t}.pt" for t in range(every - 1, steps, every)]
    # records at the one-based total_it: critic_loss 1..steps, actor_loss on the even ones
    step_of = lambda key: [int(s) for s, k in zip(run["run/rec_step"], run["run/rec_key"]) if str(k) == key]
    assert step_of("critic_loss") == list(range(1, steps + 1)) and step_of("actor_loss") == list(range(2, steps + 1, 2))
    assert step_of("d4rl_normalized_score") == list(range(every, steps + 1, every))
