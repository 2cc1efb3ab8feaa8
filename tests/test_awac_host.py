"""awac (algorithms/offline/awac.py) without a GPU: the torch restatement of tests/awac_cases.py against
tests/golden/awac_step.npz (the reference's own ``update``) bit for bit in fp32 -- torch on both sides, one thread --
and at the float64 gap; what the step cases must have (kink shares, weights at the cap and below it, no pre-clamp
action or critic tie within 1e-5 of its edge); ``modify_reward`` / ``return_reward_range`` against the reference's
values; the mirrored surface; the envelope refusals of the layout call; ``train()``'s bookkeeping on a stub stepper;
and the choices make_awac_fixture.py committed."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from iqlpref_amd import _lib, awac
from tests import awac_cases as ac, helpers, minari_cases as mc, offline_bc_env as obe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step(golden_dir):
    return mc.load(golden_dir, "awac_step.npz")


@pytest.fixture(scope="module")
def run(golden_dir):
    return mc.load(golden_dir, "awac_run.npz")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _restated(case, dtype):
    """STEPS chained updates of the restatement from the case's inputs in ``dtype``: per step (losses, grads, p, m, v)."""
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
    np_t = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    p = {n: {k: v.astype(np_t) for k, v in params[n].items()} for n in params}
    m = {n: {k: np.zeros_like(v) for k, v in p[n].items()} for n in ac.TRAINED}
    v = {n: {k: np.zeros_like(x) for k, x in p[n].items()} for n in ac.TRAINED}
    out = []
    for t in range(ac.STEPS):
        batch = ac.batch_of(data, idx[t, :B])
        lc, gc, _, _ = ac.critic_half(p["actor"], p["critic_1"], p["critic_2"], p["target_critic_1"], p["target_critic_2"],
                                      batch, eps[t, 0], dtype)
        for n in ac.TRAINED[1:]:
            for k in p[n]:
                p[n][k], m[n][k], v[n][k] = ac.adam_step(p[n][k], m[n][k], v[n][k], gc[f"{n}.{k}"], t + 1, dtype, lr=ac.LR)
        la, ga, _, _ = ac.actor_half(p["actor"], p["critic_1"], p["critic_2"], batch, eps[t, 1], lam, dtype)
        for k in p["actor"]:
            p["actor"][k], m["actor"][k], v["actor"][k] = ac.adam_step(p["actor"][k], m["actor"][k], v["actor"][k],
                                                                      ga[f"actor.{k}"], t + 1, dtype, lr=ac.LR)
        for c, tg in zip(ac.TRAINED[1:], ac.TARGETS):
            if dtype is torch.float32:
                p[tg] = {k: ac.polyak32(p[tg][k], p[c][k]) for k in p[tg]}
            else:
                p[tg] = {k: (1 - ac.TAU) * p[tg][k] + ac.TAU * p[c][k] for k in p[tg]}
        flat = lambda d: {f"{n}.{k}": x.copy() for n in d for k, x in d[n].items()}
        out.append(({"critic_loss": lc, "actor_loss": la}, {**gc, **ga}, flat(p), flat(m), flat(v)))
    return out


def test_restatement_is_the_references_update(step):
    """fp32: every stored tensor bit for bit (torch on both sides, one thread, the numpy target formula included);
    float64: within 4 x the fp32 / float64 gap of the restatement itself, floored at the fp32 rounding unit."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for case in step["cases"]:
            case = str(case)
            r32, r64 = _restated(case, torch.float32), _restated(case, torch.float64)
            for t in range(ac.STEPS):
                pre = f"{case}/{t}"
                losses, grads, p, m, v = r32[t]
                for k in ("critic_loss", "actor_loss"):
                    assert np.float32(losses[k]) == np.float32(step[f"{pre}/{k}"]), (pre, k)
                    ratio, _ = ac.judge(step[f"{pre}/{k}"], r64[t][0][k], np.float32(losses[k]))
                    assert ratio <= 1, (pre, k, ratio)
                for what, ours, ours64 in (("grad", grads, r64[t][1]), ("param", p, r64[t][2]), ("exp_avg", m, r64[t][3]),
                                           ("exp_avg_sq", v, r64[t][4])):
                    for name, x in ours.items():
                        key = f"{pre}/{what}/{name}"
                        np.testing.assert_allclose(x.astype(np.float64).sum(), step[key + "/sum"], rtol=1e-12, atol=1e-300, err_msg=key)
                        if key in step:
                            assert np.array_equal(bits(x), bits(step[key])), key
                            ratio, _ = ac.judge(step[key], ours64[name], x)
                            assert ratio <= 1, (key, ratio)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_cases_keep_their_margins(case):
    """From the float64 restatement alone: at most KINK_CAP of the (row, unit) pairs of the differentiated networks
    within KINK of zero in every step.  No pre-clamp action (a' or pi) within 1e-5 of +-1 and no |q1 - q2| below
    1e-5 at either action: both are continuous (clamp and min change value smoothly and are evaluated under no-grad),
    so nothing would have to be allowed for -- the cases simply have none.  The lambda case has weights at the cap of
    100 and below it in every step; the others have none at the cap."""
    for t, o in enumerate(ac.f64_trajectory(case)):
        assert o["share"] <= ac.KINK_CAP, (case, t, o["share"])
        pre = np.concatenate([o["critic"]["pre"].ravel(), o["actor"]["pre"].ravel()])
        assert not np.any(np.abs(np.abs(pre) - 1.0) < 1e-5), (case, t)
        assert not np.any(np.abs(o["actor"]["ties"]) < 1e-5), (case, t)
        w = o["actor"]["w"]
        at_cap = int((w >= ac.EXP_ADV_MAX).sum())
        if case == ac.LAMBDA_CASE:
            assert 0 < at_cap < w.size, (case, t, at_cap)
        else:
            assert at_cap == 0, (case, t, at_cap)
        assert np.isfinite(o["critic_loss"]) and np.isfinite(o["actor_loss"])


def test_permuted_orders_are_the_same_restatement():
    """``awac_cases.fp32_gap`` measures the fp32 side of a bound over several summation orders: the permuted networks
    must be the same function.  In float64 loss and gradients (put back in order) agree to rounding; in fp32 the gap
    over the orders is at least the gap of the restatement as it stands, which is order 0."""
    case = "s17_a6_b17_h256"
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
    batch = ac.batch_of(data, idx[0, :B])
    nets = tuple(params[n] for n in ("actor", "critic_1", "critic_2") + ac.TARGETS)
    rest = (batch, eps[0, 0])
    l64, g64, _, _ = ac.critic_half(*nets, *rest, torch.float64)
    rng = np.random.default_rng(3)
    perms = [[rng.permutation(H) for _ in range(3)] for _ in nets]
    l2, g2 = ac.critic_half(*[ac.permute_hidden(n, pm) for n, pm in zip(nets, perms)], *rest, torch.float64)[:2]
    assert abs(l2 - l64) <= 1e-13 * abs(l64)
    for prefix, i in (("critic_1", 1), ("critic_2", 2)):
        own = ac.unpermute_grads({k[len(prefix) + 1:]: v for k, v in g2.items() if k.startswith(prefix + ".")}, perms[i])
        for k, v in own.items():
            assert np.max(np.abs(v - g64[f"{prefix}.{k}"])) <= 1e-13 * max(1.0, np.abs(v).max()), (prefix, k)
    trained = {"critic_1": 1, "critic_2": 2}
    l1, g1 = ac.fp32_gap(ac.critic_half, nets, rest, trained, l64, g64, orders=1)
    l8, g8 = ac.fp32_gap(ac.critic_half, nets, rest, trained, l64, g64)
    l32, g32, _, _ = ac.critic_half(*nets, *rest, torch.float32)
    assert l1 == abs(l32 - l64) and l8 >= l1
    for k in g64:
        assert np.array_equal(g1[k], np.abs(g32[k].astype(np.float64) - g64[k])) and np.all(g8[k] >= g1[k]), k
    anets = nets[:3]
    la64, ga64, _, _ = ac.actor_half(*anets, batch, eps[0, 1], lam, torch.float64)
    la2, ga2 = ac.actor_half(*[ac.permute_hidden(n, pm) for n, pm in zip(anets, perms)], batch, eps[0, 1], lam, torch.float64)[:2]
    own = ac.unpermute_grads({k[6:]: v for k, v in ga2.items()}, perms[0])
    assert abs(la2 - la64) <= 1e-13 * abs(la64)
    assert all(np.max(np.abs(v - ga64["actor." + k])) <= 1e-12 * max(1.0, np.abs(v).max()) for k, v in own.items())


def test_cases_are_what_the_issue_lists():
    assert sorted(v[:4] for v in ac.CASES.values()) == sorted([(3, 1, 1, 16), (17, 6, 17, 256), (45, 24, 64, 64),
                                                               (96, 32, 48, 128), (29, 8, 256, 256)])
    assert sorted(v[4] for v in ac.CASES.values()) == [0.1, 1.0, 1.0, 1.0, 1.0]
    for case in ac.CASES:
        S, A, B, H, lam, params, data, idx, eps, poison = ac.case_inputs(case)
        named = set(idx[:, :B].reshape(-1).tolist())
        assert all(np.all(data[k][sorted(set(range(len(data["rewards"]))) - named)] == ac.POISON)
                   for k in ("observations", "actions", "next_observations", "rewards"))
        assert not np.any(data["observations"][sorted(named)] == ac.POISON)
        assert set(idx[:, B:].reshape(-1).tolist()) <= set(poison.tolist())
        assert eps.shape == (ac.STEPS, 2, B, A) and eps.dtype == np.float32


def test_modify_reward_is_awacs_not_iqls(step):
    for name in ("halfcheetah-medium-v2", "antmaze-medium-diverse-v2", "pen-human-v1"):
        d = obe.make_dataset(11)
        before = d["rewards"].copy()
        awac.modify_reward(d, name)
        assert np.array_equal(bits(d["rewards"]), bits(step[f"reward/{name}/rewards"])), name
        if "antmaze" in name:
            assert np.array_equal(d["rewards"], before - np.float32(1.0))
        if "pen" in name:
            assert np.array_equal(d["rewards"], before)
    d = obe.make_dataset(11)
    assert list(awac.return_reward_range(d, 1000)) == step["reward/halfcheetah-medium-v2/range"].tolist()
    assert list(awac.return_reward_range(d, 40)) == step["reward/halfcheetah-medium-v2/range40"].tolist()


def test_config_fields_and_defaults(tmp_path):
    want = [("project", "CORL"), ("group", "AWAC-D4RL"), ("name", None), ("env_name", "halfcheetah-medium-expert-v2"),
            ("hidden_dim", 256), ("learning_rate", 3e-4), ("gamma", 0.99), ("tau", 5e-3), ("awac_lambda", 1.0),
            ("num_train_ops", 1_000_000), ("batch_size", 256), ("buffer_size", 2_000_000), ("normalize_reward", False),
            ("eval_frequency", 1000), ("n_test_episodes", 10), ("checkpoints_path", None), ("deterministic_torch", False),
            ("seed", 42), ("test_seed", 69), ("device", "cuda")]
    c = awac.TrainConfig()
    assert [f.name for f in dataclasses.fields(c)] == [k for k, _ in want]
    assert all(getattr(c, k) == v for k, v in want if k != "name")
    assert c.name.startswith("AWAC-halfcheetah-medium-expert-v2-") and len(c.name.split("-")[-1]) == 8
    path = tmp_path / "c.yaml"
    path.write_text("env_name: hopper-medium-v2\nlearning_rate: 1e-3\nnormalize_reward: true\nhidden_dim: 64\n")
    c = awac.load_config(str(path), awac_lambda="0.3333", checkpoints_path=str(tmp_path))
    assert (c.env_name, c.learning_rate, c.normalize_reward, c.hidden_dim, c.awac_lambda) == ("hopper-medium-v2", 1e-3, True, 64, 0.3333)
    assert c.checkpoints_path == os.path.join(str(tmp_path), c.name)
    with pytest.raises(ValueError, match="unknown"):
        awac.load_config(None, load_model="x")  # awac has no load_model


def test_modules_have_the_references_names(run):
    actor, critic = awac.Actor(17, 6, 32), awac.Critic(17, 6, 32)
    whole = str(run["run/whole"])
    assert list(actor.state_dict()) == [str(k) for k in run[f"run/{whole}/actor/names"]]
    assert list(critic.state_dict()) == [str(k) for k in run[f"run/{whole}/critic_1/names"]]
    assert [str(k) for k in run[f"run/{whole}/keys"]] == ["actor", "critic_1", "critic_2"]
    assert tuple(actor._log_std.shape) == (6,) and float(actor._log_std.detach().abs().sum()) == 0.0
    assert (actor._min_log_std, actor._max_log_std, actor._min_action, actor._max_action) == (-20.0, 2.0, -1.0, 1.0)
    assert awac._net_dims(actor, (critic, awac.Critic(17, 6, 32))) == (17, 6, 32)
    with pytest.raises(NotImplementedError):
        awac._net_dims(actor, (critic, awac.Critic(17, 6, 48)))
    with pytest.raises(NotImplementedError):
        awac._net_dims(awac.Actor(17, 6, 32, max_log_std=1.0), (critic, critic))
    with pytest.raises(TypeError):
        awac._net_dims(torch.nn.Linear(3, 3), (critic, critic))
    # soft_update is awac:213-215
    a, b = awac.Critic(3, 1, 16), awac.Critic(3, 1, 16)
    want = [ac.polyak32(x.detach().numpy(), y.detach().numpy()) for x, y in zip(a.parameters(), b.parameters())]
    awac.soft_update(a, b, ac.TAU)
    assert all(np.array_equal(bits(x.detach().numpy()), bits(w)) for x, w in zip(a.parameters(), want))


def test_new_entry_points_are_bound_as_declared():
    with open(os.path.join(ROOT, "include", "iqlhip.h")) as f:
        header = helpers.parse_c_header(f.read())
    new = {f"iqlhip_awac_{n}" for n in ("arena_layout", "create", "destroy", "sync_weights", "set_step", "set_lr",
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
    offs, n, nt = (C.c_int64 * 25)(), C.c_int64(), C.c_int64()
    call = lambda cfg: lib.iqlhip_awac_arena_layout(C.byref(cfg), C.byref(offs), C.byref(n), C.byref(nt))
    for H in range(16, 257, 16):
        assert call(awac._config(17, 6, H, 256)) == 0
    assert call(awac._config(128, 32, 256, 1)) == 0
    for field, value in (("precision", _lib.PREC_BF16), ("hidden_dim", 8), ("hidden_dim", 24), ("hidden_dim", 272),
                         ("n_hidden", 2), ("n_hidden", 0), ("n_hidden", 4), ("dropout_p", 0.1), ("state_dim", 129),
                         ("action_dim", 33), ("batch_size", 65537)):
        cfg = awac._config(17, 6, 64, 64)
        setattr(cfg, field, value)
        assert call(cfg) == _lib.ERR_UNSUPPORTED, field
        h = C.c_void_p()
        ar = _lib.Arenas(1, 1, 1, 1, None)  # (never dereferenced: the config is refused first)
        assert lib.iqlhip_awac_create(C.byref(h), C.byref(cfg), 5e-3, 100.0, C.byref(ar)) == _lib.ERR_UNSUPPORTED, field
    assert call(awac._config(17, 6, 64, 0)) == _lib.ERR_INVALID
    # the layout: 25 tensors in order, each on a 128-byte line, the targets' part behind the actor's
    assert call(awac._config(17, 6, 32, 64)) == 0
    o = list(offs)
    sizes = [32 * 17, 32, 32 * 32, 32, 32 * 32, 32, 6 * 32, 6, 6] + 2 * [32 * 23, 32, 32 * 32, 32, 32 * 32, 32, 32, 1]
    assert o[0] == 0 and all(x % 32 == 0 for x in o)
    assert all(b == a + -(-s // 32) * 32 for a, b, s in zip(o, o[1:] + [n.value], sizes))
    assert nt.value == n.value - o[9]
    with pytest.raises(NotImplementedError):
        awac.check_envelope(17, 6, 40)
    with pytest.raises(NotImplementedError):
        awac.train(awac.TrainConfig(hidden_dim=40, batch_size=4), obe.make_dataset(11), obe.OfflineBCEnv(), device="cpu")


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
    def __init__(self):
        self._actor, self.total_it, self._dev = _Actor(), 0, "cpu"

    def state_dict(self):
        return {"total_it": self.total_it}


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
            out.append(torch.stack([base, -base], 1))
            tr.total_it += n
        return out

    def synchronize(self):
        pass

    def close(self):
        pass


def _stub_train(monkeypatch, tmp_path, noise="device", seeds_per_gpu=1, **config_kw):
    _Buffer.made.clear(), _Stepper.seen.clear()
    monkeypatch.setattr(awac, "ReplayBuffer", _Buffer)
    monkeypatch.setattr(awac, "_build_trainer", lambda *a, **k: _Trainer())
    monkeypatch.setattr(awac, "stepper", lambda trainers: _Stepper(trainers))
    config = awac.TrainConfig(env_name=obe.ENV, num_train_ops=7, eval_frequency=3, batch_size=4, n_test_episodes=2,
                              hidden_dim=32, seed=6, checkpoints_path=str(tmp_path), **config_kw)
    records = []
    dataset = obe.make_dataset(11)
    out = awac.train(config, dataset, obe.OfflineBCEnv(), logger=lambda d, step: records.append((step, dict(d))),
                     sampler="host", noise=noise, device="cpu", chunk=2, seeds_per_gpu=seeds_per_gpu)
    return config, records, out, dataset


def test_train_bookkeeping_on_a_stub_stepper(monkeypatch, tmp_path):
    config, records, trainer, dataset = _stub_train(monkeypatch, tmp_path)
    # both losses every step at step = t (zero-based); eval_score and the d4rl score right behind the step that ends a period
    keys = [(s, list(d)) for s, d in records]
    loss = ["critic_loss", "actor_loss"]
    assert keys == [(0, loss), (1, loss), (2, loss), (2, ["eval_score"]), (2, ["d4rl_normalized_score"]), (3, loss), (4, loss),
                    (5, loss), (5, ["eval_score"]), (5, ["d4rl_normalized_score"]), (6, loss)]
    assert [d["critic_loss"] for s, d in records if "critic_loss" in d] == [float(i) for i in range(7)]
    assert sorted(os.listdir(config.checkpoints_path)) == ["checkpoint_2.pt", "checkpoint_5.pt", "config.yaml"]
    assert torch.load(os.path.join(config.checkpoints_path, "checkpoint_5.pt"))["total_it"] == 6
    assert trainer.total_it == 7 and trainer._actor.mode == "train"
    # the scores are awac:487-492's: the mean return, and (get_normalized_score(returns) * 100).mean()
    env = awac.wrap_env(obe.OfflineBCEnv(), 0.0, 1.0)
    scores = awac.eval_actor(env, _Actor(), "cpu", 2, config.test_seed)
    assert [d["eval_score"] for s, d in records if "eval_score" in d] == [scores.mean()] * 2
    want = (env.get_normalized_score(scores) * 100.0).mean()
    assert [d["d4rl_normalized_score"] for s, d in records if "d4rl_normalized_score" in d] == [want, want]
    # the buffer got the z-scored dataset, rewards untouched (normalize_reward is off), the dict rewritten in place
    raw = obe.make_dataset(11)
    mean, std = awac.compute_mean_std(raw["observations"], eps=1e-3)
    np.testing.assert_array_equal(_Buffer.made[0].data["observations"], (raw["observations"] - mean) / std)
    np.testing.assert_array_equal(_Buffer.made[0].data["rewards"], raw["rewards"])
    assert dataset["observations"] is not None and np.array_equal(dataset["observations"], _Buffer.made[0].data["observations"])
    assert all(e is None for e in _Stepper.seen)  # noise="device": nothing injected


def test_group_records_carry_their_seed_and_no_other_key(monkeypatch, tmp_path):
    """K = 2: what reaches the logger is a loss record or one of awac's two evaluation records, each under the
    seed of its member -- nothing the loop and the flavour pass between them leaks into a record."""
    config, records, trainers, _ = _stub_train(monkeypatch, tmp_path, seeds_per_gpu=2)
    seeds = [config.seed, config.seed + 1]
    assert len(trainers) == 2 and sorted(os.listdir(config.checkpoints_path)) == ["config.yaml", "seed_6", "seed_7"]
    allowed = set(awac.LOSS_NAMES) | {"eval_score", "d4rl_normalized_score", "seed"}
    assert all(set(d) <= allowed and d["seed"] in seeds for s, d in records)
    for seed in seeds:
        mine = [(s, [k for k in d if k != "seed"]) for s, d in records if d["seed"] == seed]
        assert [s for s, k in mine if k == ["critic_loss", "actor_loss"]] == list(range(7))
        assert [(s, k) for s, k in mine if len(k) == 1] == [(2, ["eval_score"]), (2, ["d4rl_normalized_score"]),
                                                            (5, ["eval_score"]), (5, ["d4rl_normalized_score"])]
    # evaluations in member order, each member's two records together
    evals = [(s, d["seed"], next(k for k in d if k != "seed")) for s, d in records if "critic_loss" not in d]
    assert evals == [(t, seed, name) for t in (2, 5) for seed in seeds for name in ("eval_score", "d4rl_normalized_score")]
    env = awac.wrap_env(obe.OfflineBCEnv(), 0.0, 1.0)
    scores = awac.eval_actor(env, _Actor(), "cpu", 2, config.test_seed)
    assert all(d["eval_score"] == scores.mean() for s, d in records if "eval_score" in d)
    want = (env.get_normalized_score(scores) * 100.0).mean()
    assert all(d["d4rl_normalized_score"] == want for s, d in records if "d4rl_normalized_score" in d)


def test_train_hands_recorded_noise_to_the_steps(monkeypatch, tmp_path):
    eps = np.random.default_rng(0).standard_normal((7, 2, 4, 6)).astype(np.float32)
    _stub_train(monkeypatch, tmp_path, noise=eps)
    got = torch.cat(_Stepper.seen).numpy()
    assert np.array_equal(got, eps)
    calls = []

    def source(k, t, n):
        calls.append((k, t, n))
        return eps[t:t + n]
    _stub_train(monkeypatch, tmp_path / "b", noise=source, normalize_reward=True)
    assert calls == [(0, 0, 2), (0, 2, 1), (0, 3, 2), (0, 5, 1), (0, 6, 1)]
    d = obe.make_dataset(11)
    awac.modify_reward(d, obe.ENV)
    np.testing.assert_array_equal(_Buffer.made[0].data["rewards"], d["rewards"])
    with pytest.raises(ValueError, match="shape"):
        _stub_train(monkeypatch, tmp_path / "c", noise=eps[:, :1])


def test_train_checks_its_arguments_first():
    with pytest.raises(ValueError, match="sampler"):
        awac.train(awac.TrainConfig(), {}, None, sampler="philox")
    with pytest.raises(ValueError, match="seeds_per_gpu"):
        awac.train(awac.TrainConfig(), {}, None, seeds_per_gpu=17)
    with pytest.raises(ValueError, match="noise"):
        awac.train(awac.TrainConfig(hidden_dim=32), obe.make_dataset(11), obe.OfflineBCEnv(), noise="host", device="cpu")


def test_fixture_run_is_what_the_generator_would_choose_again(run):
    """The recorded seed is the first candidate that kept both margins, the candidates before it did not, and the
    stored fractions of the float64 twin stay under 1 for twice the recorded length."""
    steps, every = int(run["common/num_train_ops"]), int(run["common/eval_frequency"])
    cand, ok = run["run/candidates"].tolist(), run["run/candidate_ok"].tolist()
    assert cand == list(range(int(run["common/first_seed"]), int(run["run/seed"]) + 1)) and ok == [False] * (len(ok) - 1) + [True]
    assert run["run/f64_gap_of_bound"].shape == (2 * steps, 2) and run["run/f64_gap_of_bound"].max() < 1
    assert run["run/f64_eval_gap_of_bound"].shape == (2 * steps // every,) and run["run/f64_eval_gap_of_bound"].max() < 1
    assert float(run["run/kink_margin"]) > 1 and float(run["common/kink_sigmas"]) == 4.0
    assert run["run/eps"].shape == (steps, 2, int(run["common/batch_size"]), 6) and run["run/eps"].dtype == np.float32
    assert run["run/eval_returns"].shape == (steps // every, int(run["common/n_test_episodes"]))
    assert [str(n) for n in run["run/save_name"]] == [f"checkpoint_{t}.pt" for t in range(every - 1, steps, every)]
