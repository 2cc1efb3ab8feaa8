"""GPU: the general (layer-wise) preference-transformer relabel, iqlhip_pt_relabel_general, for
shapes beyond the tuned one-block kernel: deeper, wider, more heads, wider MLPs, larger inputs.
-m gpu.

PT numerics are PARITY UNPINNED (no runnable reference: JAX is absent): the checkers are the numpy
restatement oracle/relabel_oracle.py:pt_value_last and the tuned kernel at the shape both paths
cover.  The loose bound (5e-3, as test_gpu_relabel.py) absorbs bf16 rounding flips of a q.k logit;
the tight median bound catches a transposed tile or a wrong head split, whose errors are the size
of the values themselves."""
import numpy as np
import pytest
import torch

from oracle import relabel_oracle as ro
from tests.test_relabel_oracle import g5_dataset
from tests import helpers
from tests.helpers import PT_TOL as TOL, check_close, oracle_windows, random_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class FakeEnv:
    def __init__(self, m):
        self._max_episode_steps = m


def make_model(p, S, A, max_ep, heads, max_pos=64):
    """A RewardPT of whatever depth and width ``p`` holds (oracle.relabel_oracle.make_pt_params)."""
    import iqlpref_amd as ia
    E = p["state_linear.weight"].shape[0]
    L = 0
    while f"gpt.layers.{L}.layer_norm_0.weight" in p:
        L += 1
    m = ia.RewardPT(S, A, max_ep, embd_dim=E, pref_attn_embd_dim=(p["pref_linear.weight"].shape[0] - 1) // 2,
                    num_heads=heads, intermediate_dim=p["gpt.layers.0.mlp.in_linear.weight"].shape[0],
                    num_layers=L, max_pos=max_pos)
    missing = m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    assert all(k.endswith("causal_bias") for k in missing.missing_keys) and not missing.unexpected_keys
    return m.to(DEV)


@pytest.mark.parametrize("L,E,heads,I,S,A,QL", [
    (2, 64, 4, 256, 29, 8, 20),
    (3, 128, 8, 512, 45, 24, 25),
    (1, 256, 4, 1024, 29, 8, 100),
    (2, 256, 16, 1024, 5, 3, 12),
    (8, 64, 1, 64, 7, 3, 6),
    (1, 64, 4, 320, 29, 8, 20),   # only the MLP width leaves the tuned envelope
    (1, 64, 2, 256, 150, 100, 10),  # S + A > 192
    (2, 192, 8, 384, 11, 5, 16),    # head_dim 24: three features per lane of an 8-lane group
])
def test_general_vs_oracle(L, E, heads, I, S, A, QL):
    """Observed on an MI355X (max / median |d| over all windows, win_t0 given; the median bound is
    applied to the windows of len <= 8): L2 E64 h4 I256 1.5e-4 / 2.4e-7; L3 E128 h8 I512 2.0e-4 /
    9.5e-7; L1 E256 h4 I1024 QL100 3.6e-5 / 3.0e-7; L2 E256 h16 I1024 4.2e-4 / 6.0e-7; L8 E64 h1 I64
    3.9e-4 / 3.6e-7; L1 E64 h4 I320 3.5e-5 / 1.8e-7; S+A 250 1.5e-5 / 1.8e-7; L2 E192 h8 I384
    1.0e-4 / 3.4e-7."""
    rng = np.random.default_rng(1000 * L + E + I + S)
    max_ep = 150
    p = ro.make_pt_params(rng, S, A, max_ep, embd=E, pref=8, inter=I, layers=L)
    m = make_model(p, S, A, max_ep, heads, max_pos=max(64, 2 * QL))
    assert not m.tuned_shape()
    n_rows = 400
    obs = rng.standard_normal((n_rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    lens, starts, t0 = random_windows(rng, n_rows, max_ep, QL, 40)
    dv = lambda x: torch.from_numpy(x).to(DEV)
    got = m.window_values(dv(obs), dv(act), dv(starts), dv(lens), QL, win_t0=dv(t0)).cpu().numpy()
    want = oracle_windows(p, obs, act, starts, lens, t0, QL, heads)
    mx, med = check_close(got, want, short=lens <= 8)
    print(f"L{L} E{E} h{heads} I{I} S{S} A{A} QL{QL}: max |d| {mx:.3g}, median {med:.3g}")
    # win_t0 = None: timesteps 0..len-1
    got0 = m.window_values(dv(obs), dv(act), dv(starts), dv(lens), QL).cpu().numpy()
    check_close(got0, oracle_windows(p, obs, act, starts, lens, None, QL, heads), short=lens <= 8)


@pytest.mark.parametrize("heads", [1, 4, 16])
def test_general_vs_tuned_kernel(heads):
    """The two HIP implementations against each other at the tuned shape (1 block, embd_dim 64), and
    kernel="auto" there is the tuned kernel, bit for bit.  Observed on an MI355X (3,000 windows, max /
    median |d|): 1 head 2.1e-3 / 1.8e-7, 4 heads 4.0e-4 / 1.8e-7, 16 heads 1.5e-4 / 1.2e-7."""
    S, A, QL, max_ep = 29, 8, 20, 120
    rng = np.random.default_rng(heads)
    p = ro.make_pt_params(rng, S, A, max_ep, embd=64, pref=8, inter=256, layers=1)
    m = make_model(p, S, A, max_ep, heads)
    assert m.tuned_shape()
    n_rows, n_win = 5000, 3000
    dv = lambda x: torch.from_numpy(x).to(DEV)
    obs = dv(rng.standard_normal((n_rows, S)).astype(np.float32))
    act = dv(rng.uniform(-1, 1, (n_rows, A)).astype(np.float32))
    lens = rng.integers(1, QL + 1, n_win).astype(np.int32)
    starts = rng.integers(0, n_rows - QL, n_win).astype(np.int64)
    t0 = rng.integers(0, max_ep - QL, n_win).astype(np.int32)
    args = (obs, act, dv(starts), dv(lens), QL)
    tuned = m.window_values(*args, win_t0=dv(t0), kernel="tuned").cpu().numpy()
    general = m.window_values(*args, win_t0=dv(t0), kernel="general").cpu().numpy()
    auto = m.window_values(*args, win_t0=dv(t0)).cpu().numpy()
    np.testing.assert_array_equal(auto, tuned)
    mx, med = check_close(general, tuned.astype(np.float64), short=lens <= 8)
    print(f"heads {heads}: general vs tuned max |d| {mx:.3g}, median {med:.3g}")


def test_chunking_is_invisible():
    """50k windows through a workspace sized for 3,000 (17 chunks, the last one partial): bit-identical
    to one call per 1,000-window slice and to a second identical call; 24 spot checks vs the oracle."""
    S, A, QL, max_ep, heads = 11, 3, 8, 60, 4
    rng = np.random.default_rng(5)
    p = ro.make_pt_params(rng, S, A, max_ep, embd=64, pref=8, inter=128, layers=2)
    m = make_model(p, S, A, max_ep, heads)
    n_rows, n_win = 20000, 50000
    obs_np = rng.standard_normal((n_rows, S)).astype(np.float32)
    act_np = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    lens = rng.integers(1, QL + 1, n_win).astype(np.int32)
    starts = rng.integers(0, n_rows - QL, n_win).astype(np.int64)
    t0 = rng.integers(0, max_ep - QL, n_win).astype(np.int32)
    dv = lambda x: torch.from_numpy(x).to(DEV)
    o, a_, st, ln, tt = dv(obs_np), dv(act_np), dv(starts), dv(lens), dv(t0)
    got = m.window_values(o, a_, st, ln, QL, win_t0=tt, workspace_windows=3000).cpu().numpy()
    again = m.window_values(o, a_, st, ln, QL, win_t0=tt, workspace_windows=3000).cpu().numpy()
    np.testing.assert_array_equal(got, again)
    sliced = np.concatenate([m.window_values(o, a_, st[i:i + 1000], ln[i:i + 1000], QL,
                                             win_t0=tt[i:i + 1000]).cpu().numpy()
                             for i in range(0, n_win, 1000)])
    np.testing.assert_array_equal(got, sliced)
    pick = rng.choice(n_win, 24, replace=False)
    want = oracle_windows(p, obs_np, act_np, starts[pick], lens[pick], t0[pick], QL, heads)
    np.testing.assert_allclose(got[pick], want, rtol=TOL, atol=TOL)


@pytest.mark.parametrize("correct", [False, True])
def test_qlearning_dataset_pt_two_blocks(correct):
    import iqlpref_amd as ia
    ds = g5_dataset(np.load(helpers.GOLDEN + "/dataset_ops.npz"))
    S, A, QL = 4, 2, 5
    rng = np.random.default_rng(19)
    p = ro.make_pt_params(rng, S, A, 20, embd=128, pref=8, inter=256, layers=2)
    m = make_model(p, S, A, 20, 4)
    out = ia.qlearning_dataset_pt(FakeEnv(15), m, query_length=QL, dataset=ds, correct_window_offsets=correct)
    want = ro.qlearning_dataset_pt(ds, p, 15, QL, num_heads=4, correct_window_offsets=correct)
    for k in want:
        np.testing.assert_allclose(np.asarray(out[k], dtype=np.float32), np.asarray(want[k], dtype=np.float32),
                                   rtol=TOL, atol=TOL, err_msg=k)


def test_custom_offline_dataset_two_blocks():
    from iqlpref_amd import custom_offline as co
    S, A, QL = 11, 3, 8
    rng = np.random.default_rng(23)
    eps = [{"observations": rng.standard_normal((L + 1, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (L, A)).astype(np.float32),
            "terminations": (np.arange(L) == L - 1) & (rng.uniform() < 0.5)} for L in (3, 8, 9, 25, 1)]
    p = ro.make_pt_params(rng, S, A, 200, embd=128, pref=16, inter=512, layers=2)
    model = make_model(p, S, A, 200, 4)
    got = co.qlearning_dataset(eps, model, QL)
    want = ro.custom_qlearning_dataset(eps, p, QL, num_heads=4)
    for k in ("observations", "actions", "next_observations", "terminals"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got["rewards"], want["rewards"], rtol=TOL, atol=TOL)


def _loader_windows(rng, p, m, S, A, QL, max_ep, heads):
    n_rows = 200
    obs = rng.standard_normal((n_rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (n_rows, A)).astype(np.float32)
    lens, starts, t0 = random_windows(rng, n_rows, max_ep, QL, 20)
    dv = lambda x: torch.from_numpy(x).to(DEV)
    got = m.window_values(dv(obs), dv(act), dv(starts), dv(lens), QL, win_t0=dv(t0)).cpu().numpy()
    np.testing.assert_allclose(got, oracle_windows(p, obs, act, starts, lens, t0, QL, heads), rtol=TOL, atol=TOL)


def test_loaders_three_blocks(tmp_path):
    """A checkpoint in the reference's key layout (best_model.pt {"net": ...} with the torch.compile
    prefix, config.yaml with num_heads / intermediate_dim) and a flax-style nested tree, both with
    3 blocks of width 128."""
    import iqlpref_amd as ia
    from iqlpref_amd import custom_offline as co
    S, A, QL, max_ep, heads, L = 9, 4, 12, 80, 8, 3
    rng = np.random.default_rng(31)
    p = ro.make_pt_params(rng, S, A, max_ep, embd=128, pref=16, inter=384, layers=L)
    state = {"_orig_mod." + k: torch.from_numpy(v) for k, v in p.items()}
    for l in range(L):
        state[f"_orig_mod.gpt.layers.{l}.attention.causal_bias"] = torch.tril(torch.ones(1, 1, 64, 64))
    torch.save({"net": state}, tmp_path / "best_model.pt")
    (tmp_path / "config.yaml").write_text(f"num_heads: {heads}\nintermediate_dim: 384\nmodel_eps: 1.0e-5\n")
    m = ia.load_pt_reward_model(str(tmp_path), device=DEV)
    assert len(m.gpt.layers) == L and m.state_linear.out_features == 128 and m.num_heads == heads
    _loader_windows(rng, p, m, S, A, QL, max_ep, heads)

    # flax nnx tree: kernel [in, out], LayerNorm scale, Embed embedding; layers as a nested dict
    def lin(name):
        return {"kernel": p[name + ".weight"].T.copy(), "bias": p[name + ".bias"]}

    def ln(name):
        return {"scale": p[name + ".weight"], "bias": p[name + ".bias"]}
    tree = {"state_linear": lin("state_linear"), "action_linear": lin("action_linear"),
            "timestep_embed": {"embedding": p["timestep_embed.weight"]},
            "stacked_layer_norm": ln("stacked_layer_norm"),
            "gpt": {"layers": {l: {"layer_norm_0": ln(f"gpt.layers.{l}.layer_norm_0"),
                                   "attention": {"in_linear": lin(f"gpt.layers.{l}.attention.in_linear"),
                                                 "out_linear": lin(f"gpt.layers.{l}.attention.out_linear")},
                                   "layer_norm_1": ln(f"gpt.layers.{l}.layer_norm_1"),
                                   "mlp": {"in_linear": lin(f"gpt.layers.{l}.mlp.in_linear"),
                                           "out_linear": lin(f"gpt.layers.{l}.mlp.out_linear")}}
                               for l in range(L)},
                    "layer_norm": ln("gpt.layer_norm")},
            "pref_linear": lin("pref_linear")}
    fm = ia.RewardPT(S, A, max_ep, embd_dim=128, pref_attn_embd_dim=16, num_heads=heads, intermediate_dim=384,
                     num_layers=L, max_pos=64)
    fm = co.load_pt_flax_params(fm, tree).to(DEV)
    _loader_windows(rng, p, fm, S, A, QL, max_ep, heads)
