"""The actor's dropout masks of the tuned step are drawn once per step, with the batch (k_stage, the idle
work-groups of k_update), into a plane that the forward kernels read.  Nothing of that may show: a trainer
that draws its own masks equals, bit for bit (losses and every tensor of ``state_dict()``), a twin that is
handed ``oracle.philox.dropout_keep`` through ``dropout_keep=``, whatever forward kernel the launch takes and
however calls, buffers, index modes and step jumps follow each other.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

from oracle import philox
from tests import helpers

pytestmark = pytest.mark.gpu

P_DROP = 0.1
N_ROWS = 600


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


def _case(S, A, H, E=2, p=P_DROP, seed=0):
    """(hyper, nets, data): random networks (an actor with dropout p) and a small synthetic dataset."""
    rng = np.random.default_rng(1000 * H + 10 * S + E + seed)
    hyper = dict(s_dim=S, a_dim=A, hidden=H, n_hidden=2, deterministic=False, dropout=p, iql_tau=0.8, beta=3.0,
                 max_steps=1000, discount=0.99, tau=0.005, n_rows=N_ROWS, n_critics=E)
    nets = helpers.forward_nets(rng, S, A, H, n_critics=E, dropout=p)
    data = {"observations": rng.standard_normal((N_ROWS, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (N_ROWS, A)).astype(np.float32),
            "rewards": rng.standard_normal(N_ROWS).astype(np.float32),
            "next_observations": rng.standard_normal((N_ROWS, S)).astype(np.float32),
            "terminals": (rng.uniform(size=N_ROWS) < 0.05).astype(np.float32)}
    return hyper, nets, data


def _oracle_keep(gh, seed, step0, n, B, H, p=P_DROP):
    """[n, 2, B, H] uint8 on the device: the masks of steps step0 .. step0 + n - 1 of a trainer of this seed.
    (The stream is keyed by the row block, not by the batch size: a batch of B rows takes the first B rows
    of the masks of B rounded up to 16, the rows the kernels work on.)"""
    Bp = (B + 15) // 16 * 16
    m = np.stack([np.stack([philox.dropout_keep(seed, step0 + t, layer, Bp, H, p)[:B] for layer in (1, 2)])
                  for t in range(n)])
    return torch.from_numpy(m.astype(np.uint8)).to(gh.DEV)


def _tensors(x, path=""):
    if isinstance(x, torch.Tensor):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _tensors(v, f"{path}/{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _tensors(v, f"{path}/{i}")


def _same_state(a, b):
    ta, tb = list(_tensors(a.state_dict())), list(_tensors(b.state_dict()))
    assert [k for k, _ in ta] == [k for k, _ in tb] and len(ta) > 12
    for (k, va), (_, vb) in zip(ta, tb):
        assert torch.equal(va, vb), k
    for (k, va), (_, vb) in zip(a.q_target.state_dict().items(), b.q_target.state_dict().items()):
        assert torch.equal(va, vb), "q_target/" + k
    assert a.total_it == b.total_it


def _device_equals_injected(gh, S, A, H, B, mode, E=2, steps=4, seed=7):
    hyper, nets, data = _case(S, A, H, E)
    buf = gh.make_buffer(hyper, data)
    dev, inj = (gh.make_trainer(hyper, nets, mode, seed=seed) for _ in range(2))
    assert dev.step_kind(B) == "tuned"
    ld = dev.train_steps(buf, steps, B, graph_unroll=0)
    li = inj.train_steps(buf, steps, B, dropout_keep=_oracle_keep(gh, seed, 0, steps, B, H), graph_unroll=0)
    assert torch.isfinite(ld).all()
    assert torch.equal(ld, li)
    _same_state(dev, inj)
    return dev


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [16, 48])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_device_masks_equal_injected_oracle_masks(gh, H, B, mode):
    """One, two and four layer-2 parts per slab (H = 64, 128, 256: which part work-group stores a layer-1
    tile differs), one and three slabs.  Step 0's masks come from k_stage, the others from k_update."""
    _device_equals_injected(gh, 11, 3, H, B, mode)


def test_two_output_tiles_and_three_layer1_k_steps(gh):
    """The pen shapes: A = 24 is two output tiles, S + A = 69 three bf16 k-steps of layer 1."""
    _device_equals_injected(gh, 45, 24, 256, 48, "bf16")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_padded_batch(gh, mode):
    """batch_size 17 runs on 32 rows (the counted kernels); the plane has the padded batch's row blocks."""
    _device_equals_injected(gh, 11, 3, 128, 17, mode)


def test_precomputation_is_invisible(gh, monkeypatch):
    """tests/test_gpu_step.py::test_batch_prefetch_is_invisible with a dropout trainer: the masks drawn ahead
    by k_update never serve a stale step -- whatever follows what, the bits are those of a trainer that
    draws them in k_stage before every step."""
    S, A, H, B = 11, 3, 128, 48
    hyper, nets, data = _case(S, A, H)
    buf_a = gh.make_buffer(hyper, data)
    buf_b = gh.make_buffer(hyper, {k: np.ascontiguousarray(v[::-1]) for k, v in data.items()})
    rng = np.random.default_rng(5)
    idx = torch.from_numpy(rng.integers(0, N_ROWS, (4, B))).to(gh.DEV)
    foreign = _oracle_keep(gh, 999, 0, 2, B, H, 0.3)  # injected masks that are nobody's own

    def run(tr):
        out = [tr.train_steps(buf_a, 4, B, graph_unroll=0)]                           # Philox, eager
        tr.train_steps(buf_a, 3, B, return_losses=False, graph_unroll=0)               # no outputs ...
        tr.train_steps(buf_a, 2, B, return_losses=False, graph_unroll=0)               # ... so this call continues it
        out.append(tr.train_steps(buf_b, 5, B, graph_unroll=2))                       # other buffer, graph + tail
        out.append(tr.train_steps(buf_a, 3, B, indices=idx[:3], graph_unroll=0))      # injected indices, own masks
        o = tr.train(buf_b.sample(B, indices=idx[3]))                                 # explicit batch
        out.append(torch.tensor([[o["value_loss"], o["q_loss"], o["actor_loss"]]], device=gh.DEV))
        out.append(tr.train_steps(buf_a, 2, B, dropout_keep=foreign, graph_unroll=0))  # injected masks ...
        tr.train_steps(buf_a, 2, B, return_losses=False, graph_unroll=0)               # ... then a call without
        out.append(tr.train_steps(buf_b, 5, B, graph_unroll=2))
        return torch.cat(out).cpu().numpy()

    # (the library reads the variable when it builds the native trainer, which step_kind() makes happen)
    tr_p = gh.make_trainer(hyper, nets, "bf16", seed=11)
    assert tr_p.step_kind(B) == "tuned"
    monkeypatch.setenv("IQLHIP_NO_PREFETCH", "1")
    tr_n = gh.make_trainer(hyper, nets, "bf16", seed=11)
    assert tr_n.step_kind(B) == "tuned"
    monkeypatch.delenv("IQLHIP_NO_PREFETCH")
    lp, ln = run(tr_p), run(tr_n)
    assert np.isfinite(lp).all()
    np.testing.assert_array_equal(lp, ln)
    _same_state(tr_p, tr_n)


@pytest.mark.parametrize("before", [0, 1])
def test_step_jump_rekeys_the_masks(gh, before):
    """3 steps, the checkpoint into another trainer of the same seed (fresh, or one step old: its plane then
    holds the masks of step 1), 3 more steps there = 6 steps straight.  (load_state_dict starts the target
    critics as a copy of qf, ref:679; the straight run's are handed over, as load_resume_state does.)"""
    S, A, H, B = 11, 3, 128, 48
    hyper, nets, data = _case(S, A, H)
    buf = gh.make_buffer(hyper, data)
    straight, first, second = (gh.make_trainer(hyper, nets, "bf16", seed=21) for _ in range(3))
    want = straight.train_steps(buf, 6, B, graph_unroll=0)
    got = [first.train_steps(buf, 3, B, graph_unroll=0)]
    if before:
        second.train_steps(buf, before, B, return_losses=False, graph_unroll=0)
    second.load_state_dict(first.state_dict())
    second.q_target.load_state_dict(first.q_target.state_dict())
    second.sync_weights()
    assert second.total_it == 3
    got.append(second.train_steps(buf, 3, B, graph_unroll=0))
    assert torch.equal(want, torch.cat(got))
    _same_state(straight, second)


def _group_equals_members_alone(gh, K, H, B, mode, rates=None, steps=3):
    """A group launch of K dropout trainers (their own masks, drawn on the device) against each member
    stepped alone with the oracle's masks injected."""
    import iqlpref_amd as ia
    S, A = 11, 3
    rates = rates or [P_DROP] * K
    cases = {p: _case(S, A, H, p=p) for p in set(rates)}
    buf = gh.make_buffer(*[cases[rates[0]][i] for i in (0, 2)])
    seeds = [30 + k for k in range(K)]
    alone = [gh.make_trainer(cases[p][0], cases[p][1], mode, seed=s) for s, p in zip(seeds, rates)]
    want = [t.train_steps(buf, steps, B, dropout_keep=_oracle_keep(gh, s, 0, steps, B, H, p), graph_unroll=0)
            for t, s, p in zip(alone, seeds, rates)]
    group = ia.SeedGroup([gh.make_trainer(cases[p][0], cases[p][1], mode, seed=s) for s, p in zip(seeds, rates)],
                         mode="group")
    assert group.mode == "group"
    got = group.train_steps(buf, steps, B, return_losses=True, graph_unroll=0)
    group.synchronize()
    for w, g, ta, tg in zip(want, got, alone, group.trainers):
        assert torch.equal(w, g)
        _same_state(ta, tg)
    assert not torch.equal(want[0], want[1])
    group.close()


def test_group_of_8_two_row_tiles(gh):
    """512 rows per launch: k_forward<.., MT 2, PW 1>."""
    _group_equals_members_alone(gh, 8, 128, 64, "bf16")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_group_of_16_two_row_tiles_two_parts(gh, mode):
    """1,024 rows per launch: k_forward<.., MT 2, PW 2>."""
    _group_equals_members_alone(gh, 16, 128, 64, mode)


def test_two_dropout_rates_in_one_group(gh):
    """Members of one group launch with different rates (tests/test_gpu_sweep.py groups pen runs so): the
    threshold is each member's own."""
    _group_equals_members_alone(gh, 2, 64, 16, "bf16", rates=[0.1, 0.25])


def test_throughput_forward(gh):
    """E = 8 critics at H 256 / batch 256 in bf16: 19 evaluations x 4 slabs of 64 rows = 76 forward
    work-groups, inside the window that takes k_forward_tp<256, true>."""
    _device_equals_injected(gh, 17, 6, 256, 256, "bf16", E=8, steps=3)
