"""Host side of the BB flavour's seed groups (no GPU): the two new C entry points are declared, exported and
bound with the stated signatures and without an ABI bump; how ``custom_offline_bb.train(seeds_per_gpu=K)``
gets its K permutations and its K seeds; the range checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import bb_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = bb_env.N_ROWS, bb_env.BATCH


@pytest.fixture(scope="module")
def bb():
    from iqlpref_amd import custom_offline_bb
    return custom_offline_bb


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    lib = _lib.load()
    P, PP, RV = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_lib.ReplayView)
    want = {
        # (g, views, n_steps, idx, n_valid, dropout_keep, losses_out, graph_unroll, stream)
        "iqlhip_group_train_steps_valid": (C.c_int, [P, RV, C.c_int64, PP, PP, PP, PP, C.c_int32, P]),
        # (perm[K], n_rows, batch, t0, n_steps, idx[K], n_valid, K, stream)
        "iqlhip_block_epoch_indices_group": (C.c_int, [PP, C.c_int64, C.c_int32, C.c_int64, C.c_int64, PP, P,
                                                       C.c_int32, P]),
    }
    for name, (res, args) in want.items():
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args
    assert "seed groups take no counts" not in header
    assert _lib.ABI_VERSION == 6 and lib.iqlhip_abi_version() == 6
    # refused before any device work: null handles, K outside 1..MAX_GROUP
    assert lib.iqlhip_group_train_steps_valid(None, None, 1, None, None, None, None, 0, None) == _lib.ERR_INVALID
    one = (C.c_void_p * 1)(None)
    for K in (0, _lib.MAX_GROUP + 1):
        assert lib.iqlhip_block_epoch_indices_group(one, N, B, 0, 1, one, C.c_void_p(8), K, None) == _lib.ERR_INVALID
    assert lib.iqlhip_block_epoch_indices_group(one, N, B, 0, 1, None, None, 1, None) == _lib.ERR_INVALID


def test_python_surface(bb):
    import inspect
    import iqlpref_amd as ia
    assert inspect.signature(ia.SeedGroup.train_steps).parameters["n_valid"].default is None
    sig = inspect.signature(bb.train).parameters["seeds_per_gpu"]
    assert sig.default == 1 and sig.kind is inspect.Parameter.KEYWORD_ONLY
    assert "Seed groups, sweeps and bf16 are not offered" not in bb.__doc__
    assert "Sweeps and bf16 are not offered" in bb.__doc__


def test_none_draws_k_permutations_in_member_order(bb):
    torch.manual_seed(1234)
    group = bb.BlockEpochSamplerGroup.draw(N, B, 3)
    after = torch.randperm(N // B)  # the generator is where three draws leave it
    torch.manual_seed(1234)
    want = [torch.randperm(N // B) for _ in range(4)]
    assert len(group) == 3 and (group.n_rows, group.batch_size) == (N, B)
    for sm, w in zip(group.samplers, want):
        np.testing.assert_array_equal(sm.perm.numpy(), w.numpy())
    np.testing.assert_array_equal(after.numpy(), want[3].numpy())
    # one member: the draw of a lone BlockEpochSampler
    torch.manual_seed(7)
    one = bb.BlockEpochSamplerGroup.draw(N, B, 1).samplers[0].perm
    torch.manual_seed(7)
    np.testing.assert_array_equal(one.numpy(), bb.BlockEpochSampler(N, B).perm.numpy())


def test_explicit_permutations(bb):
    perms = [np.array([4, 3, 2, 1, 0]), [0, 1, 2, 3, 4], torch.tensor([2, 0, 4, 1, 3])]
    state = torch.get_rng_state()
    group = bb.BlockEpochSamplerGroup.draw(N, B, 3, perms)
    assert torch.equal(torch.get_rng_state(), state)  # nothing is drawn
    for sm, p in zip(group.samplers, perms):
        np.testing.assert_array_equal(sm.perm.numpy(), np.asarray(p))
        np.testing.assert_array_equal(sm.host_indices(0, 6)[1], [B] * 5 + [N % B])
    for bad in (perms[:2], perms + perms[:1], perms[0], []):  # wrong length; ONE permutation for three seeds
        with pytest.raises(ValueError, match="sequence of 3"):
            bb.BlockEpochSamplerGroup.draw(N, B, 3, bad)
    with pytest.raises(ValueError, match="permutation of 0..4"):
        bb.BlockEpochSamplerGroup.draw(N, B, 2, [perms[0], [0, 1, 2, 3, 3]])


def test_samplers_of_a_group_share_one_epoch_shape(bb):
    a = bb.BlockEpochSampler(N, B)
    with pytest.raises(ValueError, match="one epoch shape"):
        bb.BlockEpochSamplerGroup([a, bb.BlockEpochSampler(N - 7, B)])
    with pytest.raises(ValueError, match="one epoch shape"):
        bb.BlockEpochSamplerGroup([a, bb.BlockEpochSampler(N, B // 2)])
    from iqlpref_amd import _lib
    with pytest.raises(ValueError, match="1..16"):
        bb.BlockEpochSamplerGroup([])
    with pytest.raises(ValueError, match="1..16"):
        bb.BlockEpochSamplerGroup([a] * (_lib.MAX_GROUP + 1))
    assert len(bb.BlockEpochSamplerGroup([a] * _lib.MAX_GROUP)) == _lib.MAX_GROUP


def test_seeds_come_from_rank_seed(bb, monkeypatch):
    from iqlpref_amd import distributed as D
    assert bb.group_seeds(10, 1) == [10] and bb.group_seeds(10, 3) == [10, 11, 12]
    calls = []

    def rank2(base, k=1):  # what rank 2 of a distributed run gets
        calls.append((base, k))
        return base + 2 * k

    monkeypatch.setattr(D, "rank_seed", rank2)
    assert bb.group_seeds(10, 4) == [18, 19, 20, 21] and calls == [(10, 4)]


@pytest.mark.parametrize("k", [0, -1, 17])
def test_seeds_per_gpu_range(bb, k):
    with pytest.raises(ValueError, match="seeds_per_gpu must be in 1..16"):
        bb.group_seeds(0, k)
    # train() checks it first: before the reward model, the dataset or a device is looked at
    with pytest.raises(ValueError, match="seeds_per_gpu must be in 1..16"):
        bb.train(bb.TrainConfig(), seeds_per_gpu=k)
