"""K seeds per GPU for the fine-tune flavour, what needs no GPU: the two group entry points exist and refuse
bad arguments before they look at a device, and ``finetune.train(seeds_per_gpu=...)`` checks its arguments
before anything is built, loaded or launched (on a machine without a GPU any later step would raise
RuntimeError instead)."""
import ctypes as C

import pytest

from iqlpref_amd import _lib
from iqlpref_amd import finetune as ft
from tests import finetune_env as fe


def test_library_exports_the_group_entry_points():
    lib = _lib.load()
    assert "iqlhip_explore_action_group" in _lib.SYMBOLS and "iqlhip_replay_append_group" in _lib.SYMBOLS
    assert lib.iqlhip_explore_action_group is not None and lib.iqlhip_replay_append_group is not None
    assert _lib.ABI_VERSION == 6 and lib.iqlhip_abi_version() == 6  # entry points were added, nothing changed


def test_explore_action_group_refuses_null_and_k_out_of_range():
    lib = _lib.load()
    some = C.c_void_p(64)  # never dereferenced: the calls below fail on an earlier check
    trainers = (C.c_void_p * 17)(*[64] * 17)
    calls = (C.c_uint32 * 17)()
    call = lambda tr, K, s, c, out: lib.iqlhip_explore_action_group(tr, K, s, 8, None, 0.03, 0.5, 1.0, c, out, None)
    assert call(None, 1, some, calls, some) == _lib.ERR_INVALID
    assert call(trainers, 1, None, calls, some) == _lib.ERR_INVALID
    assert call(trainers, 1, some, None, some) == _lib.ERR_INVALID
    assert call(trainers, 1, some, calls, None) == _lib.ERR_INVALID
    for K in (0, 17, -1):
        assert call(trainers, K, some, calls, some) == _lib.ERR_INVALID
        assert b"1..16" in lib.iqlhip_last_error()
    none = (C.c_void_p * 2)(None, None)
    assert call(none, 2, some, calls, some) == _lib.ERR_INVALID  # a null member


def test_replay_append_group_refuses_null_and_k_out_of_range():
    lib = _lib.load()
    some = C.c_void_p(64)
    rows = (C.c_void_p * 17)(*[64 * (k + 1) for k in range(17)])
    cap, pointer = (C.c_int64 * 17)(*[4] * 17), (C.c_int64 * 17)()
    S, A = 5, 3
    stride = lib.iqlhip_replay_row_stride(S, A)
    call = lambda r, c, p, K, stage, st=stride: lib.iqlhip_replay_append_group(r, st, S, A, c, p, K, stage, None)
    assert call(None, cap, pointer, 1, some) == _lib.ERR_INVALID
    assert call(rows, None, pointer, 1, some) == _lib.ERR_INVALID
    assert call(rows, cap, None, 1, some) == _lib.ERR_INVALID
    assert call(rows, cap, pointer, 1, None) == _lib.ERR_INVALID
    for K in (0, 17):
        assert call(rows, cap, pointer, K, some) == _lib.ERR_INVALID
        assert b"1..16" in lib.iqlhip_last_error()
    assert call(rows, cap, pointer, 2, some, stride - 4) == _lib.ERR_INVALID  # a stride below the row's
    full = (C.c_int64 * 17)(*[4] * 17)  # pointer == capacity: the full ring of fref:173
    assert call(rows, cap, full, 2, some) == _lib.ERR_INVALID
    odd = (C.c_void_p * 2)(64, 68)  # not on a 16-byte boundary
    assert call(odd, cap, pointer, 2, some) == _lib.ERR_INVALID
    twice = (C.c_void_p * 2)(64, 64)
    assert call(twice, cap, pointer, 2, some) == _lib.ERR_INVALID


def _config():
    return ft.TrainConfig(device="cuda", env="antmaze-test", offline_iterations=2, online_iterations=2, buffer_size=16,
                          batch_size=16, eval_freq=2, n_episodes=1)


@pytest.mark.parametrize("K", [0, 17, -3])
def test_train_refuses_a_group_size_out_of_range(K):
    envs = [fe.FinetuneEnv("antmaze-test") for _ in range(max(K, 1))]
    with pytest.raises(ValueError, match="seeds_per_gpu"):
        ft.train(_config(), envs, envs, fe.make_dataset("antmaze-test", 8, 0), seeds_per_gpu=K)


@pytest.mark.parametrize("which", ["env", "eval_env", "single"])
def test_train_refuses_a_wrong_number_of_environments(which):
    mk = lambda n: [fe.FinetuneEnv("antmaze-test") for _ in range(n)]
    env, eval_env = (mk(2), mk(3)) if which == "env" else (mk(3), mk(4)) if which == "eval_env" else (mk(3), mk(1)[0])
    dataset = fe.make_dataset("antmaze-test", 8, 0)
    before = {k: v.copy() for k, v in dataset.items()}
    with pytest.raises(ValueError, match="environments"):
        ft.train(_config(), env, eval_env, dataset, seeds_per_gpu=3)
    assert all((dataset[k] == before[k]).all() for k in before)  # nothing was normalised or rescaled
