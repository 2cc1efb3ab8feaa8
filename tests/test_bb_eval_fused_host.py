"""Host side of the fused BB evaluation (no GPU): iqlhip_bb_sim_episodes and its scratch-size helper are
declared, exported and bound without an ABI bump; every refusal of theirs that returns before a HIP call, with
its code and message; the ``eval_on`` argument check of ``custom_offline_bb.train``.

The pointers handed over here are made-up non-null addresses: a refused call dereferences none of them."""
import ctypes as C
import os
import re

import pytest

from tests import bb_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from iqlpref_amd import _lib
    return _lib.load()


def _sim(injected=False, n_near=6):
    from iqlpref_amd import _lib
    b = _lib.BbSim()
    b.n_obs, b.n_near, b.state_dim, b.action_dim, b.max_horizon = 50, n_near, 2 + 3 * n_near + 6, 2, 8
    b.actor_out_stride = 2 if injected else 0
    for name in ("state", "drift", "ctl", "obs_hist", "act_hist", "record", "actor_in", "actor_out", "state_mean",
                 "state_std", "min_actions", "max_actions"):
        setattr(b, name, FAKE)
    return b


def _actor(dims, hidden_act=0, out_act=1, dropout_p=0.0):
    from iqlpref_amd import _lib
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, w in enumerate(dims):
        d.dims[i] = w
    for i in range(d.n_layers):
        d.weights[i], d.biases[i] = FAKE, FAKE
    d.hidden_act, d.out_act, d.dropout_p = hidden_act, out_act, dropout_p
    return d


def _call(lib, sims, actors, n=None, scratch=FAKE, scratch_bytes=1 << 30):
    from iqlpref_amd import _lib
    K = len(sims)
    sim_arr = (_lib.BbSim * K)(*sims) if sims else None
    act_arr = (C.POINTER(_lib.MlpDesc) * max(K, 1))(*[C.pointer(a) if a is not None else C.POINTER(_lib.MlpDesc)()
                                                      for a in actors]) if actors is not None else None
    rc = lib.iqlhip_bb_sim_episodes(sim_arr, act_arr, K if n is None else n, scratch, scratch_bytes, None)
    return rc, lib.iqlhip_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from iqlpref_amd import _lib
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    P, PD = C.c_void_p, C.POINTER(C.POINTER(_lib.MlpDesc))
    want = {
        # (sims[n], actors[n], n, scratch, scratch_bytes, stream)
        "iqlhip_bb_sim_episodes": (C.c_int, [C.POINTER(_lib.BbSim), PD, C.c_int32, P, C.c_size_t, P]),
        # (actors[n], n, bytes)
        "iqlhip_bb_sim_episodes_scratch_bytes": (C.c_int, [PD, C.c_int32, C.POINTER(C.c_size_t)]),
    }
    for name, (res, args) in want.items():
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 6 and lib.iqlhip_abi_version() == 6
    import iqlpref_amd as ia
    assert ia.bb_run_eval_fused is ia.custom_offline_bb.bb_run_eval_fused
    assert ia.bb_run_eval_fused_group is ia.custom_offline_bb.bb_run_eval_fused_group


def test_scratch_holds_the_blocks_and_one_image_per_actor(lib):
    from iqlpref_amd import _lib
    a = _actor([26, 40, 40, 2])  # padded 32 x 48, 48 x 48, 48 x 16 floats
    image = (32 * 48 + 48 * 48 + 48 * 16) * 4
    sizes = []
    for K in (1, 3):
        arr = (C.POINTER(_lib.MlpDesc) * K)(*[C.pointer(a)] * K)
        need = C.c_size_t(0)
        assert lib.iqlhip_bb_sim_episodes_scratch_bytes(arr, K, C.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] >= image and sizes[1] - sizes[0] >= 2 * image
    assert sizes[1] - sizes[0] < 2 * (image + 256) + 3 * 1024  # (two images and two argument blocks more)
    none = (C.POINTER(_lib.MlpDesc) * 1)(C.POINTER(_lib.MlpDesc)())
    need = C.c_size_t(0)
    assert lib.iqlhip_bb_sim_episodes_scratch_bytes(none, 1, C.byref(need)) == 0 and 0 < need.value <= 1024
    for K in (0, _lib.MAX_GROUP + 1):
        assert lib.iqlhip_bb_sim_episodes_scratch_bytes(none, K, C.byref(need)) == _lib.ERR_INVALID
    assert lib.iqlhip_bb_sim_episodes_scratch_bytes(None, 1, C.byref(need)) == _lib.ERR_INVALID
    assert lib.iqlhip_bb_sim_episodes_scratch_bytes(none, 1, None) == _lib.ERR_INVALID
    wide = _actor([26, 272, 2])
    arr = (C.POINTER(_lib.MlpDesc) * 1)(C.pointer(wide))
    assert lib.iqlhip_bb_sim_episodes_scratch_bytes(arr, 1, C.byref(need)) == _lib.ERR_UNSUPPORTED


def test_refusals_before_any_hip_call(lib):
    from iqlpref_amd import _lib
    good = _actor([26, 32, 2])
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    nine = _actor([26, 16, 2])
    nine.n_layers = 9
    cases = [
        ("n = 0", _call(lib, [_sim()], [good], n=0), INV, "n = 0"),
        ("n = 17", _call(lib, [_sim()], [good], n=17), INV, "n = 17"),
        ("null sims", _call(lib, [], [good], n=1), INV, "null simulators"),
        ("null actors", _call(lib, [_sim()], None), INV, "null actors"),
        ("null scratch", _call(lib, [_sim()], [good], scratch=None), INV, "null scratch"),
        ("misaligned scratch", _call(lib, [_sim()], [good], scratch=FAKE + 4), INV, "16-byte"),
        ("null actor, no table", _call(lib, [_sim()], [None]), INV, "null actor and no injected table"),
        ("second episode's null actor", _call(lib, [_sim(True), _sim()], [None, None]), INV, "episode 1"),
        ("11 -> 2 actor", _call(lib, [_sim()], [_actor([11, 32, 2])]), INV, "maps 11 -> 2"),
        ("26 -> 3 actor", _call(lib, [_sim()], [_actor([26, 32, 3])]), INV, "maps 26 -> 3"),
        ("272 wide", _call(lib, [_sim()], [_actor([26, 272, 2])]), UNS, "272 > 256"),
        ("9 layers", _call(lib, [_sim()], [nine]), INV, "n_layers"),
        ("table activation", _call(lib, [_sim()], [_actor([26, 32, 2], hidden_act=8)]), UNS, "activations"),
        ("dropout", _call(lib, [_sim()], [_actor([26, 32, 2], dropout_p=0.1)]), UNS, "dropout"),
        ("short scratch", _call(lib, [_sim()], [good], scratch_bytes=1024), INV, "scratch of 1024 bytes"),
        ("a simulator's own check", _call(lib, [_sim(n_near=6), _sim(n_near=17)], [good, good]), UNS, "n_near = 17"),
    ]
    for what, (rc, msg), code, text in cases:
        assert rc == code and text in msg, (what, rc, msg)
    null_w = _actor([26, 32, 2])
    null_w.weights[1] = None
    rc, msg = _call(lib, [_sim()], [null_w])
    assert rc == INV and "null weight" in msg


def test_eval_on_argument_check():
    from iqlpref_amd import custom_offline_bb as bb
    with pytest.raises(ValueError, match="eval_on"):
        bb.train(bb.TrainConfig(), dataset=bb_env.synth_dataset(), move_stats=bb_env.MOVE_STATS, device="cuda:0",
                 eval_on="nonsense")
    # "fused" passes the argument check: the call gets as far as the missing reward model
    with pytest.raises((ImportError, NotImplementedError), match="reward_model"):
        bb.train(bb.TrainConfig(), dataset=bb_env.synth_dataset(), move_stats=bb_env.MOVE_STATS, device="cuda:0",
                 eval_on="fused")
