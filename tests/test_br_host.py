"""The Bayesian-reward flavour (custom_offline_br, bref = algorithms/custom_offline/iql_br.py) without
a GPU: the library's new entry points refuse what is outside their envelope before any HIP call, the
Python surface carries the reference's config and errors, and the numpy restatement "N choice() calls
are one randint stream" reproduces the reference's recorded output bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import br_env
from tests import custom_train_env as cte


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "br_relabel.npz")))


@pytest.fixture(scope="module")
def lib():
    from iqlpref_amd import _lib
    return _lib.load()


# --------------------------------------------------------------------------- #
# C-ABI
# --------------------------------------------------------------------------- #
def test_symbols_exported_and_abi_kept(lib):
    from iqlpref_amd import _lib
    assert "iqlhip_posterior_choice" in _lib.SYMBOLS and "iqlhip_posterior_choice_workspace_bytes" in _lib.SYMBOLS
    assert lib.iqlhip_posterior_choice is not None
    assert lib.iqlhip_abi_version() == 6


def test_workspace_is_chunk_sized(lib):
    from iqlpref_amd import _lib
    b6, b7, small = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.iqlhip_posterior_choice_workspace_bytes(500, 10 ** 6, 100, C.byref(b6)) == 0
    assert lib.iqlhip_posterior_choice_workspace_bytes(500, 10 ** 7, 100, C.byref(b7)) == 0
    assert b6.value == b7.value
    # O(chunk): a fraction of the 200 MB an uint16 index matrix of 1M x 100 would take
    assert 0 < b6.value <= 16 << 20
    assert lib.iqlhip_posterior_choice_workspace_bytes(500, 10, 100, C.byref(small)) == 0
    assert 0 < small.value < b6.value
    for S, N, n in ((1, 10, 1), (2401, 10, 1), (500, 0, 1), (500, 10, 0), (500, 10, 1025)):
        assert lib.iqlhip_posterior_choice_workspace_bytes(S, N, n, C.byref(small)) == _lib.ERR_INVALID
    assert lib.iqlhip_posterior_choice_workspace_bytes(500, 10, 1, None) == _lib.ERR_INVALID


def test_invalid_arguments_refused_without_a_gpu(lib):
    """Every refusal below happens before the first HIP call: the pointers are never read."""
    from iqlpref_amd import _lib
    p = C.c_void_p(4096)  # (16-byte aligned, never dereferenced)
    null = C.c_void_p(0)

    def call(S=500, N=10, n=3, mode=0, state=p, preds=p, out=p, ws=p, ws_bytes=1 << 20):
        return lib.iqlhip_posterior_choice(state, preds, S, N, n, mode, out, null, ws, ws_bytes, null)

    for kw in (dict(S=1), dict(S=0), dict(S=2401), dict(n=0), dict(n=1025), dict(N=0), dict(N=-3),
               dict(mode=2), dict(mode=-1), dict(state=null), dict(preds=null), dict(out=null), dict(ws=null),
               dict(ws=C.c_void_p(4100)), dict(ws_bytes=0), dict(ws_bytes=100)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert lib.iqlhip_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(S=1))


# --------------------------------------------------------------------------- #
# Python surface
# --------------------------------------------------------------------------- #
def test_train_config_matches_reference(golden):
    import iqlpref_amd
    from iqlpref_amd import custom_offline_br as br
    assert iqlpref_amd.custom_offline_br is br
    cfg = br.TrainConfig()
    assert sorted(vars(cfg)) == list(golden["config/fields"])
    for k, v in vars(cfg).items():
        if k == "name":
            assert v.startswith("iql-br-D4RL/pen/human-v2-") and len(v) == len("iql-br-D4RL/pen/human-v2-") + 8
            continue
        want = golden[f"config/default/{k}"]
        assert ("None" if v is None else v) == want.item(), k
    assert not hasattr(cfg, "ckpt_path")  # bref sets it under use_optim_prior only
    opt = br.TrainConfig(use_optim_prior=True, reward_model_path="/m", mapper_num_iters=7, checkpoints_path="/c")
    assert opt.saved_dir == str(golden["config/optim/saved_dir"])
    assert opt.ckpt_path == str(golden["config/optim/ckpt_path"])
    assert os.path.dirname(opt.checkpoints_path) == str(golden["config/optim/checkpoints_dir"])
    assert br.TrainConfig(reward_model_path="/m").saved_dir == str(golden["config/std/saved_dir"])


class _NoPredictions:
    def predictions(self, obs_act):
        raise AssertionError("no prediction may be asked for")

    map_predictions = predictions


def test_errors_come_before_any_work():
    from iqlpref_amd import custom_offline_br as br
    dataset = cte.MinariDataset(11, (5, 6))
    state = np.random.get_state()
    for rtype in (1, 2):
        with pytest.raises(ValueError, match="n_samples"):
            br.qlearning_dataset(dataset, _NoPredictions(), rtype, None)
    one_step = cte.MinariDataset(11, (5, 1, 6))
    for rtype in (0, 1, 2, 3):
        with pytest.raises(ValueError, match="one step"):
            br.qlearning_dataset(one_step, _NoPredictions(), rtype, 4)

    class OneNet:
        def predictions(self, obs_act):
            import torch
            return torch.zeros((1, len(obs_act)))

    for rtype in (0, 1, 2, 9):
        with pytest.raises(ValueError, match="fewer than 2"):
            br.qlearning_dataset(dataset, OneNet(), rtype, 4)

    class NoMap:
        predictions = _NoPredictions.predictions

    with pytest.raises(NotImplementedError, match="find_map"):
        br.qlearning_dataset(dataset, NoMap(), 3)
    with pytest.raises(NotImplementedError, match="find_map"):
        br.train(br.TrainConfig(reward_type=3), dataset, None)
    st = np.random.get_state()
    assert st[2] == state[2] and (st[1] == state[1]).all()  # nothing drew


def test_posterior_choice_envelope_is_checked_in_python():
    import torch
    from iqlpref_amd import custom_offline_br as br
    with pytest.raises(ValueError):
        br.posterior_choice(torch.zeros((1, 4)), 1)
    with pytest.raises(ValueError):
        br.posterior_choice(torch.zeros((2401, 4)), 1)
    with pytest.raises(ValueError):
        br.posterior_choice(torch.zeros(4), 1)


def test_from_saved_dir_reads_the_assumed_layout(tmp_path, monkeypatch):
    """chain_*/sampled_weights/sampled_weights_0000000 under saved_dir, chains in sorted order; an empty
    directory is a FileNotFoundError."""
    import torch
    from iqlpref_amd import _lib
    from iqlpref_amd import custom_offline_br as br
    sets = br_env.posterior_layers(40, 5, 3, 2)
    for chain, part in (("chain_1", sets[3:]), ("chain_0", sets[:3])):
        d = tmp_path / "sampling_std" / chain / "sampled_weights"
        d.mkdir(parents=True)
        torch.save({"sampled_weights": [[torch.from_numpy(a) for a in w] for w in part]},
                   str(d / "sampled_weights_0000000"))
    monkeypatch.setattr(_lib, "require_gpu", lambda device: torch.device("cpu"))  # (only the upload is under test)
    cfg = br.TrainConfig(reward_model_path=str(tmp_path))
    net = br.PosteriorRewardNet.from_saved_dir(cfg.saved_dir)
    assert net.n_posterior == 5 and net.map_set is None
    for (ws, bs), w in zip(net.sets, sets):
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(ws, w[0::2]))
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(bs, w[1::2]))
    with pytest.raises(FileNotFoundError):
        br.PosteriorRewardNet.from_saved_dir(str(tmp_path / "sampling_optim"))
    with pytest.raises(ValueError):
        br.PosteriorRewardNet(sets, transfer_fn="gelu")


# --------------------------------------------------------------------------- #
# "N choice() calls are one randint stream", against the reference's own output
# --------------------------------------------------------------------------- #
def _cases(golden, prefix):
    return sorted({k.split("/")[1] for k in golden if k.startswith(prefix + "/")})


def test_fixture_covers_what_it_must(golden):
    cases = _cases(golden, "sampler")
    S = {int(c.split("_")[0][1:]) for c in cases}
    n = {int(c.split("_")[1][1:]) for c in cases}
    assert 64 in S and (65 in S or 129 in S)  # no rejection / nearly half the words rejected
    assert 1 in n and any(v > 1 and v % 2 for v in n) and any(v % 2 == 0 for v in n)
    assert {c.split("_")[0] for c in _cases(golden, "dataset")} >= {"type0", "type1", "type2", "type3", "type7"}


def test_restatement_reproduces_reference_sampler(golden):
    for case in _cases(golden, "sampler"):
        S, n = (int(x[1:]) for x in case.split("_"))
        g = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"sampler/{case}/")}
        np.random.seed(int(g["seed"]))
        samples, idx = br_env.posterior_sampler(golden[f"preds/{S}"], n)
        assert np.array_equal(idx, g["idx"]), case
        assert samples.tobytes() == g["samples"].reshape(samples.shape).tobytes(), case
        st = np.random.get_state()
        assert np.array_equal(st[1], g["np_key"]) and st[2] == g["np_pos"], case


def test_restatement_reproduces_reference_dataset(golden):
    for case in _cases(golden, "dataset"):
        rtype, n = case.split("_")
        rtype, n = int(rtype[4:]), (None if n == "nNone" else int(n[1:]))
        g = {k.split("/", 2)[2]: v for k, v in golden.items() if k.startswith(f"dataset/{case}/")}
        np.random.seed(int(g["seed"]))
        before = np.random.get_state()
        rewards = br_env.relabel(golden["preds/65"], golden["map_preds"], rtype, n)
        assert rewards.dtype == g["rewards"].dtype == np.float32
        assert rewards.tobytes() == g["rewards"].tobytes(), case
        st = np.random.get_state()
        assert np.array_equal(st[1], g["np_key"]) and st[2] == g["np_pos"], case
        if rtype == 3:
            assert st[2] == before[2] and np.array_equal(st[1], before[1])
    # an out-of-range type is type 0
    assert np.array_equal(br_env.relabel(golden["preds/65"], None, 7, rng=np.random.RandomState(17)),
                          golden["dataset/type7_nNone/rewards"])
    np.random.seed(17)
    assert np.array_equal(br_env.relabel(golden["preds/65"], None, 0), golden["dataset/type7_nNone/rewards"])


def test_fixture_predictions_are_the_stand_in_networks(golden):
    """The stored [S, N] matrices are a function of the stored seeds (no code is stored)."""
    dataset = cte.MinariDataset(int(golden["data_seed"]), tuple(golden["lengths"]))
    env = dataset.recover_environment()
    sets = br_env.posterior_layers(int(golden["post_seed"]), 65, env.S, env.A, int(golden["hidden"]))
    got = br_env.predictions_of(sets, dataset)
    np.testing.assert_allclose(got, golden["preds/65"], rtol=0, atol=1e-6)
