"""Construction and release of the native trainers and groups (csrc/api.hip: iqlhip_trainer_create,
iqlhip_group_create / _destroy, attach / detach), on the tuned and on the general step: what the library refuses
leaves every handle usable, and groups that come and go leak nothing and hand their members back intact.  The
refusals go through ctypes straight on the handles -- ``multi.py`` turns most of them down before the library
sees them.  Everything is compared bit for bit against untouched twins from the same seeds.  -m gpu."""
import ctypes as C
import functools
import gc

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
STATE = ("_params", "_target", "_exp_avg", "_exp_avg_sq")
TUNED, GENERAL = "traj_antmaze", "traj_deep3_w96"
MODE = "bf16"


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return gpu_helpers


@functools.lru_cache(maxsize=None)
def _traj(name):
    _, hyper, data, nets = helpers.load_traj(name, MODE)
    return hyper, data, nets


def _trainers(gh, name, seeds):
    hyper, _, nets = _traj(name)
    trs = [gh.make_trainer(hyper, nets, MODE, seed=s) for s in seeds]
    for t in trs:
        t._ensure_handle(hyper["batch"])
        assert t.step_kind(hyper["batch"]) == ("tuned" if name == TUNED else "general")
    return trs


def _same_state(a, b, where=""):
    torch.cuda.synchronize()
    for ta, tb in zip(a, b):
        assert ta.total_it == tb.total_it, where
        for name in STATE:
            assert torch.equal(getattr(ta, name), getattr(tb, name)), f"{where}{name}"


def test_refusals_leave_everything_usable(gh):
    """Every iqlhip_group_create / iqlhip_trainer_destroy the library turns down returns IQLHIP_ERR_INVALID with
    a message and touches nothing: afterwards the two groups (K = 2) and the two free trainers step 3 steps to
    the bits of twins that saw no refusal."""
    import iqlpref_amd as ia
    lib = ia._lib.load()
    kinds = ((TUNED, "group"), (GENERAL, "general"))

    def build():
        groups, free = [], []
        for name, mode in kinds:
            trs = _trainers(gh, name, (51, 52, 53))
            grp = ia.SeedGroup(trs[:2], mode=mode)
            grp._ensure_group(_traj(name)[0]["batch"])
            groups.append(grp), free.append(trs[2])
        return groups, free

    def step(groups, free):
        for (name, _), grp, lone in zip(kinds, groups, free):
            hyper, data, _ = _traj(name)
            buf = gh.make_buffer(hyper, data)
            grp.train_steps(buf, 3, hyper["batch"], return_losses=False)
            lone.train_steps(buf, 3, hyper["batch"], return_losses=False)
            torch.cuda.synchronize()

    groups, free = build()

    def refused_group(trainers, n=None):
        arr = (C.c_void_p * max(len(trainers), 1))(*[t._handle.value for t in trainers])
        out = C.c_void_p()
        rc = lib.iqlhip_group_create(C.byref(out), arr, len(trainers) if n is None else n)
        assert rc == ia._lib.ERR_INVALID and not out.value, (rc, out.value)
        assert lib.iqlhip_last_error(), "no message"

    (tuned_grp, general_grp), (tuned_free, general_free) = groups, free
    for grp, lone in zip(groups, free):
        refused_group([lone, grp.trainers[0]])   # a trainer that already belongs to a group
        refused_group([grp.trainers[1], lone])
        refused_group([lone, lone])              # a trainer listed twice
    refused_group([tuned_free, general_free])    # a tuned and a general trainer together
    refused_group([general_free, tuned_free])
    refused_group([tuned_free], n=0)
    refused_group([tuned_free] * 17, n=17)
    refused_group([general_free] * 17, n=17)
    for grp in groups:
        for member in grp.trainers:              # a member is destroyed with (after) its group only
            assert lib.iqlhip_trainer_destroy(member._handle) == ia._lib.ERR_INVALID
            assert lib.iqlhip_last_error(), "no message"

    step(groups, free)
    twin_groups, twin_free = build()
    step(twin_groups, twin_free)
    for (name, _), grp, twin, lone, twin_lone in zip(kinds, groups, twin_groups, free, twin_free):
        _same_state(twin.trainers + [twin_lone], grp.trainers + [lone], f"{name}: ")
        assert all(t.total_it == 3 for t in grp.trainers + [lone])
        assert not torch.equal(grp.trainers[0]._params, grp.trainers[1]._params)
        grp.close(), twin.close()


@pytest.mark.parametrize("name,mode", [(TUNED, "group"), (GENERAL, "general")])
def test_groups_do_not_leak(gh, name, mode):
    """20 x (create a group of 2, 3 steps with graph_unroll = 2, destroy it): the device memory comes back (the
    bound of test_trainer_lifecycle_does_not_leak) and the members stand where 60 steps of one standing group
    put their twins."""
    import iqlpref_amd as ia
    hyper, data, _ = _traj(name)
    B = hyper["batch"]
    buf = gh.make_buffer(hyper, data)
    trs, twins = _trainers(gh, name, (61, 62)), _trainers(gh, name, (61, 62))
    standing = ia.SeedGroup(twins, mode=mode)
    standing.train_steps(buf, 60, B, return_losses=False, graph_unroll=2)
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        grp = ia.SeedGroup(trs, mode=mode)
        grp.train_steps(buf, 3, B, return_losses=False, graph_unroll=2)
        assert grp.launch_counts() == (1, 1)
        grp.close()
        assert all(t._group_owner is None for t in trs)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 64 << 20, f"{(free0 - free1) >> 20} MiB not returned after 20 groups"
    _same_state(twins, trs, f"{name}: ")
    assert all(t.total_it == 60 for t in trs)
    standing.close()
