"""The bits of the BC step (csrc/bc_step.hip) and the AWAC step (csrc/awac_step.hip), pinned: sha256 digests of
everything a step writes, over the smallest shapes of both envelopes.  Test infrastructure, our own code; it drives
the public Python surface only (``minari_bc.BC`` / ``BCGroup``, ``awac.AdvantageWeightedActorCritic`` /
``AWACGroup``), so the same file runs against any revision that has both families.

Per unit -- every case of ``minari_cases.CASES``; every case of ``awac_cases.CASES`` twice, once with the case's
injected eps and once with noise drawn on the device; one three-member group per family at the 17-row case
(different initial parameters, separate buffers and indices per member; AWAC: member 0 injected, the others device
noise) -- the trainer is built with ``keep_grads=True`` and takes ``STEPS`` steps, one call each.  After each step:
the parameter arena, ``exp_avg``, ``exp_avg_sq``, the gradient arena, the target arena (AWAC), the loss tensor,
every tensor of ``weight_copies()`` and, for AWAC, ``last_eps()``.

    python -m tests.slab_digests --record out.json

writes the digests with the library's ``iqlhip_build_tag()`` and the compiler's version line.
tests/golden/slab_digests.json was recorded this way from an export of the commit BEFORE the slab-step core
(``git archive`` into a directory of its own, this file copied in, built with that revision's own
``iqlpref_amd/build.py``): its ``build_tag`` is ``build.source_tag()`` of that export, never of the tree under test.
tests/test_gpu_slab_digests.py recomputes on the current build and compares entry by entry.
"""
import hashlib
import json
import subprocess
import sys

import numpy as np
import torch

from tests import awac_cases as ac
from tests import minari_cases as mc

DEV = "cuda:0"
STEPS = 3
BC_GROUP_CASE, AWAC_GROUP_CASE, MEMBERS = "s17_a6_b17", "s17_a6_b17_h256", 3


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def compiler_line():
    """The ``clang version`` line of ``hipcc --version`` (the first line without one)."""
    import os
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        lines = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError) as e:
        return f"hipcc --version failed: {e}"
    return next((l.strip() for l in lines if "clang version" in l), lines[0].strip() if lines else "")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(tr, loss, out, pre, awac):
    torch.cuda.synchronize()
    out[pre + "params"], out[pre + "exp_avg"], out[pre + "exp_avg_sq"] = sha(tr._params), sha(tr._exp_avg), sha(tr._exp_avg_sq)
    out[pre + "grads"], out[pre + "loss"] = sha(tr._grads), sha(loss)
    if awac:
        out[pre + "target"], out[pre + "last_eps"] = sha(tr._target), sha(tr.last_eps())
    for k, w in tr.weight_copies().items():
        out[pre + "copy." + k] = sha(w)


# --------------------------------------------------------------------------- #
# builders
# --------------------------------------------------------------------------- #
def _bc(S, A, max_action, params=None, seed=0):
    from iqlpref_amd import minari_bc
    torch.manual_seed(seed)
    actor = minari_bc.Actor(S, A, max_action)
    if params is not None:
        actor.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    actor = actor.to(DEV)
    return minari_bc.BC(max_action, actor, torch.optim.Adam(actor.parameters(), lr=mc.LR), DEV, keep_grads=True)


def _awac(S, A, H, lam, params=None, seed=0, gamma=ac.GAMMA):
    from iqlpref_amd import awac
    torch.manual_seed(seed)
    actor, c1, c2 = awac.Actor(S, A, H), awac.Critic(S, A, H), awac.Critic(S, A, H)
    for m, n in ((actor, "actor"), (c1, "critic_1"), (c2, "critic_2")):
        if params is not None:
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params[n].items()})
        m.to(DEV)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=ac.LR)
    tr = awac.AdvantageWeightedActorCritic(actor, adam(actor), c1, adam(c1), c2, adam(c2), gamma=gamma, tau=ac.TAU,
                                           awac_lambda=lam, seed=1000 + seed, keep_grads=True)
    if params is not None:
        with torch.no_grad():
            for m, n in ((tr._target_critic_1, "target_critic_1"), (tr._target_critic_2, "target_critic_2")):
                for k, p in m.named_parameters():
                    p.copy_(torch.from_numpy(params[n][k]))
    return tr


def _member_data(data, k):
    """Member k's own rows: the case's, every column scaled by 1 + k / 8 (poisoned rows stay finite and huge)."""
    return {name: (v * np.float32(1 + k / 8)).astype(np.float32) for name, v in data.items()}


# --------------------------------------------------------------------------- #
# units: name -> {entry: sha256}
# --------------------------------------------------------------------------- #
def bc_unit(case):
    from iqlpref_amd import custom_offline as co
    S, A, B, max_action, params, data, idx, _ = mc.bc_case_inputs(case)
    tr = _bc(S, A, max_action, params)
    buf = co.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_dataset(data)
    idx_t, out = _up(idx[:, :B]), {}
    for t in range(STEPS):
        loss = tr.train_steps(buf, 1, B, indices=idx_t[t:t + 1])
        _state(tr, loss, out, f"step{t + 1}/", False)
    return out


def awac_unit(case, injected):
    from iqlpref_amd import awac
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(case)
    tr = _awac(S, A, H, lam, params)
    buf = awac.ReplayBuffer(S, A, len(data["observations"]), DEV)
    buf.load_d4rl_dataset(data)
    idx_t, eps_t, out = _up(idx[:, :B]), _up(eps), {}
    for t in range(STEPS):
        loss = tr.train_steps(buf, 1, B, indices=idx_t[t:t + 1], eps=eps_t[t:t + 1] if injected else None)
        _state(tr, loss, out, f"step{t + 1}/", True)
    return out


def bc_group_unit():
    from iqlpref_amd import custom_offline as co, minari_bc
    S, A, B, max_action, params, data, idx, _ = mc.bc_case_inputs(BC_GROUP_CASE)
    trs = [_bc(S, A, max_action, params if k == 0 else None, seed=7 + k) for k in range(MEMBERS)]
    bufs = []
    for k in range(MEMBERS):
        bufs.append(co.ReplayBuffer(S, A, len(data["observations"]), DEV))
        bufs[-1].load_dataset(_member_data(data, k))
    idx_t = [_up(np.roll(idx[:, :B], k, axis=1)) for k in range(MEMBERS)]
    group, out = minari_bc.BCGroup(trs), {}
    for t in range(STEPS):
        losses = group.train_steps(bufs, 1, B, indices=[i[t:t + 1] for i in idx_t], return_losses=True)
        for k, (tr, loss) in enumerate(zip(trs, losses)):
            _state(tr, loss, out, f"member{k}/step{t + 1}/", False)
    group.close()
    return out


def awac_group_unit():
    from iqlpref_amd import awac
    S, A, B, H, lam, params, data, idx, eps, _ = ac.case_inputs(AWAC_GROUP_CASE)
    trs = [_awac(S, A, H, lam, params if k == 0 else None, seed=7 + k) for k in range(MEMBERS)]
    bufs = []
    for k in range(MEMBERS):
        bufs.append(awac.ReplayBuffer(S, A, len(data["observations"]), DEV))
        bufs[-1].load_d4rl_dataset(_member_data(data, k))
    idx_t, eps_t = [_up(np.roll(idx[:, :B], k, axis=1)) for k in range(MEMBERS)], _up(eps)
    group, out = awac.AWACGroup(trs), {}
    for t in range(STEPS):
        losses = group.train_steps(bufs, 1, B, indices=[i[t:t + 1] for i in idx_t],
                                   eps=[eps_t[t:t + 1]] + [None] * (MEMBERS - 1), return_losses=True)
        for k, (tr, loss) in enumerate(zip(trs, losses)):
            _state(tr, loss, out, f"member{k}/step{t + 1}/", True)
    group.close()
    return out


UNITS = {f"bc/{c}": (lambda c=c: bc_unit(c)) for c in mc.CASES}
for _c in ac.CASES:
    UNITS[f"awac/{_c}/injected"] = lambda c=_c: awac_unit(c, True)
    UNITS[f"awac/{_c}/device"] = lambda c=_c: awac_unit(c, False)
UNITS[f"bc_group/{BC_GROUP_CASE}"] = bc_group_unit
UNITS[f"awac_group/{AWAC_GROUP_CASE}"] = awac_group_unit


def record():
    from iqlpref_amd import _lib
    return {"build_tag": _lib.build_tag(), "compiler": compiler_line(), "steps": STEPS,
            "digests": {name: unit() for name, unit in UNITS.items()}}


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        raise SystemExit("usage: python -m tests.slab_digests --record out.json")
    rec = record()
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in rec['digests'].values())} digests of {len(rec['digests'])} units at build "
          f"{rec['build_tag']} ({rec['compiler']})")
