#!/usr/bin/env python3
"""Golden trajectories of the reference at batch sizes that are no multiple of 16.

    python tests/golden/make_anybatch_fixture.py [--ref /root/reference] [--only NAME,...]

Run where the reference is (it never travels to the GPU box).  The reference's own offline/iql.py is driven by
make_fixtures.run_trajectory on seeded synthetic inputs; arrays only are written, in the formats
tests/helpers.load_traj reads (full parameter sets for width 64, strided summaries beyond: the ``regen_seed`` form
of make_fixtures.big_regen where helpers.regen_inputs can rebuild the inputs).  The shapes are the smallest at
which a row mask can go wrong: see CASES.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden import make_fixtures as mf  # noqa: E402
from tests.golden.make_fixtures import import_reference, run_trajectory, save  # noqa: E402

ANTMAZE = dict(beta=10.0, iql_tau=0.9, discount=0.99, tau=0.005, reward_kind="sparse")
CASES = {
    # one full slab plus one real row; recorded dropout masks with batch % 4 != 0; pen shapes
    "traj_b17_pen_drop": dict(s_dim=45, a_dim=24, hidden=64, n_hidden=2, batch=17, n_rows=500, k_steps=6, seed=62,
                              beta=3.0, iql_tau=0.8, discount=0.99, tau=0.005, deterministic=False, dropout=0.1,
                              max_steps=50, reward_kind="normal"),
    # six slabs plus four rows
    "traj_b100_antmaze": dict(s_dim=29, a_dim=8, hidden=64, n_hidden=2, batch=100, n_rows=1000, k_steps=8, seed=63,
                              deterministic=False, dropout=None, max_steps=1000, **ANTMAZE),
    # the general layer-wise step: three hidden layers of a width that is no multiple of 32 (written by
    # summarised(): three hidden layers are not what helpers.regen_inputs rebuilds)
    "traj_b50_deep3_w96": dict(s_dim=29, a_dim=8, hidden=96, n_hidden=3, batch=50, n_rows=400, k_steps=6, seed=66,
                               deterministic=False, dropout=None, max_steps=1000, **ANTMAZE),
}
# strided summaries, inputs rebuilt from the seed (make_fixtures.big_regen): the widths whose full parameter sets
# would make a large file
BIG_CASES = {
    # less than one 16-row slab; halfcheetah shapes, deterministic policy
    "traj_b7_cheetah_det": dict(s_dim=17, a_dim=6, hidden=128, batch=7, n_rows=700, k_steps=6, seed=61,
                                beta=3.0, iql_tau=0.7, discount=0.99, tau=0.005, deterministic=True, dropout=None,
                                max_steps=100, reward_kind="normal"),
    # the H = 256 instantiations
    "traj_b250_h256": dict(s_dim=29, a_dim=8, hidden=256, batch=250, n_rows=1024, k_steps=6, seed=64,
                           deterministic=False, dropout=None, max_steps=1_000_000, **ANTMAZE),
    # two parts per backward work-group, late GEMM operands, k_update's long-batch path
    # (seed: of 65..76 the one whose fp32 trajectory stays farthest from a ReLU / advantage kink by the oracle's own
    # margin, 1.2e-7, among those at which the oracle alone stays inside the "all but x % of entries" caps of the GPU
    # test against the reference's arrays -- tests/test_anybatch_host.py::test_oracle_alone_stays_inside_the_gpu_caps.
    # At 65 and 76 a value sits exactly ON a kink, margin 0.0, where relu'(z) is whatever the summation order of an
    # implementation makes of it; at 75 and 68 the oracle's own bf16 Adam moments leave the reference's in 2.7 % /
    # 0.17 % of a tensor's entries, where the cap is 0.5 %.)
    "traj_b1000_h256": dict(s_dim=29, a_dim=8, hidden=256, batch=1000, n_rows=4096, k_steps=4, seed=67,
                            deterministic=False, dropout=None, max_steps=1_000_000, **ANTMAZE),
}


def summarised(full):
    """Initial parameters and data whole (helpers.load_traj reads them from the file), every later tensor of more
    than 2048 elements as make_fixtures.big_summary keeps it: every 37th element and two sums."""
    keep = {}
    for k, v in full.items():
        if k.startswith(("step1/", "final/")) and v.size > 2048:
            keep[k + "#stride37"] = v.reshape(-1)[::37].copy()
            keep[k + "#sum"] = np.asarray(v.astype(np.float64).sum())
            keep[k + "#abssum"] = np.asarray(np.abs(v.astype(np.float64)).sum())
        else:
            keep[k] = v
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default=None, help="comma-separated case names")
    args = ap.parse_args()
    torch.set_num_threads(1)  # fixed summation order for the captured vectors
    ref = import_reference(args.ref)
    only = set(args.only.split(",")) if args.only else None
    for name, cfg in CASES.items():
        if only is None or name in only:
            for fp32 in (True, False):
                full = run_trajectory(ref, fp32=fp32, **cfg)
                save(f"{name}_{'fp32' if fp32 else 'bf16'}.npz", summarised(full) if cfg["n_hidden"] > 2 else full)
    mf.BIG.update(BIG_CASES)  # big_regen looks its case up by name
    for name in BIG_CASES:
        if only is None or name in only:
            for fp32 in (True, False):
                save(f"{name}_{'fp32' if fp32 else 'bf16'}.npz", mf.big_regen(ref, name, fp32))


if __name__ == "__main__":
    main()
