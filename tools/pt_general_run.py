"""Throughput of the PT relabel paths: windows/s and fp32 TFLOP/s of iqlhip_pt_relabel_general (and of
the tuned iqlhip_pt_relabel where the shape allows it), full-length windows with true timesteps.

    python tools/pt_general_run.py [out.json]

Flop formula (the work value[:, 0, -1, 0] needs per window of QL transitions, T = 2 QL tokens, all
of them real; multiply-add = 2):
    embed             2 QL (S + A) E
    block < L - 1     2 T E 3E (QKV) + 2 T (T + 1) E (q.k and p.v over the causal prefixes)
                      + 2 T E E (out projection) + 4 T E I (MLP)
    last block        2 T E 2E (keys and values of every token) + 2 E E (one query) + 4 T E (its
                      attention) + 2 E E + 4 E I
    value head        2 E
Both paths are credited with this count.  (The general path also computes the last block's queries
of every token -- 2 T E E more, not credited -- because its QKV GEMM runs over all rows.)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import iqlpref_amd as ia  # noqa: E402
from oracle import relabel_oracle as ro  # noqa: E402

DEV = "cuda:0"


def flops_per_window(S, A, QL, L, E, I):
    T = 2 * QL
    f = 2 * QL * (S + A) * E + 2 * E
    for l in range(L):
        if l < L - 1:
            f += 2 * T * E * 3 * E + 2 * T * (T + 1) * E + 2 * T * E * E + 4 * T * E * I
        else:
            f += 2 * T * E * 2 * E + 2 * E * E + 4 * T * E + 2 * E * E + 4 * E * I
    return f


def run(name, S, A, max_ep, QL, L, E, I, heads, n_win, kernel, reps=3):
    rng = np.random.default_rng(0)
    p = ro.make_pt_params(rng, S, A, max_ep, embd=E, pref=64, inter=I, layers=L)
    m = ia.RewardPT(S, A, max_ep, embd_dim=E, num_heads=heads, intermediate_dim=I, num_layers=L,
                    max_pos=max(1024, 2 * QL))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    m = m.to(DEV)
    n_rows = max(n_win + QL, 10_000)
    obs = torch.randn(n_rows, S, device=DEV)
    act = torch.rand(n_rows, A, device=DEV) * 2 - 1
    starts = torch.from_numpy(rng.integers(0, n_rows - QL, n_win)).to(DEV)
    lens = torch.full((n_win,), QL, dtype=torch.int32, device=DEV)
    t0 = torch.from_numpy(rng.integers(0, max_ep + 1 - QL, n_win).astype(np.int32)).to(DEV)
    call = lambda: m.window_values(obs, act, starts, lens, QL, win_t0=t0, kernel=kernel)
    call()  # warm-up (and the workspace allocation of the general path)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / 1e3)
    t = float(np.median(times))
    fl = flops_per_window(S, A, QL, L, E, I)
    return {"case": name, "kernel": kernel, "S": S, "A": A, "QL": QL, "L": L, "E": E, "I": I, "heads": heads,
            "n_win": n_win, "s": t, "windows_per_s": n_win / t, "gflop_per_window": fl / 1e9,
            "tflops": fl * n_win / t / 1e12}


CASES = [
    # name, S, A, max_ep, QL, L, E, I, heads, n_win, kernels
    ("antmaze", 29, 8, 1000, 100, 1, 64, 256, 4, 200_000, ("tuned", "general")),
    ("antmaze", 29, 8, 1000, 100, 2, 128, 512, 4, 100_000, ("general",)),
    ("antmaze", 29, 8, 1000, 100, 2, 256, 1024, 4, 20_000, ("general",)),
    ("pen", 45, 24, 100, 100, 1, 64, 256, 4, 5_000, ("tuned", "general")),
    ("pen", 45, 24, 100, 100, 2, 128, 512, 4, 5_000, ("general",)),
]

if __name__ == "__main__":
    rows = []
    for name, S, A, max_ep, QL, L, E, I, heads, n_win, kernels in CASES:
        for k in kernels:
            r = run(name, S, A, max_ep, QL, L, E, I, heads, n_win, k)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
