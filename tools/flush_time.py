"""Host time of ``_offline_loop.run``'s loss flush, the only per-step Python of the chunked loop: 20,000 steps over
a stub stepper (zero loss tensors on the CPU), K = 1 and K = 8 members, no evaluation, a logger that appends.
No GPU.  ``python tools/flush_time.py [TREE]`` prints one line per K with the seconds of one run; TREE (default:
this checkout) may be a checkout from before the recorders, whose ``run`` takes no ``records``."""
import os
import sys
import time

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
from iqlpref_amd import _offline_loop as ol  # noqa: E402


def once(K: int, n: int = 20000) -> float:
    out = []
    args = ([object()] * K, list(range(K)), lambda active: None, n, n + 1, 2000, lambda d, s: out.append((d, s)),
            [None] * K, lambda group, active, t, m: [torch.zeros(m, 3) for _ in active], lambda k, tr, s: None)
    if hasattr(ol, "BestModelRecords"):
        args += (ol.BestModelRecords([None] * K),)
    t0 = time.perf_counter()
    ol.run(*args)
    dt = time.perf_counter() - t0
    assert len(out) == n * K
    return dt


if __name__ == "__main__":
    once(1, 2000)  # (imports and first calls)
    for K in (1, 8):
        print(f"K={K} {once(K) * 1e3:.1f} ms")
