#!/usr/bin/env python3
"""Times bk_contam_match (the device matcher of `align -H`) on the synthetic input of tools/contam_host_bench.cpp: random reads, every 10th
with 12 adaptor bases at either end, two entries, trims 0.  Wall time of the whole call - staging copies, uploads, kernel, results.

    python tools/contam_device_bench.py [reads = 50000000] [read length = 100] [repeats = 3]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import biokanga_amd as bk  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
    length = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    rng = np.random.default_rng(1)
    a5, a3 = rng.integers(0, 4, 33, dtype=np.uint8), rng.integers(0, 4, 33, dtype=np.uint8)
    bases = rng.integers(0, 4, (n, length), dtype=np.uint8)
    bases[::10, :12] = a5[-12:]
    bases[::10, -12:] = a3[:12]
    lens = np.full(n, length, dtype=np.uint32)
    with bk.ContamMatcher([(a5, 1), (a3, 3)]) as m:
        for k in range(reps):
            t0 = time.perf_counter()
            out = m.match(bases.reshape(-1), None, lens)
            dt = time.perf_counter() - t0
            print(f"run {k}: reads {n} length {length}: {dt:.3f} s, {1e-6 * n / dt:.1f} M reads/s, cuts sum {int(out.sum())}", flush=True)


if __name__ == "__main__":
    main()
