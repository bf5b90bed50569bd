#!/usr/bin/env python3
"""Read-accuracy evaluation throughput: Backend.align (rd_align_batch) on seeded generated pairs (radian_amd.synthetic.alignment_pairs).

    python tools/align_bench.py [--pairs 10000] [--median-len 1500] [--reps 3] [--out results.json]

Times whole Backend.align calls after one warm-up call of the same pairs: a host clock around a call that ends in a stream
synchronise (upload, forward kernel, traceback kernel, copy-back, host packing).  Reports cells = sum n * m, GCUPS, and the share of
the VALU issue bound of the forward kernel:
  256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 VALU instruction = 1.23e12 wave-instructions/s, one 64-cell step costs
  VALU_PER_STEP wave-instructions (counted in the gfx950 ISA of align_fwd_kernel's inner step: DESIGN.md section 10)
  -> 1.23e12 * 64 / VALU_PER_STEP cells/s (estimated, not measured).
The kernel times alone come from a rocprofv3 --kernel-trace --stats run of this tool (profiles/r07_align_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_STEP = 46
ISSUE_BOUND_CUPS = 256 * 4 * 2.4e9 / 2 * 64 / VALU_PER_STEP
HBM_BOUND_CUPS = 6.29e12 / 0.55   # direction words: ~0.55 B per cell (tile padding included)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--median-len", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from radian_amd import Backend, synthetic
    _, refs, reads = synthetic.alignment_pairs(a.pairs, seed=a.seed, median_len=a.median_len)
    reads = [q.replace("U", "T") for q in reads]
    cells = sum(len(r) * len(q) for r, q in zip(refs, reads))
    with Backend(0) as be:
        t0 = time.perf_counter()
        first = be.align(refs, reads)   # warm-up: code objects, workspace allocation
        warm = time.perf_counter() - t0
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = be.align(refs, reads)
            times.append(time.perf_counter() - t0)
        same = bool((res.score == first.score).all() and (res.counts == first.counts).all())
    best = min(times)
    out = {
        "pairs": a.pairs, "median_len": a.median_len, "cells": cells,
        "call_s": times, "warmup_call_s": warm, "repeat_results_identical": same,
        "gcups_call_best": cells / best / 1e9, "gcups_call_median": cells / sorted(times)[len(times) // 2] / 1e9,
        "bound": "VALU issue of align_fwd_kernel (estimated from the ISA, not measured)",
        "bound_gcups": ISSUE_BOUND_CUPS / 1e9, "hbm_dir_store_bound_gcups": HBM_BOUND_CUPS / 1e9,
        "bound_share_call_best": cells / best / ISSUE_BOUND_CUPS,
        "status_counts": {int(s): int((res.status == s).sum()) for s in set(res.status.tolist())},
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
