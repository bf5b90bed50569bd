#!/usr/bin/env python3
"""Event detection cost: rd_segment on the eventalign benchmark's reads (tools/eventalign_bench.py: 64 simulated reads of 1000 bases and
4 of 4000, about 2.4 million samples) and, as a yardstick for streaming passes over the same samples, rd_polya_segment on the same reads.
The commands' default parameters.

    python tools/segment_bench.py [--reps 5] [--only segment|polya] [--out results.json]
    python tools/segment_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool (--only segment)

Host clock around whole calls (each uploads the samples, ends in a stream synchronise and fetches its results) after two warm-up calls:
median of --reps with [min, max].  The detector's own traffic is 2 B per sample read twice (the peak kernel's tile and halo, the event
kernel) and 1 B of flags written: `detector_gb_per_s` is 5 B per sample over the call's time, to be read beside the chip's HBM rate (8 TB/s
on an MI355X) -- a call of this size is a few hundred microseconds of kernels behind two synchronisations and eight copies, so the
figure says how far from the memory system the CALL is, not the kernels; --stats gives the kernels' own split."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("sg_peak_kernel", "sg_combine_kernel", "sg_start_kernel", "sg_event_kernel", "scan")
HBM_GB_PER_S = 8000.0


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def run(reps, seed, only):
    import eventalign_bench
    from radian_amd import Backend
    from radian_amd.backend import PolyaParams, SegmentParams
    p = SegmentParams()
    res = {"params": dict(zip(SegmentParams.__slots__, p.args())), "reps": reps}
    with Backend(0) as be:
        raws, _, t_lo = eventalign_bench.reads(be, seed)
        wins = [np.ascontiguousarray(x[t:], dtype=np.int16) for x, t in zip(raws, t_lo)]
        n = int(sum(len(x) for x in wins))
        res.update(reads=len(wins), samples=n)
        if only in (None, "segment"):
            got, res["segment"] = timed(lambda: be.segment(wins, p), reps)
            res["events"] = int(got.n_events.sum())
            res["events_per_1000_samples"] = 1000.0 * res["events"] / n
            res["segment_msamples_per_s"] = n / res["segment"]["median_ms"] / 1e3
            res["detector_gb_per_s"] = 5.0 * n / res["segment"]["median_ms"] / 1e6
            res["hbm_gb_per_s"] = HBM_GB_PER_S
        if only in (None, "polya"):
            _, res["polya_segment"] = timed(lambda: be.polya_segment(wins, PolyaParams()), reps)
        if only is None:
            res["segment_over_polya"] = res["segment"]["median_ms"] / res["polya_segment"]["median_ms"]
    return res


def summarise(path, reps):
    """kernel_stats.csv of a `--only segment` run: every kernel's time per call (the run makes reps + 2 calls)"""
    calls = reps + 2
    with open(path) as f:
        rows = list(csv.DictReader(f))
    groups = {k: 0.0 for k in KERNELS + ("other",)}
    for r in rows:
        name = r.get("Name") or r.get("KernelName")
        key = next((k for k in KERNELS if k in name), "other")
        groups[key] += float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0) / calls / 1e3
    total = sum(groups[k] for k in KERNELS)
    return {"calls": calls, "kernel_us_per_call": groups, "share_of_segment_kernel_time": {k: groups[k] / total for k in KERNELS} if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--only", default=None, choices=["segment", "polya"], help="time one of the two only (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps) if a.stats else run(a.reps, a.seed, a.only)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
