#!/usr/bin/env python3
"""Poly(A) segmentation cost: rd_polya_segment against rd_normalise_reads -- the existing code that sweeps the same bytes five times (two
radix selects and the write) -- on three batches of synthetic tailed reads (radian_amd.synthetic.tail_read): 64 reads of 4096 samples,
6 of 40 960 and 1 of 1 000 000.  The command's default parameters.

    python tools/polya_bench.py [--reps 20] [--out results.json]
    python tools/polya_bench.py --stats kernel_stats.csv [--reps 20]      # summarise a rocprofv3 run of this tool

Host clock around whole calls (each uploads the samples, ends in a stream synchronise and fetches its results: 2 B per sample up for both,
4 B per sample down for the normalisation, 56 B per read for the segmentation) after two warm-up calls of each: median of --reps with
[min, max].  The feature is new, so there is no parent number; rd_normalise_reads is the yardstick.  With --stats the per-kernel times
of a `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/polya_bench.py --reps R --only polya` run are divided by the
3 (R + 2) calls the run made: the three kernels of polya.hip, their shares, and everything else; given the same run's kernel_trace.csv
instead, the median duration of each kernel per batch."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (("64x4096", 64, 4096), ("6x40960", 6, 40960), ("1x1000000", 1, 1000000))
KERNELS = ("pa_scale_kernel", "pa_window_kernel", "pa_segment_kernel")


def batch(n_reads, n_samples, seed):
    from radian_amd import synthetic
    rng = np.random.default_rng(seed)
    tail = max(640, n_samples // 16)
    lead = n_samples // 40
    return [synthetic.tail_read(rng, leader=lead, adapter=lead, tail=tail, body=n_samples - 2 * lead - tail)[0] for _ in range(n_reads)]


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
    from radian_amd import Backend
    from radian_amd.backend import PolyaParams
    p = PolyaParams()
    res = {"params": dict(zip(PolyaParams.__slots__, p.args())), "reps": reps, "batches": {}}
    with Backend(0) as be:
        for name, n, T in BATCHES:
            raws = batch(n, T, seed)
            b = {"reads": n, "samples": n * T, "windows": n * (T // p.win)}
            if only in (None, "polya"):
                got, b["polya_segment"] = timed(lambda: be.polya_segment(raws, p), reps)
                b["status_ok"] = int((got.status == 0).sum())
                b["tail_samples_median"] = float(np.median(got.tail_end - got.tail_start))
                b["polya_msamples_per_s"] = n * T / b["polya_segment"]["median_ms"] / 1e3
            if only in (None, "normalise"):
                _, b["normalise_reads"] = timed(lambda: be.normalise_reads(raws, 4), reps)
            if only is None:
                b["polya_over_normalise"] = b["polya_segment"]["median_ms"] / b["normalise_reads"]["median_ms"]
            res["batches"][name] = b
    return res


def summarise(path, reps):
    """kernel_stats.csv: the three kernels' time per call over all batches; kernel_trace.csv (the same run's): per batch, the median
    duration of each kernel's launches -- the run makes reps + 2 calls per batch, in BATCHES order, one launch of each kernel per call"""
    calls = len(BATCHES) * (reps + 2)
    with open(path) as f:
        rows = list(csv.DictReader(f))
    if rows and "Start_Timestamp" in rows[0]:
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        dur = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
        out = {"calls": calls, "kernel_us_median": {}, "share_of_polya_kernel_time": {}}
        for i, (name, _, _) in enumerate(BATCHES):
            med = {}
            for k in KERNELS:
                if len(dur[k]) != calls:
                    raise SystemExit(f"{path}: {len(dur[k])} launches of {k}, expected {calls} (--reps must match the profiled run)")
                med[k] = float(np.median(dur[k][i * (reps + 2):(i + 1) * (reps + 2)]))
            out["kernel_us_median"][name] = med
            out["share_of_polya_kernel_time"][name] = {k: v / sum(med.values()) for k, v in med.items()}
        return out
    groups = {k: [0.0, 0] for k in KERNELS + ("other",)}
    for r in rows:
        name = r.get("Name") or r.get("KernelName")
        total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
        key = next((k for k in KERNELS if k in name), "other")
        groups[key][0] += total_ns / calls / 1e3
        groups[key][1] += int(r.get("Calls", 0))
    total = sum(groups[k][0] for k in KERNELS)
    return {"calls": calls, "kernel_us_per_call": {k: v[0] for k, v in groups.items()}, "launches_per_call": {k: v[1] / calls for k, v in groups.items()},
            "share_of_polya_kernel_time": {k: groups[k][0] / total for k in KERNELS} if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2027)
    ap.add_argument("--only", default=None, choices=["polya", "normalise"], help="time one of the two only (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv (or kernel_trace.csv) of a run of this tool")
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
