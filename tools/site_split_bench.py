#!/usr/bin/env python
"""Two-cluster split cost: whole calls of rd_site_split at the shapes of tools/site_compare_bench.py, beside rd_site_compare on the same
events (it shares the counting pass, the upload, the sort and the segmenting: the natural yardstick) and rd_site_split_host (std::sort
and plain loops on one CPU core), and -- from a profiler run -- each call's kernel time by class.  DESIGN.md section 26.

    python tools/site_split_bench.py [--reps 20] [--host-reps 3] [--out results.json]
    python tools/site_split_bench.py --stats kernel_trace.csv [--reps 20]      # summarise a rocprofv3 run of this tool

Whole calls are host-clock times around the synchronous entry points (each ends in a stream synchronise); two untimed calls first; the
median of --reps with the minimum and the maximum.  The input is site_compare_bench's (seeded; the skewed shapes hold four sites of
100 000 events each).  A site above 2^16 events comes back DEEP from rd_site_split: totals only, its chunks do no search -- so the three
shapes of section 20 measure the split of the shallow sites, and a fourth shape, 1M_20k_skewed_60k, holds four sites of 60 000 events,
which are split.  min_frac_q16 is 6554 (0.1), the command's default.  With --stats the rows of the kernel_trace.csv of a
`rocprofv3 --kernel-trace --output-format csv -- python tools/site_split_bench.py --reps R --only gpu` run are cut into calls at every
ss_pick_kernel launch (one per call under the default budget) and each shape's calls give the median time per call of the sort's kernels,
the item kernel, the pick kernel, the other kernels of sitecmp.hip and the scans (the two prefix scans among them)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, events, sites, skew (shape of the log-normal weight), deep sites, events of a deep site
SHAPES = (("1M_20k_even", 1_000_000, 20_000, 0.0, 0, 0), ("1M_20k_skewed", 1_000_000, 20_000, 1.5, 4, 100_000),
          ("8M_100k_skewed", 8_000_000, 100_000, 1.5, 4, 100_000), ("1M_20k_skewed_60k", 1_000_000, 20_000, 1.5, 4, 60_000))
CLASSES = ("sort", "item_kernel", "pick_kernel", "own_other", "scan", "other")
MIN_FRAC_Q16 = 6554


def events(n_events, n_sites, skew, n_deep, deep, seed):
    """site_compare_bench.events with the deep sites' size a parameter; at the modified half of the sites a third of sample 0 sits 1 z up"""
    rng = np.random.default_rng(seed)
    w = np.exp(skew * rng.standard_normal(n_sites))
    counts = rng.multinomial(n_events - deep * n_deep, w / w.sum())
    counts[rng.choice(n_sites, n_deep, replace=False)] += deep
    site = np.repeat(np.arange(n_sites, dtype=np.uint32), counts)
    cond = rng.integers(0, 2, n_events).astype(np.uint8)
    moved = (site % 2 == 0) & (cond == 0) & (rng.random(n_events) < 1 / 3)
    level = rng.uniform(-1.5, 1.5, n_sites)[site] + 0.3 * rng.standard_normal(n_events) + 1.0 * moved
    value = np.clip(np.rint(level * 1024), -32768, 32767).astype(np.int16)
    p = rng.permutation(n_events)
    return site[p], cond[p], value[p], counts


def timed(fn, reps, warm=2):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def run(reps, host_reps, seed, only):
    from radian_amd import Backend
    from radian_amd.backend import SITE_DEEP, SITE_NONE, SITE_OK, SPLIT_FIELDS, site_split_host
    res = {"reps": reps, "host_reps": host_reps, "min_frac_q16": MIN_FRAC_Q16, "shapes": {}}
    with Backend(0) as be:
        for name, n_events, n_sites, skew, n_deep, deep in SHAPES:
            site, cond, value, counts = events(n_events, n_sites, skew, n_deep, deep, seed)
            b = {"events": n_events, "sites": n_sites, "skew": skew, "deepest_site": int(counts.max()), "median_site": float(np.median(counts))}
            got, b["site_split"] = timed(lambda: be.site_split(site, cond, value, n_sites, MIN_FRAC_Q16), reps)
            b["sites_out"] = int(len(got.status))
            b["status_ok"], b["status_deep"], b["status_none"] = (int((got.status == s).sum()) for s in (SITE_OK, SITE_DEEP, SITE_NONE))
            b["events_in_deep_sites"] = int(got.n[got.status == SITE_DEEP].sum())
            b["mevents_per_s"] = n_events / b["site_split"]["median_ms"] / 1e3
            if only is None:
                cmp_, b["site_compare"] = timed(lambda: be.site_compare(site, cond, value, n_sites), reps)
                b["totals_equal_site_compare"] = all(np.array_equal(getattr(got, f), getattr(cmp_, f)) for f in ("out_site", "n", "sum", "sumsq"))
                b["split_over_compare"] = b["site_split"]["median_ms"] / b["site_compare"]["median_ms"]
                host, b["site_split_host"] = timed(lambda: site_split_host(site, cond, value, n_sites, MIN_FRAC_Q16), host_reps, warm=1)
                b["equal_to_host"] = all(np.array_equal(getattr(got, f), getattr(host, f)) for f in SPLIT_FIELDS)
                b["host_over_gpu"] = b["site_split_host"]["median_ms"] / b["site_split"]["median_ms"]
            res["shapes"][name] = b
    return res


def classify(kernel):
    if "ss_item_kernel" in kernel:
        return "item_kernel"
    if "ss_pick_kernel" in kernel:
        return "pick_kernel"
    if "sc_" in kernel and "_kernel" in kernel and "rocprim" not in kernel:
        return "own_other"
    if "radix" in kernel or "onesweep" in kernel or "sort" in kernel:
        return "sort"
    if "scan" in kernel or "lookback" in kernel:
        return "scan"
    return "other"


def summarise(path, reps):
    """kernel_trace.csv of a `--only gpu` run: per shape, the median over its reps + 2 calls of each class's kernel time per call"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {c: 0.0 for c in CLASSES}
    for r in rows:
        c = classify(r["Kernel_Name"])
        cur[c] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if c == "pick_kernel":
            calls.append(cur)
            cur = {c: 0.0 for c in CLASSES}
    per = reps + 2
    if len(calls) != per * len(SHAPES):
        raise SystemExit(f"{path}: {len(calls)} launches of ss_pick_kernel, expected {per * len(SHAPES)} (--reps must match the profiled run)")
    out = {"calls_per_shape": per, "kernel_us_per_call_median": {}, "share_of_kernel_time": {}}
    for i, (name, *_) in enumerate(SHAPES):
        mine = calls[i * per:(i + 1) * per]
        med = {c: float(np.median([m[c] for m in mine])) for c in CLASSES}
        out["kernel_us_per_call_median"][name] = med
        out["share_of_kernel_time"][name] = {c: med[c] / sum(med.values()) for c in CLASSES}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2028)
    ap.add_argument("--only", default=None, choices=["gpu"], help="skip rd_site_compare and the host twin (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_trace.csv of a `--only gpu` run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps) if a.stats else run(a.reps, a.host_reps, a.seed, a.only)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
