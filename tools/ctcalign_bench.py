#!/usr/bin/env python3
"""Forced CTC alignment cost: what rd_basecall_raw_global_q adds to rd_basecall_raw_global on one bench-like batch -- 64 reads of
4096 samples and 6 reads of 40960 samples, beam width 6, default geometry (chunk 1024, step 128: assembled float64 rows).

    python tools/ctcalign_bench.py [--reps 5] [--head soft|plain] [--out results.json]
    python tools/ctcalign_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls of each route: median of --reps with
[min, max].  The batch is generated: Gaussian int16 reads through seeded He-normal weights; `--head soft` scales the last Dense
layer by 0.05 (labelings of about a base every five rows -- more states per row than a trained model's base every ten or so),
`--head plain` leaves the random-weight model's saturated rows (a handful of bases per window).  Cells = sum over reads of
rows x (2 labels + 1).  In a tree that has no fused route (the parent commit) only rd_basecall_raw_global is timed.
With --stats the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ctcalign_bench.py
--reps R` run are divided by the fused calls the run made (R + 2) for the alignment's kernels (ca_*)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("RADIAN_BENCH_TREE") or ROOT)   # another checkout of the package (the parent commit's)


def batch(seed):
    from radian_amd import synthetic
    short = synthetic.synthetic_reads(64, 4096, seed)
    long_ = synthetic.synthetic_reads(6, 40960, seed + 1)
    return [r for r in short] + [r for r in long_]


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def run(reps, head, seed):
    from radian_amd import Backend, weights
    flat = weights.synthetic_weights(seed=1234)
    if head == "soft":
        flat[-645:-5] *= np.float32(0.05)
    raws = batch(seed)
    res = {"reads": len(raws), "samples": int(sum(len(r) for r in raws)), "head": head, "beam_width": 6, "chunk": 1024, "step": 128}
    with Backend(0) as be:
        be.load_weights(flat)
        (labels, _), res["basecall_raw_global"] = timed(lambda: be.basecall_raw_global(raws, 4, 1024, 128, 6, False), reps)
        res["labels"] = int(sum(len(l) for l in labels))
        res["labels_long_read"] = int(max(len(l) for l in labels))
        res["cells"] = int(sum(len(r) * (2 * len(l) + 1) for r, l in zip(raws, labels)))
        if hasattr(be, "basecall_raw_global_q"):
            (labels_q, _, aln), res["basecall_raw_global_q"] = timed(lambda: be.basecall_raw_global_q(raws, 4, 1024, 128, 6, False), reps)
            assert all(np.array_equal(a, b) for a, b in zip(labels, labels_q))
            res["align_status"] = {str(k): int((aln.status == k).sum()) for k in range(3)}
            q = np.concatenate(aln.qual)
            res["qual_median"] = float(np.median(q)) if len(q) else None
            add = res["basecall_raw_global_q"]["median_ms"] - res["basecall_raw_global"]["median_ms"]
            res["added_ms_host_clock"] = add
            res["added_share_of_blocking_route"] = add / res["basecall_raw_global"]["median_ms"]
            res["cells_per_s_host_clock"] = res["cells"] / (add * 1e-3) if add > 0 else None
    return res


def summarise(path, calls):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            if "ca_" in name:
                rows.append({"name": name[:100], "ms_per_call": total_ns / calls / 1e6, "launches_per_call": int(r.get("Calls", 0)) / calls})
    rows.sort(key=lambda t: -t["ms_per_call"])
    return {"fused_calls": calls, "align_kernel_ms_per_call": sum(t["ms_per_call"] for t in rows), "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--head", default="soft", choices=["soft", "plain"])
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps + 2) if a.stats else run(a.reps, a.head, a.seed)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
