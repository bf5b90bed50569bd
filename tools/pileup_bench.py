#!/usr/bin/env python3
"""What the pileup adds to an alignment call: Backend.pileup_add (rd_pileup_add) against Backend.align (rd_align_batch) on the same
seeded generated pairs (radian_amd.synthetic.alignment_pairs, tools/align_bench.py's sizes).

    python tools/pileup_bench.py [--pairs 10000] [--median-len 1500] [--reps 3] [--dist spread,hot] [--out results.json]
    python tools/pileup_bench.py --stats kernel_stats.csv [--out summary.json]

Two site distributions: `spread` puts every pair on sites of its own (reads over many transcripts); `hot` puts every pair at site 0 of
one table as long as the longest span (every read on one short transcript: the same-address atomics that DESIGN.md section 22 found
binding for quant).  Times whole calls after one warm-up call of each (a host clock around calls that end in a stream synchronise),
median of --reps with [min, max]; reports the share pileup_add adds to align, the columns piled per second, and that a repeated call
doubles the table (integer counters: the result does not depend on the run).  rd_pileup_read at min_depth 1 is timed beside them.
--stats turns the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its own, one --dist at a time,
--skip-align) into the device time per launch of pileup_kernel next to align_fwd_kernel and align_tb_kernel, and its share of the three."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def stats_summary(path):
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key in ("pileup_kernel", "align_fwd_kernel", "align_tb_kernel", "pileup_flag_kernel", "pileup_gather_kernel"):
                if key in r["Name"]:
                    out[key] = {"calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])), "average_ns": float(r["AverageNs"])}
    three = sum(out.get(k, {}).get("total_ns", 0) for k in ("pileup_kernel", "align_fwd_kernel", "align_tb_kernel"))
    if three:
        out["pileup_kernel_share_of_the_three"] = out.get("pileup_kernel", {}).get("total_ns", 0) / three
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--median-len", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--dist", default="spread,hot")
    ap.add_argument("--skip-align", action="store_true", help="the pileup calls only (a profiled run)")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stats:
        out = stats_summary(a.stats)
    else:
        import numpy as np
        from radian_amd import Backend, synthetic
        _, refs, reads = synthetic.alignment_pairs(a.pairs, seed=a.seed, median_len=a.median_len)
        reads = [q.replace("U", "T") for q in reads]
        cells = sum(len(r) * len(q) for r, q in zip(refs, reads))
        out = {"pairs": a.pairs, "median_len": a.median_len, "cells": cells}
        with Backend(0) as be:
            if not a.skip_align:
                first = be.align(refs, reads)
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = be.align(refs, reads)
                    times.append(time.perf_counter() - t0)
                out["align_call_s"] = {"median": med(times), "min": min(times), "max": max(times)}
                out["align_repeat_identical"] = bool((res.score == first.score).all())
            for dist in a.dist.split(","):
                if dist == "spread":
                    site0 = np.concatenate([[0], np.cumsum([len(r) for r in refs])])[:-1]
                    n_sites = int(sum(len(r) for r in refs))
                else:
                    site0 = np.zeros(len(refs), dtype=np.int64)
                    n_sites = max(len(r) for r in refs)
                be.pileup_open(n_sites)
                warm = be.pileup_add(refs, reads, site0)
                t1 = be.pileup_read()
                times, read_times = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = be.pileup_add(refs, reads, site0)
                    times.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    t2 = be.pileup_read()
                    read_times.append(time.perf_counter() - t0)
                be.pileup_close()
                cols = int(res.n_match.sum() + res.n_sub.sum() + res.n_ins.sum() + res.n_del.sum())
                d = {"n_sites": n_sites, "sites_covered": int(len(t2.site)), "columns_in_intervals": cols,
                     "pileup_add_call_s": {"median": med(times), "min": min(times), "max": max(times)},
                     "pileup_read_call_s": {"median": med(read_times), "min": min(read_times), "max": max(read_times)},
                     "columns_per_s_call_median": cols / med(times),
                     "repeat_identical": bool((res.out == warm.out).all()),
                     "table_after_k_calls_is_k_times_the_first": bool((t2.counts.astype(np.int64) == (a.reps + 1) * t1.counts.astype(np.int64)).all()
                                                                      and (t2.profile == (a.reps + 1) * t1.profile).all()),
                     "status_counts": {int(s): int((res.status == s).sum()) for s in set(res.status.tolist())}}
                if not a.skip_align:
                    d["added_share_of_align_call"] = med(times) / out["align_call_s"]["median"] - 1.0
                out[dist] = d
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
