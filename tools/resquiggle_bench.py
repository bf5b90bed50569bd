#!/usr/bin/env python3
"""Signal-to-reference alignment cost: rd_resquiggle_raw against rd_basecall_raw_global_q on tools/ctcalign_bench.py's batch -- 64 reads of
4096 samples and 6 reads of 40960 samples, soft head, default geometry (chunk 1024, step 128: assembled float64 rows).  The references
are the reads' own calls (beam width 6) with 12 % substitutions / insertions / deletions.

    python tools/resquiggle_bench.py [--reps 5] [--out results.json]
    python tools/resquiggle_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls of each route: median of --reps with
[min, max].  The new route drops the beam search and adds the event kernel.  In a tree that has no resquiggle route (the parent commit;
RADIAN_BENCH_TREE names its checkout) only rd_basecall_raw_global_q is timed.  With --stats the per-kernel times of a `rocprofv3
--kernel-trace --stats --output-format csv -- python tools/resquiggle_bench.py --reps R --only resquiggle` run are divided by the R + 2
calls the run made: the event kernel (ev_stats_kernel), the alignment's kernels (ca_*) and everything else."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import batch, timed   # noqa: E402  (also puts the package -- or RADIAN_BENCH_TREE's -- on the path)


def mutate(labels, rate, rng):
    out = []
    for c in labels:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(int((int(c) + 1 + rng.integers(0, 3)) % 4) if u < 2 * rate / 3 else int(c))
        if rng.random() < rate / 3:
            out.append(int(rng.integers(0, 4)))
    return np.array(out, dtype=np.uint8)


def run(reps, seed, only):
    from radian_amd import Backend, weights
    flat = weights.synthetic_weights(seed=1234)
    flat[-645:-5] *= np.float32(0.05)
    raws = batch(seed)
    res = {"reads": len(raws), "samples": int(sum(len(r) for r in raws)), "head": "soft", "beam_width": 6, "chunk": 1024, "step": 128, "mutation_rate": 0.12}
    with Backend(0) as be:
        be.load_weights(flat)
        calls, _ = be.basecall_raw_global(raws, 4, 1024, 128, 6, False)
        rng = np.random.default_rng(7)
        refs = [mutate(c, 0.12, rng) for c in calls]
        res["labels_called"] = int(sum(len(c) for c in calls))
        res["labels_reference"] = int(sum(len(r) for r in refs))
        res["cells_reference"] = int(sum(len(x) * (2 * len(r) + 1) for x, r in zip(raws, refs)))
        if only in (None, "q"):
            _, res["basecall_raw_global_q"] = timed(lambda: be.basecall_raw_global_q(raws, 4, 1024, 128, 6, False), reps)
        if hasattr(be, "resquiggle_raw") and only in (None, "resquiggle"):
            (aln, ev, rst), res["resquiggle_raw"] = timed(lambda: be.resquiggle_raw(raws, refs, 4, 1024, 128), reps)
            res["align_status"] = {str(k): int((aln.status == k).sum()) for k in range(3)}
            n = np.concatenate(ev.n)
            res["events"] = int(len(n))
            res["dwell_median"] = float(np.median(n)) if len(n) else None
            res["dwell_max"] = int(n.max()) if len(n) else None
            if "basecall_raw_global_q" in res:
                res["resquiggle_over_q"] = res["resquiggle_raw"]["median_ms"] / res["basecall_raw_global_q"]["median_ms"]
    return res


def summarise(path, calls):
    groups = {"ev_stats_kernel": [0.0, 0], "ca_": [0.0, 0], "other": [0.0, 0]}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            key = "ev_stats_kernel" if "ev_stats_kernel" in name else "ca_" if "ca_" in name else "other"
            groups[key][0] += total_ns / calls / 1e6
            groups[key][1] += int(r.get("Calls", 0))
    total = sum(v[0] for v in groups.values())
    return {"calls": calls, "kernel_ms_per_call": {k: v[0] for k, v in groups.items()}, "launches_per_call": {k: v[1] / calls for k, v in groups.items()},
            "event_kernel_share_of_kernel_time": groups["ev_stats_kernel"][0] / total if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--only", default=None, choices=["q", "resquiggle"], help="time one route only (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps + 2) if a.stats else run(a.reps, a.seed, a.only)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
