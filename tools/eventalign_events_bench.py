#!/usr/bin/env python3
"""Eventalign on event rows at the workload's size: tools/eventalign_bench.py's batch -- 64 simulated reads of 1000
bases and 4 of 4000, the stand-in pore model at k = 5 -- through rd_segment plus one rd_eventalign_events round, and, beside it in the same
process, one rd_eventalign round on the same windows.

    python tools/eventalign_events_bench.py [--reps 5] [--only events|samples] [--skip-penalty 96] [--out results.json]
    python tools/eventalign_events_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool (--only events)

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls: median of --reps with [min, max].  Reported:
rd_segment on every window (the window its own scale window, `segment`'s defaults), one rd_eventalign_events round on the detector's scale,
the two together, the round alone for the short reads and for the long reads (call time per row of the longest read: an upper bound of
the DP's row time), rows and rows per base, the share of bases skipped, and rd_eventalign's first round on the same windows with its
sample rows.  With --stats the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/eventalign_events_bench.py --reps R --only events` run are divided by the calls that put the whole batch through: R + 2 for the
detector's kernels, 2 (R + 2) for the alignment's (the round, and the short and the long reads apart)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import timed   # noqa: E402  (also puts the package on the path)
from eventalign_bench import LONG, SHORT, reads   # noqa: E402

EAR_KERNELS = ("ear_row_kernel", "ear_dp_kernel", "ear_tb_kernel", "ear_reduce_kernel", "ea_sums_kernel")


def run(reps, seed, only, pen):
    from radian_amd import Backend, eventalign
    from radian_amd.backend import SegmentParams
    from radian_amd.segment import window_segmenter
    from radian_amd.simulate import standin_tables
    res = {}
    with Backend(0) as be:
        raws, codes, t_lo = reads(be, seed)
        model, _ = eventalign.model_tables(5, *standin_tables(5, 7)[:2], 1.0)
        windows = [x[t:] for x, t in zip(raws, t_lo)]
        T = [len(x) for x in windows]
        res.update(reads=len(raws), samples=int(sum(len(r) for r in raws)), sample_rows=int(sum(T)), bases=int(sum(len(c) for c in codes)), skip_penalty=pen)
        if only in (None, "events"):
            seg = window_segmenter(be.segment, SegmentParams())
            ev, res["segment"] = timed(lambda: seg(windows), reps)
            E = [int(n) for n in ev.n_events]
            res.update(rows=int(sum(E)), rows_per_base=sum(E) / res["bases"], sample_rows_per_row=sum(T) / sum(E))
            align = lambda sel: be.eventalign_events([ev.events[i] for i in sel], [T[i] for i in sel], [codes[i] for i in sel], model,
                                                     [ev.m2[i] for i in sel], [ev.d4[i] for i in sel], sample_off=[t_lo[i] for i in sel], skip_pen=pen)
            first, res["events_round"] = timed(lambda: align(range(len(raws))), reps)
            res["status"] = {str(k): int((first.status == k).sum()) for k in range(6)}
            res["skipped_share"] = float(first.n_skipped.sum()) / res["bases"]
            res["segment_plus_round_ms"] = res["segment"]["median_ms"] + res["events_round"]["median_ms"]
            for name, sel in (("short", range(SHORT[0])), ("long", range(SHORT[0], SHORT[0] + LONG[0]))):
                _, t = timed(lambda sel=sel: align(sel), reps)
                res[name] = dict(t, max_rows=max(E[i] for i in sel), call_us_per_row=t["median_ms"] * 1e3 / max(E[i] for i in sel))
        if only in (None, "samples"):
            first, res["samples_round"] = timed(lambda: be.eventalign(raws, codes, model, t_lo=t_lo), reps)
            res["samples_status"] = {str(k): int((first.status == k).sum()) for k in range(6)}
            if "events_round" in res:
                res["samples_over_segment_plus_round"] = res["samples_round"]["median_ms"] / res["segment_plus_round_ms"]
    return res


def summarise(path, reps):
    groups = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            key = next((k for k in EAR_KERNELS if k in name), "sg_*" if "sg_" in name else "other")
            calls = (2 if key in EAR_KERNELS else 1) * (reps + 2)
            g = groups.setdefault(key, [0.0, 0.0])
            g[0] += total_ns / calls / 1e6
            g[1] += int(r.get("Calls", 0)) / calls
    total = sum(v[0] for k, v in groups.items() if k in EAR_KERNELS)
    return {"kernel_ms_per_batch": {k: v[0] for k, v in groups.items()}, "launches_per_batch": {k: v[1] for k, v in groups.items()},
            "dp_share_of_the_alignment_kernels": groups.get("ear_dp_kernel", [0.0])[0] / total if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--only", default=None, choices=["events", "samples"], help="time one route only (a profiler run)")
    ap.add_argument("--skip-penalty", type=int, default=96)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool (--only events)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps) if a.stats else run(a.reps, a.seed, a.only, a.skip_penalty)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
