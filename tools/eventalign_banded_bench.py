#!/usr/bin/env python3
"""Banded eventalign at the workload's size: tools/eventalign_bench.py's batch -- 64 simulated reads of 1000 bases and
4 of 4000, the stand-in pore model at k = 5 -- through, in one process: one rd_eventalign round; rd_segment; one rd_eventalign_events round
on the detector's scale; and one rd_eventalign_banded pass on the refit of that round, guided by its event starts.

    python tools/eventalign_banded_bench.py [--reps 5] [--only banded] [--skip-penalty 96] [--out results.json]
    python tools/eventalign_banded_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool (--only banded)

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls: median of --reps with [min, max].  Reported
besides the four times: the banded pass's statuses, the share of reads with n_edge > 0, the share of reads whose every output equals one
rd_eventalign round on the same scale, the banded call's time per row of the longest read, the per-read workspace of both sample-row
routes, and detection + event round + banded pass against the rd_eventalign round.  --only banded leaves the full sample round out of the
timed part (a profiler run).  With --stats the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/eventalign_banded_bench.py --reps R --only banded` run are divided by the R + 2 calls that put the whole batch through."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import timed   # noqa: E402  (also puts the package on the path)
from eventalign_bench import reads   # noqa: E402

EAB_KERNELS = ("eab_rows_kernel", "eab_dp_kernel", "eab_tb_kernel", "eab_edge_kernel", "ev_stats_kernel", "ea_sums_kernel", "signal_scale_kernel")


def same(a, i, b, j):
    if any(int(getattr(a, f)[i]) != int(getattr(b, f)[j]) for f in ("status", "score", "m2", "d4")):
        return False
    if a.fit_sums[i].tolist() != b.fit_sums[j].tolist() or a.first_step[i].tolist() != b.first_step[j].tolist() or a.last_step[i].tolist() != b.last_step[j].tolist():
        return False
    return all(getattr(a.events, f)[i].tolist() == getattr(b.events, f)[j].tolist() for f in ("start", "end", "sum", "sumsq", "min", "max"))


def run(reps, seed, only, pen):
    from radian_amd import Backend, eventalign
    from radian_amd.backend import SegmentParams, eventalign_banded_workspace_bytes, eventalign_workspace_bytes
    from radian_amd.segment import window_segmenter
    from radian_amd.simulate import standin_tables
    res = {}
    with Backend(0) as be:
        raws, codes, t_lo = reads(be, seed)
        model, _ = eventalign.model_tables(5, *standin_tables(5, 7)[:2], 1.0)
        windows = [x[t:] for x, t in zip(raws, t_lo)]
        T = [len(x) for x in windows]
        n = len(raws)
        res.update(reads=n, sample_rows=int(sum(T)), max_rows=int(max(T)), bases=int(sum(len(c) for c in codes)), skip_penalty=pen)
        seg = window_segmenter(be.segment, SegmentParams())
        ev, res["segment"] = timed(lambda: seg(windows), reps)
        rows, res["events_round"] = timed(lambda: be.eventalign_events(ev.events, T, codes, model, ev.m2, ev.d4, sample_off=t_lo, skip_pen=pen), reps)
        ok = [r for r in range(n) if int(rows.status[r]) == 0]
        scale = [eventalign.refit(rows.fit_sums[r], rows.m2[r], rows.d4[r]) for r in ok]
        args = ([raws[r] for r in ok], [codes[r] for r in ok])
        kw = dict(t_lo=[t_lo[r] for r in ok], m2=[m for m, _ in scale], d4=[d for _, d in scale])
        fine, res["banded_pass"] = timed(lambda: be.eventalign_banded(*args, [rows.events.start[r] for r in ok], model, **kw), reps)
        res["banded_status"] = {str(k): int((fine.status == k).sum()) for k in range(7)}
        res["share_with_edge"] = float((fine.n_edge > 0).mean())
        res["banded_call_us_per_row"] = res["banded_pass"]["median_ms"] * 1e3 / max(T)
        big = int(np.argmax(T))
        res["workspace_bytes_longest_read"] = {"banded": eventalign_banded_workspace_bytes(T[big], len(codes[big])),
                                               "full": eventalign_workspace_bytes(T[big], len(codes[big]))}
        res["three_stages_ms"] = res["segment"]["median_ms"] + res["events_round"]["median_ms"] + res["banded_pass"]["median_ms"]
        if only is None:
            full, res["samples_round_same_scale"] = timed(lambda: be.eventalign(*args, model, **kw), reps)
            res["share_equal_to_the_full_round"] = float(np.mean([same(fine, j, full, j) for j in range(len(ok))]))
            _, res["samples_round"] = timed(lambda: be.eventalign(raws, codes, model, t_lo=t_lo), reps)
            res["samples_round_over_three_stages"] = res["samples_round"]["median_ms"] / res["three_stages_ms"]
    return res


def summarise(path, reps):
    groups = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            key = next((k for k in EAB_KERNELS if k in name), "ear_*" if "ear_" in name else "sg_*" if "sg_" in name else "other")
            g = groups.setdefault(key, [0.0, 0.0])
            g[0] += total_ns / (reps + 2) / 1e6
            g[1] += int(r.get("Calls", 0)) / (reps + 2)
    return {"kernel_ms_per_batch": {k: v[0] for k, v in groups.items()}, "launches_per_batch": {k: v[1] for k, v in groups.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--only", default=None, choices=["banded"], help="leave the full sample rounds out (a profiler run)")
    ap.add_argument("--skip-penalty", type=int, default=96)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool (--only banded)")
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
