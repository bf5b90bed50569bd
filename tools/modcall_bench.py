#!/usr/bin/env python3
"""Per-read modification calls at the workload's size: tools/eventalign_bench.py's batch -- 64 simulated reads of
1000 bases and 4 of 4000, the stand-in pore model at k = 5 -- aligned once (rd_segment, one rd_eventalign_events round, one
rd_eventalign_banded pass on its refit), then ONE rd_modcall with a job at every A of every read (the site's own state, its level moved by
1 z; flank 6) on the banded pass's steps and scale.  Beside it, in the same process, the banded pass itself, for scale.

    python tools/modcall_bench.py [--reps 5] [--flank 6] [--out results.json]
    python tools/modcall_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls: median of --reps with [min, max].  rd_modcall is
timed at the library's entry (`modcall`) and through Backend.modcall (`modcall_from_python`).  Reported: ms per call of these and of the
banded pass, the jobs and their statuses, the rows of all jobs and of the longest, the library call's microseconds per row of the longest
job and nanoseconds per (job, row), the block of the largest read.  With --stats the per-kernel times of a `rocprofv3 --kernel-trace
--stats --output-format csv -- python tools/modcall_bench.py --reps R` run are divided by the calls that put the whole batch through (R + 2 for the
banded pass's own kernels, twice that for rd_modcall's); the set-up's kernels are given as totals of the run."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import timed   # noqa: E402  (also puts the package on the path)
from eventalign_bench import reads   # noqa: E402

KERNELS = ("mc_kernel", "eab_rows_kernel", "eab_dp_kernel", "eab_tb_kernel", "eab_edge_kernel", "ev_stats_kernel", "ea_sums_kernel", "signal_scale_kernel")


def run(reps, seed, flank):
    from radian_amd import Backend, eventalign
    from radian_amd.backend import MC_STATUS_NAMES, SegmentParams, modcall_workspace_bytes
    from radian_amd.segment import window_segmenter
    from radian_amd.simulate import standin_tables
    res = {}
    with Backend(0) as be:
        raws, codes, t_lo = reads(be, seed)
        model, _ = eventalign.model_tables(5, *standin_tables(5, 7)[:2], 1.0)
        windows = [x[t:] for x, t in zip(raws, t_lo)]
        T = [len(x) for x in windows]
        ev = window_segmenter(be.segment, SegmentParams())(windows)
        rows = be.eventalign_events(ev.events, T, codes, model, ev.m2, ev.d4, sample_off=t_lo, skip_pen=96)
        ok = [r for r in range(len(raws)) if int(rows.status[r]) == 0]
        scale = [eventalign.refit(rows.fit_sums[r], rows.m2[r], rows.d4[r]) for r in ok]
        args = ([raws[r] for r in ok], [codes[r] for r in ok])
        kw = dict(t_lo=[t_lo[r] for r in ok], m2=[m for m, _ in scale], d4=[d for _, d in scale])
        fine, res["banded_pass"] = timed(lambda: be.eventalign_banded(*args, [rows.events.start[r] for r in ok], model, **kw), reps)
        good = [j for j in range(len(ok)) if int(fine.status[j]) == 0]
        raws2, codes2 = [args[0][j] for j in good], [args[1][j] for j in good]
        idx = [eventalign.kmer_indices(c, model.k) for c in codes2]
        job_read = [r for r, c in enumerate(codes2) for b in np.flatnonzero(c == 0)]
        alt_first = [int(b) for c in codes2 for b in np.flatnonzero(c == 0)]
        unit = int(round(eventalign.MAD_UNIT))
        alts = [(np.array([model.lvl[idx[r][b]] + unit], np.int32), np.array([model.w[idx[r][b]]], np.uint32), np.array([model.bias[idx[r][b]]], np.int32))
                for r, b in zip(job_read, alt_first)]
        call = lambda: be.modcall(raws2, codes2, [int(fine.m2[j]) for j in good], [int(fine.d4[j]) for j in good], [fine.first_step[j] for j in good],
                                  [fine.last_step[j] for j in good], model, job_read, alt_first, alts, flank=flank)
        mc, res["modcall_from_python"] = timed(call, reps)      # Backend.modcall: packing some 20 000 one-entry arrays is most of it
        from radian_amd.backend import _modcall_args, _p
        keep, head, outs = _modcall_args(raws2, codes2, [int(fine.m2[j]) for j in good], [int(fine.d4[j]) for j in good], [fine.first_step[j] for j in good],
                                         [fine.last_step[j] for j in good], model, job_read, alt_first, alts, flank)
        rc, res["modcall"] = timed(lambda: be._L.rd_modcall(be._h, *head, 0, *[_p(b) for b in outs]), reps)      # the library call alone
        assert rc == 0 and all((b[:len(job_read)] == getattr(mc, f)).all() for b, f in zip(outs, mc.__slots__))
        n_rows = mc.n_rows.astype(np.int64)
        res.update(reads=len(raws2), samples=int(sum(len(x) for x in raws2)), bases=int(sum(len(c) for c in codes2)), jobs=len(job_read), flank=flank,
                   status={MC_STATUS_NAMES[k]: int((mc.status == k).sum()) for k in range(5)}, job_rows=int(n_rows.sum()), longest_job_rows=int(n_rows.max()),
                   median_job_rows=float(np.median(n_rows[mc.status == 0])), share_called=float((mc.llr()[mc.status == 0] > 0).mean()))
        res["modcall_us_per_row_of_the_longest_job"] = res["modcall"]["median_ms"] * 1e3 / res["longest_job_rows"]
        res["modcall_ns_per_job_row"] = res["modcall"]["median_ms"] * 1e6 / res["job_rows"]
        res["modcall_over_banded_pass"] = res["modcall"]["median_ms"] / res["banded_pass"]["median_ms"]
        big = int(np.argmax([len(x) for x in raws2]))
        nj = sum(1 for r in job_read if r == big)
        res["workspace_bytes_largest_read"] = modcall_workspace_bytes(len(raws2[big]), len(codes2[big]), nj, nj)
    return res


def summarise(path, reps):
    """per batch: rd_modcall's kernel (timed twice: through Backend.modcall and at the library's entry) and the banded pass's own kernels,
    which run once per timed or warm-up call.  Every other kernel -- the one-off set-up (detection, one event round) and those the set-up
    shares with the banded pass -- is given as its total over the whole run, with its launches"""
    per_batch, rest = {}, {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ms = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0) / 1e6
            calls = int(r.get("Calls", 0))
            key = next((k for k in KERNELS if k in name), "ear_*" if "ear_" in name else "sg_*" if "sg_" in name else "other")
            if key == "mc_kernel" or key.startswith("eab_"):
                n = (2 if key == "mc_kernel" else 1) * (reps + 2)
                g = per_batch.setdefault(key, [0.0, 0.0])
                g[0] += total_ms / n
                g[1] += calls / n
            else:
                g = rest.setdefault(key, [0.0, 0])
                g[0] += total_ms
                g[1] += calls
    return {"kernel_ms_per_batch": {k: v[0] for k, v in per_batch.items()}, "launches_per_batch": {k: v[1] for k, v in per_batch.items()},
            "other_kernels_total_ms_of_the_run": {k: v[0] for k, v in rest.items()}, "other_kernels_launches_of_the_run": {k: v[1] for k, v in rest.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--flank", type=int, default=6)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps) if a.stats else run(a.reps, a.seed, a.flank)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
