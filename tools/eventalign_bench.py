#!/usr/bin/env python3
"""Eventalign at the workload's size: rd_eventalign on one batch of simulated reads -- 64 reads of 1000 bases (about 3·10^4 samples each) and
4 reads of 4000 bases (about 1.2·10^5 samples), the stand-in pore model at k = 5 -- and, beside it, rd_resquiggle_raw on the same reads: the
only other way to an event table.

    python tools/eventalign_bench.py [--reps 5] [--only eventalign|resquiggle] [--out results.json]
    python tools/eventalign_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool

The reads come from rd_sim_signal (lead 400, tails of 60 A, fragments of random bases); every window starts 32 samples before the
fragment's true first sample, as --bounds would put it.  Host clock around whole calls (each ends in a stream synchronise) after two
warm-up calls: median of --reps with [min, max].  Reported: the first round (the window's own scale: scale kernel, quantisation, DP,
traceback, events, sums), a rescale round (the host's exact refit of every read plus a call with the scale given), cells per second
(T (L + 2) per read), and the call time per row of a band for the short reads alone and the long reads alone (a workgroup sweeps one read:
the reads of a group run side by side, so this is an upper bound of the DP's row time).  rd_resquiggle_raw runs with synthetic weights, its
references being the same fragments; in a tree without eventalign (the parent commit: point RADIAN_BENCH_TREE at its checkout) only
it is timed.  With --stats the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/eventalign_bench.py --reps R --only eventalign` run are divided by the 3 (R + 2) times the run put the whole batch through (the
first round, the rescale round, and the short and the long reads apart)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import timed   # noqa: E402  (also puts the package -- or RADIAN_BENCH_TREE's -- on the path)

SHORT, LONG = (64, 1000), (4, 4000)
ADAPTER, TAIL, SLACK = 30, 60, 32


def reads(be, seed):
    """-> (raws, fragment codes in pore order, t_lo)"""
    from radian_amd.backend import SimModel
    from radian_amd.simulate import dwell_cdf, standin_tables
    rng = np.random.default_rng(seed)
    seqs, n_frag = [], []
    for count, L in (SHORT, LONG):
        for _ in range(count):
            seqs.append(np.concatenate([rng.integers(0, 4, ADAPTER), np.zeros(TAIL, dtype=np.int64), rng.integers(0, 4, L)]).astype(np.uint8))
            n_frag.append(L)
    model = SimModel(5, *standin_tables(5, 7), dwell_cdf(0.2))
    keys = rng.integers(0, 1 << 32, (len(seqs), 2), dtype=np.uint64).astype(np.uint32)
    res = be.sim_signal(seqs, model, 400, 2048, 307, 600, 91091, keys)
    return res.raw, [s[ADAPTER + TAIL:] for s in seqs], [int(bf[ADAPTER + TAIL]) - SLACK for bf in res.base_first]


def run(reps, seed, only):
    from radian_amd import Backend, weights
    res = {}
    with Backend(0) as be:
        raws, codes, t_lo = reads(be, seed)
        T = [len(r) - lo for r, lo in zip(raws, t_lo)]
        res.update(reads=len(raws), samples=int(sum(len(r) for r in raws)), rows=int(sum(T)), bases=int(sum(len(c) for c in codes)),
                   cells=int(sum(t * (len(c) + 2) for t, c in zip(T, codes))))
        if hasattr(be, "eventalign") and only in (None, "eventalign"):
            from radian_amd import eventalign
            from radian_amd.simulate import standin_tables
            model, _ = eventalign.model_tables(5, *standin_tables(5, 7)[:2], 1.0)
            first, res["round0"] = timed(lambda: be.eventalign(raws, codes, model, t_lo=t_lo), reps)
            res["status"] = {str(k): int((first.status == k).sum()) for k in range(6)}
            res["cells_per_s"] = res["cells"] / (res["round0"]["median_ms"] / 1e3)

            def rescale():
                fit = [eventalign.refit(first.fit_sums[r], first.m2[r], first.d4[r]) for r in range(len(raws))]
                return be.eventalign(raws, codes, model, t_lo=t_lo, m2=[f[0] for f in fit], d4=[f[1] for f in fit])
            second, res["rescale_round"] = timed(rescale, reps)
            res["fitted_m2"] = [int(second.m2.min()), int(second.m2.max())]
            res["fitted_d4"] = [int(second.d4.min()), int(second.d4.max())]
            for name, sel in (("short", range(SHORT[0])), ("long", range(SHORT[0], SHORT[0] + LONG[0]))):
                sub = lambda a, sel=sel: [a[i] for i in sel]
                _, t = timed(lambda: be.eventalign(sub(raws), sub(codes), model, t_lo=sub(t_lo)), reps)
                bands = (max(len(codes[i]) for i in sel) + 2 + 4095) // 4096
                cells = sum(T[i] * (len(codes[i]) + 2) for i in sel)
                res[name] = dict(t, cells=int(cells), cells_per_s=cells / (t["median_ms"] / 1e3), max_rows=int(max(T[i] for i in sel)), bands=bands,
                                 call_us_per_band_row=t["median_ms"] * 1e3 / (bands * max(T[i] for i in sel)))
        if only in (None, "resquiggle"):
            flat = weights.synthetic_weights(seed=1234)
            flat[-645:-5] *= np.float32(0.05)
            be.load_weights(flat)
            (aln, ev, rst), res["resquiggle_raw"] = timed(lambda: be.resquiggle_raw(raws, codes, 4, 1024, 128), reps)
            res["resquiggle_status"] = {str(k): int((aln.status == k).sum()) for k in range(3)}
            res["resquiggle_cells"] = int(sum(len(r) * (2 * len(c) + 1) for r, c in zip(raws, codes)))
            if "round0" in res:
                res["resquiggle_over_round0"] = res["resquiggle_raw"]["median_ms"] / res["round0"]["median_ms"]
    return res


def summarise(path, calls):
    groups = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            key = next((k for k in ("signal_scale_kernel", "ea_quant_kernel", "ea_dp_kernel", "ea_tb_kernel", "ea_sums_kernel", "ev_stats_kernel") if k in name), "other")
            g = groups.setdefault(key, [0.0, 0])
            g[0] += total_ns / calls / 1e6
            g[1] += int(r.get("Calls", 0))
    total = sum(v[0] for v in groups.values())
    return {"batches": calls, "kernel_ms_per_batch": {k: v[0] for k, v in groups.items()}, "launches_per_batch": {k: v[1] / calls for k, v in groups.items()},
            "dp_share_of_kernel_time": groups.get("ea_dp_kernel", [0.0])[0] / total if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--only", default=None, choices=["eventalign", "resquiggle"], help="time one route only (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool (--only eventalign)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, 3 * (a.reps + 2)) if a.stats else run(a.reps, a.seed, a.only)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
