#!/usr/bin/env python3
"""Sigmap at the workload's size: rd_sigmap on simulated reads against a panel of about 10^6 states -- 1000 transcripts of 800 .. 1200
random bases, 8 A in front of each; 32 reads of 1000 bases from the 3' ends of 32 of them (about 3·10^4 samples each), the stand-in pore
model at k = 5 -- in the command's two shapes: the first pass (2048 rows from 32 samples before the fragment against the WHOLE panel,
n_best 8, the scale computed) and the second (the read's last 2048 samples against its candidates from their origins on, the scale given).

    python tools/sigmap_bench.py [--reps 5] [--reads 32] [--only pass1|pass2] [--payload P] [--out results.json]
    python tools/sigmap_bench.py --stats kernel_stats.csv [--reps 5]      # summarise a rocprofv3 run of this tool (--only pass1)

Host clock around whole calls (each ends in a stream synchronise) after two warm-up calls: median of --reps with [min, max].  Reported for
the first pass: useful cells (rows x states of the range) per second, and computed cells per second, the halo's included: a stripe reports
SIGMAP_PAYLOAD ends and computes rows - 1 more states in front of them.  With --stats the per-kernel times of a `rocprofv3 --kernel-trace
--stats --output-format csv -- python tools/sigmap_bench.py --reps R --only pass1` run are divided by its R + 3 calls (one to pick the candidates, two warm-ups, R timed)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctcalign_bench import timed   # noqa: E402  (also puts the package on the path)

TRANSCRIPTS, PAD, FRAGMENT, QUERY = 1000, 8, 1000, 2048
ADAPTER, TAIL, SLACK = 30, 60, 32
KERNELS = ("sm_state_kernel", "signal_scale_kernel", "sm_quant_kernel", "sm_dp_kernel", "sm_select_kernel")


def workload(be, n_reads, seed):
    """-> (flat samples, read offsets, t_lo per read, the SigmapPanel, the target of every read)"""
    from radian_amd.backend import SigmapPanel, SimModel
    from radian_amd.simulate import dwell_cdf, standin_tables
    rng = np.random.default_rng(seed)
    targets = [np.concatenate([np.zeros(PAD, dtype=np.int64), rng.integers(0, 4, int(rng.integers(800, 1201)))]).astype(np.uint8) for _ in range(TRANSCRIPTS)]
    off = np.zeros(TRANSCRIPTS + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in targets])
    truth = rng.choice(TRANSCRIPTS, n_reads, replace=False)
    seqs = [np.concatenate([rng.integers(0, 4, ADAPTER), np.zeros(TAIL, dtype=np.int64), targets[t][PAD:PAD + FRAGMENT]]).astype(np.uint8) for t in truth]
    model = SimModel(5, *standin_tables(5, 7), dwell_cdf(0.2))
    keys = rng.integers(0, 1 << 32, (n_reads, 2), dtype=np.uint64).astype(np.uint32)
    res = be.sim_signal(seqs, model, 400, 2048, 307, 600, 91091, keys)
    roff = np.zeros(n_reads + 1, dtype=np.int64)
    roff[1:] = np.cumsum([len(r) for r in res.raw])
    t_lo = np.array([int(bf[ADAPTER + TAIL]) - SLACK for bf in res.base_first], dtype=np.int64)
    return np.concatenate(res.raw), roff, t_lo, SigmapPanel(np.concatenate(targets), off), truth


def run(reps, n_reads, seed, only, payload=None):
    from radian_amd import Backend, eventalign
    from radian_amd import backend
    SIGMAP_PAYLOAD = payload or backend.SIGMAP_PAYLOAD
    from radian_amd.simulate import standin_tables
    res = {}
    with Backend(0) as be:
        flat, roff, t_lo, panel, truth = workload(be, n_reads, seed)
        model = eventalign.model_tables(5, *standin_tables(5, 7)[:2], 1.0)[0]
        R = int(panel.off[-1])
        lo, n = roff[:-1] + t_lo, roff[1:]
        stripes = -(-R // SIGMAP_PAYLOAD)
        computed = sum(min(R, (i + 1) * SIGMAP_PAYLOAD) - max(0, i * SIGMAP_PAYLOAD - (QUERY - 1)) for i in range(stripes))
        res.update(reads=n_reads, states=R, rows=QUERY, payload=SIGMAP_PAYLOAD, stripes_per_query=stripes, useful_cells=n_reads * QUERY * R,
                   computed_cells=n_reads * QUERY * computed)
        first = be.sigmap(flat, panel, model, lo, lo + QUERY, sc_lo=lo, sc_hi=n, n_best=8)
        if only in (None, "pass1"):
            first, res["pass1"] = timed(lambda: be.sigmap(flat, panel, model, lo, lo + QUERY, sc_lo=lo, sc_hi=n, n_best=8), reps)
            sec = res["pass1"]["median_ms"] / 1e3
            res["useful_cells_per_s"], res["computed_cells_per_s"] = res["useful_cells"] / sec, res["computed_cells"] / sec
        res["status"] = {str(k): int((first.status == k).sum()) for k in range(6)}
        res["top1_is_the_truth"] = int((first.tgt[:, 0] == truth).sum())
        if only in (None, "pass2"):
            within = first.score <= first.score[:, :1] + 2 * QUERY
            q, r = np.nonzero(within & (first.tgt >= 0))
            tg = first.tgt[q, r].astype(np.int64)
            args = dict(m2=first.m2[q], d4=first.d4[q], s_lo=panel.off[tg] + first.org[q, r], s_hi=panel.off[tg + 1], n_best=1)
            second, res["pass2"] = timed(lambda: be.sigmap(flat, panel, model, n[q] - QUERY, n[q], **args), reps)
            res["pass2_queries"] = int(len(q))
            res["pass2_cells"] = int(QUERY * (args["s_hi"] - args["s_lo"]).sum())
            res["pass2_cells_per_s"] = res["pass2_cells"] / (res["pass2"]["median_ms"] / 1e3)
    return res


def summarise(path, calls):
    groups = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            key = next((k for k in KERNELS if k in name), "other")
            g = groups.setdefault(key, [0.0, 0])
            g[0] += total_ns / calls / 1e6
            g[1] += int(r.get("Calls", 0))
    total = sum(v[0] for v in groups.values())
    return {"calls": calls, "kernel_ms_per_call": {k: v[0] for k, v in groups.items()}, "launches_per_call": {k: v[1] / calls for k, v in groups.items()},
            "dp_share_of_kernel_time": groups.get("sm_dp_kernel", [0.0])[0] / total if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--only", default=None, choices=["pass1", "pass2"], help="time one shape only (a profiler run)")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool (--only pass1)")
    ap.add_argument("--payload", type=int, default=None, help="the SM_PAYLOAD of a library built for a measurement (RADIAN_HIP_LIB): only the cell count uses it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.stats, a.reps + 3) if a.stats else run(a.reps, a.reads, a.seed, a.only, a.payload)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
