#!/usr/bin/env python3
"""Signal-simulation rate: rd_sim_lengths and rd_sim_signal on 10^4 reads of about 3 10^4 samples each (1000 random bases, the stand-in
model of radian_amd.simulate at k = 5: mean dwell 30), and the sample kernel against its derived issue bound.

    python tools/sim_bench.py [--reads 10000] [--bases 1000] [--reps 5] [--out results.json]
    python tools/sim_bench.py --trace kernel_trace.csv [--reads 10000] [--reps 5]      # summarise a rocprofv3 run of this tool

Host clock around whole calls after one warm-up call of each (rd_sim_lengths: bases up, dwell kernel, scan, finish kernel, 8 B per read
down; rd_sim_signal: the same and the sample kernel, then 2 B per sample and 4 B per base down and a host copy into the caller's layout):
median of --reps with [min, max].  The stages inside a call cannot be bracketed from outside a synchronous entry point, so the three
stages' device times come from a kernel trace: with --trace, the durations of a
`rocprofv3 --kernel-trace --output-format csv -- python tools/sim_bench.py --reads N --reps R` run are summed per stage (dwell; scan: the
rocprim kernels; finish; sample) and divided by the calls that ran them; the sample kernel's rate is set against the bound.

The bound: the sample kernel's gfx950 code has 913 vector instructions per thread of 8 samples, 304 of them 32-bit multiplies
(v_mul_lo_u32, v_mul_hi_u32, v_mad_i64_i32).  A SIMD issues a wave64 vector instruction in 2 cycles; taking the multiplies at a quarter
of that rate (8 cycles; an assumption, not a measurement), a wave of 512 samples costs 609 * 2 + 304 * 8 = 3650 cycles, 7.13 cycles per
sample and SIMD: 1024 SIMDs at 2.4 GHz give 3.45 10^11 samples/s.  With every instruction at full rate it is 6.9 10^11."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_THREAD, MUL_PER_THREAD, SAMPLES_PER_THREAD = 913, 304, 8
SIMDS, CLOCK_HZ = 1024, 2.4e9
STAGES = (("dwell", "sim_dwell_kernel"), ("scan", "scan"), ("finish", "sim_finish_kernel"), ("sample", "sim_sample_kernel"))


def issue_bound(mul_cycles=8):
    cycles = (VALU_PER_THREAD - MUL_PER_THREAD) * 2 + MUL_PER_THREAD * mul_cycles          # per wave of 64 threads
    return SIMDS * CLOCK_HZ * 64 * SAMPLES_PER_THREAD / cycles


def inputs(n_reads, n_bases, seed):
    from radian_amd import simulate
    from radian_amd.backend import SimModel
    rng = np.random.default_rng(seed)
    model = SimModel(5, *simulate.standin_tables(5, seed), simulate.dwell_cdf(0.2))
    seqs = list(rng.integers(0, 4, (n_reads, n_bases), dtype=np.uint8))
    keys = rng.integers(0, 1 << 32, (n_reads, 2), dtype=np.uint64).astype(np.uint32)
    return seqs, model, dict(lead=400, lead_level_q10=2048, lead_sd_q10=307, median=600, scale_q10=91091, keys=keys)


def timed(fn, reps):
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def run(n_reads, n_bases, reps, seed):
    from radian_amd import Backend
    seqs, model, kw = inputs(n_reads, n_bases, seed)
    with Backend(0) as be:
        ns, t_len = timed(lambda: be.sim_lengths(seqs, model, **kw), reps)
        res, t_sig = timed(lambda: be.sim_signal(seqs, model, n_samples=ns, **kw), reps)
    samples = int(ns.sum())
    assert sum(len(x) for x in res.raw) == samples and (res.status == 0).all()
    return {"reads": n_reads, "bases": n_reads * n_bases, "samples": samples, "reps": reps, "sim_lengths": t_len, "sim_signal": t_sig,
            "call_msamples_per_s": samples / t_sig["median_ms"] / 1e3, "issue_bound_samples_per_s": issue_bound(),
            "issue_bound_full_rate_multiplies": issue_bound(2)}


def summarise(path, n_reads, n_bases, reps, seed):
    """per stage: device time per call.  Both calls run the first three stages (1 + reps calls each); rd_sim_signal alone runs the last"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    total = {s: [0.0, 0] for s, _ in STAGES}
    for r in rows:
        name = r["Kernel_Name"]
        for s, word in STAGES:
            if word in name:
                total[s][0] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                total[s][1] += 1
                break
    calls = {"dwell": 2 * (reps + 1), "scan": 2 * (reps + 1), "finish": 2 * (reps + 1), "sample": reps + 1}
    out = {"stage_us_per_call": {s: total[s][0] / calls[s] for s, _ in STAGES}, "launches": {s: total[s][1] for s, _ in STAGES}}
    samples = n_reads * (400 + 30 * n_bases)     # (nominal: the run itself prints the exact count)
    rate = samples / (out["stage_us_per_call"]["sample"] * 1e-6) if out["stage_us_per_call"]["sample"] else 0.0
    out["sample_kernel_samples_per_s_nominal"] = rate
    out["share_of_issue_bound"] = rate / issue_bound()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--bases", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2028)
    ap.add_argument("--trace", default=None, help="rocprofv3 kernel_trace.csv of a run of this tool with the same --reads and --reps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarise(a.trace, a.reads, a.bases, a.reps, a.seed) if a.trace else run(a.reads, a.bases, a.reps, a.seed)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
