#!/usr/bin/env python3
"""Training-shard building: the fitting alignment's throughput (rd_fit_batch) and where a label_build job's time goes.

    python tools/label_build_bench.py [--queries 1000000] [--per-ref 40] [--median-ref 1500] [--median-query 30] [--reps 5]
                                      [--job-reads 256] [--job-samples 8192] [--out results.json]

Fit: seeded generated pairs at the shape of real windows -- reference lengths log-normal around --median-ref, --per-ref queries per
reference (a read's windows), query lengths log-normal around --median-query capped at 255, each a substring of its reference with 5 %
substitutions.  Times whole rd_fit_batch calls on the C ABI's own layout (Backend.fit_batch_flat: argument checks, sorting into
launch classes, staging, upload, kernels, copy-back) after one warm-up call: the median of --reps with [min, max], cells = sum m * n,
GCUPS, and the share of the VALU issue bound of the shipped kernel:
  256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 VALU instruction = 1.23e12 wave-instructions/s; one step of fit_kernel<2> -- 64 lanes
  x 2 columns = 128 cells -- is VALU_PER_STEP_B2 vector instructions in the gfx950 ISA
  -> 1.23e12 * 128 / VALU_PER_STEP_B2 cells/s (estimated from the ISA, not measured).
The kernels' own time comes from a `rocprofv3 --kernel-trace --stats` run of this tool with --reps 1 --job-reads 0.

Job: --job-reads seeded Gaussian int16 reads through radian_amd.label_build.run with the synthetic model (head_gain 3), references
built from the reads' own calls (2 % mutated, 50-base flanks); reports the wall-time shares of basecall (existing code: chunk basecall
and normalisation), fit, host selection and shard writing."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_STEP_B2 = 100
ISSUE_BOUND_CUPS = 256 * 4 * 2.4e9 / 2 * 128 / VALU_PER_STEP_B2


def generate(n_queries, per_ref, median_ref, median_query, seed):
    rng = np.random.default_rng(seed)
    n_refs = max(1, n_queries // per_ref)
    rlen = np.maximum(np.round(median_ref * np.exp(0.35 * rng.standard_normal(n_refs))).astype(np.int64), 64)
    roff = np.zeros(n_refs + 1, dtype=np.int64)
    np.cumsum(rlen, out=roff[1:])
    rbuf = rng.integers(0, 4, size=int(roff[-1]), dtype=np.uint8)
    qref = (np.arange(n_queries) % n_refs).astype(np.int32)
    qref.sort()
    qlen = np.clip(np.round(median_query * np.exp(0.5 * rng.standard_normal(n_queries))).astype(np.int64), 1, 255)
    qlen = np.minimum(qlen, rlen[qref])
    lo = (rng.random(n_queries) * (rlen[qref] - qlen + 1)).astype(np.int64)
    qoff = np.zeros(n_queries + 1, dtype=np.int64)
    np.cumsum(qlen, out=qoff[1:])
    src = np.repeat(roff[qref] + lo - qoff[:-1], qlen) + np.arange(int(qoff[-1]))
    qbuf = rbuf[src].copy()
    mut = rng.random(qbuf.size) < 0.05
    qbuf[mut] = rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)
    cells = int((qlen * rlen[qref]).sum())
    return rbuf, roff, qbuf, qoff, qref, cells, qlen, rlen


def fit_part(be, a):
    rbuf, roff, qbuf, qoff, qref, cells, qlen, rlen = generate(a.queries, a.per_ref, a.median_ref, a.median_query, a.seed)
    t0 = time.perf_counter()
    first = be.fit_batch_flat(rbuf, roff, qbuf, qoff, qref)
    warm = time.perf_counter() - t0
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = be.fit_batch_flat(rbuf, roff, qbuf, qoff, qref)
        times.append(time.perf_counter() - t0)
    same = bool((res.score == first.score).all() and (res.counts == first.counts).all() and (res.ref_start == first.ref_start).all())
    ident = res.counts[:, 0] / np.maximum(res.counts.sum(axis=1), 1)
    med = float(np.median(times)) if times else warm
    return {"queries": int(a.queries), "references": int(len(roff) - 1), "query_len_median": float(np.median(qlen)), "ref_len_median": float(np.median(rlen)),
            "cells": cells, "call_s": times, "warmup_call_s": warm, "call_s_median_min_max": [med, min(times or [warm]), max(times or [warm])],
            "gcups_call_median": cells / med / 1e9, "gcups_call_min_max": [cells / max(times or [warm]) / 1e9, cells / min(times or [warm]) / 1e9],
            "repeat_results_identical": same, "identity_median": float(np.median(ident)), "all_ok": bool((res.status == 0).all()),
            "bound": "VALU issue of fit_kernel<2> (estimated from the ISA, not measured)", "valu_per_step_b2": VALU_PER_STEP_B2,
            "bound_gcups": ISSUE_BOUND_CUPS / 1e9, "bound_share_call_median": cells / med / ISSUE_BOUND_CUPS}


def job_part(be, a):
    from radian_amd import label_build, weights
    rng = np.random.default_rng(a.seed + 1)
    w = weights.synthetic_weights(seed=a.seed, head_gain=3)
    be.load_weights(w)
    raws = [np.round(rng.normal(500.0, 80.0, size=a.job_samples)).astype(np.int16) for _ in range(a.job_reads)]
    ids = [f"read-{k:06d}" for k in range(a.job_reads)]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = {}
    for lo in range(0, a.job_reads, 128):
        calls, _ = be.basecall_raw_chunk(raws[lo: lo + 128], 4, 1024, 1024, 6)
        for rid, c in zip(ids[lo: lo + 128], calls):
            body = np.concatenate(c).astype(np.uint8) if sum(len(x) for x in c) else np.zeros(0, np.uint8)
            mut = rng.random(body.size) < 0.02
            body[mut] = rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)
            dec = np.concatenate([rng.integers(0, 4, size=50, dtype=np.uint8), body, rng.integers(0, 4, size=50, dtype=np.uint8)])
            refs[rid] = letters[dec[::-1]].tobytes().decode()
    with tempfile.TemporaryDirectory() as tmp:
        args = label_build.build_parser().parse_args(["-", "-", "-o", os.path.join(tmp, "shards"), "--step-size", str(a.job_step)])
        label_build.run(args, be, list(zip(ids[:8], raws[:8])), refs)   # warm-up: code objects, workspaces
        t0 = time.perf_counter()
        st = label_build.run(args, be, zip(ids, raws), refs)
        wall = time.perf_counter() - t0
    stages = {k: st["t_" + k] for k in ("basecall", "fit", "select", "write")}
    return {"reads": a.job_reads, "samples_per_read": a.job_samples, "step_size": a.job_step, "windows": st["windows"], "kept": st["kept"],
            "fit_cells": st["cells"], "wall_s": wall, "stage_s": stages, "stage_share": {k: v / wall for k, v in stages.items()},
            "label_length_median": float(np.median(st["label_lengths"])) if st["label_lengths"] else None,
            "statuses": {s: st[s] for s in label_build.STATUSES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--per-ref", type=int, default=40)
    ap.add_argument("--median-ref", type=int, default=1500)
    ap.add_argument("--median-query", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--job-reads", type=int, default=256)
    ap.add_argument("--job-samples", type=int, default=8192)
    ap.add_argument("--job-step", type=int, default=128)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from radian_amd import Backend
    out = {}
    with Backend(0) as be:
        if a.queries:
            out["fit"] = fit_part(be, a)
        if a.job_reads:
            out["job"] = job_part(be, a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
