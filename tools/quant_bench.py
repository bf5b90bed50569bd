#!/usr/bin/env python3
"""Transcript quantification at run scale: the time of an EM iteration of rd_quant_em, and the candidate stage's share of rd_map_candidates.

    python tools/quant_bench.py [--reads 1000000] [--transcripts 20000] [--iters 100] [--reps 5] [--map-reads 20000] [--uniform] [--out results.json]
    python tools/quant_bench.py --stats kernel_stats.csv [--iters 100] [--calls 7] [--out summary.json]

em:   seeded candidate sets -- candidate counts from 1..8 with about half of the reads single, the first transcript of a read drawn
      from a Zipf-like popularity (hot transcripts exist), the others its neighbours in the index as isoforms are -- through rd_quant_em
      with --iters iterations and tol 0: two warm-up calls, then --reps calls; per call the library's own clock of the iteration loop
      divided by the iterations (median with [min, max]), packed and multi-candidate slots per second, upload / first step / download,
      and equality of the counts with the host twin on a smaller set.  Beside them the derived bounds: the
      streamed bytes of a packed slot against HBM, one scattered 8-byte atomic per multi-candidate slot against the measured rate of
      scattered float atomics (the guide has no figure for 64-bit integer ones), and the division's instruction count against the
      vector issue rate.
map:  tools/map_bench.py's generated set at --map-reads reads: rd_map_candidates per stage from its own clocks and the candidate
      stage's share of the call, rd_map_batch's best-of-read stage beside it.
--stats turns the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its own) into the device time per
iteration of the step kernel, the delta kernel and the copies."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 6.3e12             # achievable, of 8 TB/s peak
SCATTERED_ATOMICS_PER_S = 0.08e12 / 4   # 64 lanes in 64 different rows: 0.08 TB/s of added float bytes, one dword each
VALU_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2   # wave64 instructions per second over the chip at two cycles each (64-bit ones take longer)
STEP_VALU_PER_WAVE = 201             # vector instructions of quant_step_kernel per wave in the gfx950 ISA: 119 and the 82 of the 64-bit division path (counted in the ISA)
STREAM_BYTES_PER_PACKED_SLOT = 4 + 2 + 1 + 1 + 4   # t, w, head, end loaded; the share stored


def generate(n_reads, n_tx, seed, uniform=False):
    rng = np.random.default_rng(seed)
    n = np.where(rng.random(n_reads) < 0.5, 1, rng.integers(2, 9, size=n_reads))
    pop = np.ones(n_tx) if uniform else 1.0 / (np.arange(n_tx) + 10.0)
    first = rng.choice(n_tx, size=n_reads, p=pop / pop.sum())
    off = np.zeros(n_reads + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    step = rng.integers(1, 40, size=int(off[-1]))
    step[off[:-1]] = 0
    cum = np.cumsum(step)
    t = (np.repeat(first, n) + cum - np.repeat(cum[off[:-1]], n)) % n_tx   # distinct within a read: at most 7 * 39 < n_tx apart
    w = rng.integers(1, 4097, size=int(off[-1])).astype(np.uint16)
    return off, t.astype(np.int32), w


def packed_slots(off):
    n = np.diff(off)
    pos = 0
    for k in n[n > 1].tolist():
        if pos % 64 + k > 64:
            pos = (pos + 63) // 64 * 64
        pos += k
    return (pos + 63) // 64 * 64


def em_leg(a, be):
    from radian_amd.backend import quant_em_host
    off, t, w = generate(a.reads, a.transcripts, a.seed, a.uniform)
    n = np.diff(off)
    multi = int(n[n > 1].sum())
    packed = packed_slots(off)
    small = generate(20000, 500, a.seed + 1)
    same = bool(np.array_equal(be.quant_em(*small, 500, 20, 0).count, quant_em_host(*small, 500, 20, 0).count))
    for _ in range(2):
        be.quant_em(off, t, w, a.transcripts, a.iters, 0)
    per_iter, calls, stages = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = be.quant_em(off, t, w, a.transcripts, a.iters, 0)
        calls.append(time.perf_counter() - t0)
        per_iter.append(res.stats["stage_us"]["iterations"] / max(res.stats["iterations"], 1))
        stages.append(res.stats["stage_us"])
    med = float(np.median(per_iter))
    bounds = {"hbm_stream_us": packed * STREAM_BYTES_PER_PACKED_SLOT / HBM_BYTES_PER_S * 1e6,
              "scattered_atomics_us": multi / SCATTERED_ATOMICS_PER_S * 1e6,
              "valu_issue_us": packed / 64 * STEP_VALU_PER_WAVE / VALU_WAVE_INSTR_PER_S * 1e6}
    return {"reads": a.reads, "transcripts": a.transcripts, "popularity": "uniform" if a.uniform else "zipf-like", "hottest_transcript_slots": int(np.bincount(t).max()),
            "slots": int(off[-1]), "single_reads": int((n == 1).sum()), "multi_slots": multi,
            "packed_slots": packed, "iterations": res.stats["iterations"], "last_delta": res.stats["last_delta"], "lost": res.stats["lost"],
            "us_per_iteration": per_iter, "us_per_iteration_median_min_max": [med, min(per_iter), max(per_iter)],
            "multi_slots_per_s_median": multi / (med * 1e-6), "packed_slots_per_s_median": packed / (med * 1e-6), "call_s": calls,
            "stage_us_last_call": stages[-1], "equals_host_twin_on_20000_reads": same, "bounds_us_per_iteration": bounds,
            "bound": "one scattered 64-bit atomic per multi-candidate slot (rate taken from scattered float atomics: not measured for 64-bit integers); "
                     "the host's 8-byte read per iteration is inside the measured time"}


def map_leg(a, be):
    import map_bench
    g = argparse.Namespace(transcripts=a.transcripts, transcript_len=2500, reads=a.map_reads, read_len=1000, error=0.12, seed=2026)
    tbuf, toff, rbuf, roff, src = map_bench.generate(g)
    reads = [rbuf[roff[i]: roff[i + 1]] for i in range(a.map_reads)]
    be.map_index(tbuf, toff, 14, 8, 500)
    be.map_candidates(reads[:2000])
    calls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = be.map_candidates(reads)
        calls.append(time.perf_counter() - t0)
    staged = be.map_candidates(reads, with_stats=True)
    best = be.map_batch(reads, with_stats=True)
    su = staged.stats["stage_us"]
    return {"reads": a.map_reads, "anchors": staged.stats["anchors"], "segments": staged.stats["segments"], "call_s": calls,
            "call_s_median_min_max": [float(np.median(calls)), min(calls), max(calls)], "stage_us": su,
            "candidate_stage_share_of_the_staged_call": su["candidates"] / max(sum(su.values()), 1),
            "map_batch_best_stage_us": best.stats["stage_us"]["best"], "multi_candidate_reads": int((staged.n_cand > 1).sum()),
            "row0_equals_map_batch": bool(np.array_equal(best.hits[:, [0, 1, 3, 4, 5, 6, 7]], res.cands[:, 0, :7]))}


def stats_summary(path, iters, calls):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = r
    pick = lambda frag: [r for n, r in rows.items() if frag in n]
    out = {}
    for key, frag in (("step", "quant_step_kernel"), ("delta", "quant_delta_kernel"), ("fill", "quant_fill_kernel")):
        for r in pick(frag):
            out[key] = {"calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])), "average_ns": float(r["AverageNs"])}
    out["step_plus_delta_us_per_iteration"] = (out.get("step", {}).get("average_ns", 0) + out.get("delta", {}).get("average_ns", 0)) / 1e3
    out["iterations_per_call"], out["calls"] = iters, calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--map-reads", type=int, default=20000, help="0: skip the mapping leg")
    ap.add_argument("--uniform", action="store_true", help="every transcript equally popular: no hot transcripts (what contention on them costs)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stats:
        out = stats_summary(a.stats, a.iters, a.calls)
    else:
        from radian_amd import Backend
        with Backend(0) as be:
            out = {"em": em_leg(a, be)}
            if a.map_reads:
                out["map"] = map_leg(a, be)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
