#!/usr/bin/env python3
"""Read-to-transcript mapping at transcriptome scale: where the time of rd_map_index, rd_map_batch and the span fit goes.

    python tools/map_bench.py [--transcripts 20000] [--transcript-len 2500] [--reads 100000] [--read-len 1000] [--error 0.12]
                              [--batch-reads 20000] [--reps 3] [--out results.json]

A seeded generated transcriptome (uniform bases, lengths log-normal around --transcript-len) and reads drawn from random positions of
random transcripts (lengths log-normal around --read-len), with substitutions, insertions and deletions at --error in all.  Reports
  index:  host flattening + upload + minimizer kernel + compaction (seeds) and entries + sort (sort), from rd_map_index's own clocks,
          and the whole call;
  map:    per stage from rd_map_batch's own clocks (seeds, count + scan, fill, sort, segments + chains, best-of-read; asking for them
          synchronises between the stages) summed over the batches, the whole calls without the stage clocks (median of --reps with
          [min, max]), reads/s, anchors, segments, launches;
  fit:    the two pieces of every mapped read through rd_fit_batch (radian_amd.map.map_records minus the mapping call);
  truth:  reads mapped, on the transcript they were drawn from, ambiguous (s2 = s1).
The chain kernel against its issue bound: one wave per segment, CHAIN_VALU_PER_ANCHOR vector instructions per anchor in the gfx950
ISA -> 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction / CHAIN_VALU_PER_ANCHOR anchors/s
(estimated from the ISA, not measured).  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this tool
with --reps 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAIN_VALU_PER_ANCHOR = 68
CHAIN_BOUND_ANCHORS_PER_S = 256 * 4 * 2.4e9 / 2 / CHAIN_VALU_PER_ANCHOR


def generate(a):
    rng = np.random.default_rng(a.seed)
    tlen = np.maximum(np.round(a.transcript_len * np.exp(0.5 * rng.standard_normal(a.transcripts))).astype(np.int64), 200)
    toff = np.zeros(a.transcripts + 1, dtype=np.int64)
    np.cumsum(tlen, out=toff[1:])
    tbuf = rng.integers(0, 4, size=int(toff[-1]), dtype=np.uint8)
    src = rng.integers(0, a.transcripts, size=a.reads)
    want = np.maximum(np.round(a.read_len * np.exp(0.4 * rng.standard_normal(a.reads))).astype(np.int64), 100)
    rlen = np.minimum(want, tlen[src])
    lo = (rng.random(a.reads) * (tlen[src] - rlen + 1)).astype(np.int64)
    # vectorised mutation of the concatenated reads: a third of --error each for deletions, substitutions, insertions
    roff = np.zeros(a.reads + 1, dtype=np.int64)
    np.cumsum(rlen, out=roff[1:])
    flat = tbuf[np.repeat(toff[src] + lo - roff[:-1], rlen) + np.arange(int(roff[-1]))]
    owner = np.repeat(np.arange(a.reads), rlen)
    u = rng.random(flat.size)
    keep = u >= a.error / 3
    sub = keep & (u < 2 * a.error / 3)
    flat = flat.copy()
    flat[sub] = rng.integers(0, 4, size=int(sub.sum()), dtype=np.uint8)
    ins = keep & (rng.random(flat.size) < a.error / 3)
    reps = keep.astype(np.int64) + ins.astype(np.int64)
    out = np.repeat(flat, reps)
    out_owner = np.repeat(owner, reps)
    second = np.flatnonzero(np.diff(np.repeat(np.arange(flat.size), reps), prepend=-1) == 0)
    out[second] = rng.integers(0, 4, size=second.size, dtype=np.uint8)
    new_len = np.bincount(out_owner, minlength=a.reads)
    noff = np.zeros(a.reads + 1, dtype=np.int64)
    np.cumsum(new_len, out=noff[1:])
    return tbuf, toff, out, noff, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--transcript-len", type=int, default=2500)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=1000)
    ap.add_argument("--error", type=float, default=0.12)
    ap.add_argument("--batch-reads", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from radian_amd import Backend, map as rmap
    from radian_amd.backend import MAP_OK
    t0 = time.perf_counter()
    tbuf, toff, rbuf, roff, src = generate(a)
    gen_s = time.perf_counter() - t0
    tr = rmap.Transcripts(tbuf, toff, [f"tx{t}" for t in range(a.transcripts)])
    args = rmap.check_args(rmap.build_parser().parse_args(["reads.fasta", "transcripts.fa", "-o", "read_ref.tsv", "--batch-reads", str(a.batch_reads)]))
    cuts = list(range(0, a.reads, a.batch_reads)) + [a.reads]
    out = {"transcripts": a.transcripts, "transcript_bases": int(toff[-1]), "reads": a.reads, "read_bases": int(roff[-1]), "error": a.error,
           "generate_s": gen_s}
    with Backend(0) as be:
        be.map_index(tbuf, toff, args.k, args.w, args.max_occ)   # warm-up: code objects, buffers
        calls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            st = be.map_index(tbuf, toff, args.k, args.w, args.max_occ)
            calls.append(time.perf_counter() - t0)
        out["index"] = {"entries": st["entries"], "keys": st["keys"], "keys_dropped": st["keys_dropped"], "stage_us": st["stage_us"], "call_s": calls,
                        "call_s_median_min_max": [float(np.median(calls)), min(calls), max(calls)]}

        def map_all(with_stats):
            res = []
            for b0, b1 in zip(cuts, cuts[1:]):
                res.append(be.map_batch_flat(rbuf[roff[b0]: roff[b1]], roff[b0: b1 + 1] - roff[b0], args.min_anchors, args.min_score, args.max_gap,
                                             args.bandwidth, 0, with_stats=with_stats))
            return res
        map_all(False)   # warm-up
        calls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = map_all(False)
            calls.append(time.perf_counter() - t0)
        staged = map_all(True)
        status = np.concatenate([r.status for r in res])
        hits = np.concatenate([r.hits for r in res])
        same = all(np.array_equal(x.status, y.status) and np.array_equal(x.hits, y.hits) for x, y in zip(res, staged))
        stage = {k: sum(r.stats["stage_us"][k] for r in staged) for k in staged[0].stats["stage_us"]}
        anchors = sum(r.stats["anchors"] for r in staged)
        med = float(np.median(calls))
        ok = status == MAP_OK
        out["map"] = {"call_s": calls, "call_s_median_min_max": [med, min(calls), max(calls)], "reads_per_s_median": a.reads / med,
                      "stage_us": stage, "anchors": anchors, "segments": sum(r.stats["segments"] for r in staged),
                      "minimizers": sum(r.stats["minimizers"] for r in staged), "launches": sum(r.stats["launches"] for r in staged),
                      "staged_results_identical": bool(same), "chain_valu_per_anchor": CHAIN_VALU_PER_ANCHOR,
                      "chain_bound_anchors_per_s": CHAIN_BOUND_ANCHORS_PER_S,
                      "chain_bound_share": (anchors / (stage["chain"] * 1e-6)) / CHAIN_BOUND_ANCHORS_PER_S if stage["chain"] else None,
                      "bound": "VALU issue of map_chain_kernel (estimated from the ISA, not measured)"}
        out["truth"] = {"mapped": int(ok.sum()), "on_the_true_transcript": int((ok & (hits[:, 0] == src)).sum()),
                        "ambiguous": int((ok & (hits[:, 1] == hits[:, 2])).sum()), "statuses": np.bincount(status, minlength=5).tolist()}
        # the span fit: the command's own loop on the first batch, minus its mapping call
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        n_fit = min(a.reads, a.batch_reads)
        records = [(f"r{i}", letters[rbuf[roff[i]: roff[i + 1]]].tobytes().decode()) for i in range(n_fit)]
        counters = {}
        rmap.map_records(be, tr, records[:256], args, {})   # warm-up
        t0 = time.perf_counter()
        rows = rmap.map_records(be, tr, records, args, counters)
        out["fit"] = {"reads": n_fit, "wall_s": time.perf_counter() - t0, "map_s": counters["t_map"], "fit_and_host_s": counters["t_fit"],
                      "mapped": sum(1 for r in rows if r["status"] == MAP_OK)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
