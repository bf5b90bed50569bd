"""Stage times of radian_amd.lm_build at the scale of a human protein-coding transcriptome.

    python tools/lm_build_bench.py [--records 100000] [--length 2600] [--k 11 12] [--reps 5] [--json-write] [--out FILE]

Input: `records` transcripts of `length` bases each from a seeded order-3 Markov chain (rows Dirichlet(0.3), entries under 0.02 zeroed:
tests/_lm_ref.markov_transcripts' rule, seed 2024), every 1000th base a run of 8 N.  Default 1e5 x 2600 = 2.6e8 bases.  That chain
visits few long contexts (1.5e5 of 4^11); --uniform draws independent uniform bases instead, which visit nearly all of them.

Per k, medians over `reps` warm runs (one discarded run first) of the stages rd_lm_build times itself (host staging, upload, count, marginals
+ table + entropies, download) and the windows per second of the count, and once each: rd_fasta_scan over the
same transcripts as FASTA text (60-column lines), rd_lm_json_write of the table (--json-write), the CPU restatement's count (numpy bincount)
for scale.  One JSON line per k; --out appends them to a file.  (The count that was measured against the shipped one -- one global atomic
per window -- is gone from the library; its figures from this tool are in DESIGN.md 13 and profiles/r10_lm_build_bench.json.)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def transcriptome(records, length, seed=2024, uniform=False):
    """-> codes uint8 [records * length], offsets"""
    rng = np.random.default_rng(seed)
    if uniform:
        codes = rng.integers(0, 4, size=records * length, dtype=np.uint8)
        codes[(np.arange(len(codes)) % 1000) < 8] = 255
        return codes, np.arange(records + 1, dtype=np.int64) * length
    rows = rng.dirichlet([0.3] * 4, size=64)
    rows[rows < 0.02] = 0.0
    rows /= rows.sum(1, keepdims=True)
    cum = np.cumsum(rows, axis=1)
    cum[:, 3] = 2.0
    lab = np.empty((length, records), dtype=np.uint8)
    state = rng.integers(0, 64, size=records)
    for i in range(length):
        b = (rng.random(records, dtype=np.float32)[:, None] >= cum[state]).sum(1)
        lab[i] = b
        state = (state * 4 + b) & 63
    codes = np.ascontiguousarray(lab.T).reshape(-1)
    flat = np.arange(len(codes))
    codes[(flat % 1000) < 8] = 255
    return codes, np.arange(records + 1, dtype=np.int64) * length


def fasta_text(codes, offsets):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for r in range(len(offsets) - 1):
        c = codes[offsets[r]:offsets[r + 1]]
        s = np.where(c < 4, letters[c & 3], ord("N")).astype(np.uint8)
        pad = (-len(s)) % 60
        lines = np.concatenate([s, np.full(pad, ord(" "), dtype=np.uint8)]).reshape(-1, 60)
        lines = np.concatenate([lines, np.full((len(lines), 1), ord("\n"), dtype=np.uint8)], axis=1)
        out.append(b">T%d|G|-|-|N|N|%d|protein_coding|\n" % (r, len(s)))
        out.append(lines.tobytes())
    return b"".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=2600)
    ap.add_argument("--k", type=int, nargs="+", default=[11, 12])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json-write", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the FASTA scan and the CPU restatement")
    ap.add_argument("--uniform", action="store_true", help="independent uniform bases instead of the Markov chain (every context equally likely)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from radian_amd import Backend, _lib, lm
    t = time.time()
    codes, offsets = transcriptome(args.records, args.length, uniform=args.uniform)
    print(f"generated {len(codes)} bases in {time.time() - t:.1f} s", flush=True)
    host = {}
    if not args.no_host:
        text = fasta_text(codes, offsets)
        L = _lib.load()
        buf = np.frombuffer(text, dtype=np.uint8)
        counts = np.zeros(3, dtype=np.int64)
        out_codes, out_off = np.empty(len(codes), dtype=np.uint8), np.zeros(len(offsets), dtype=np.int64)
        t = time.time()
        assert L.rd_fasta_scan(buf.ctypes.data, len(text), 7, b"protein_coding", None, None, counts.ctypes.data) == 0
        assert L.rd_fasta_scan(buf.ctypes.data, len(text), 7, b"protein_coding", out_codes.ctypes.data, out_off.ctypes.data, counts.ctypes.data) == 0
        host["scan_s"] = time.time() - t
        host["fasta_bytes"] = len(text)
        assert np.array_equal(out_codes, codes) and np.array_equal(out_off, offsets)
        del text, buf, out_codes
        print(f"scan (count pass + fill pass): {host['scan_s']:.2f} s for {host['fasta_bytes']} bytes", flush=True)
    with Backend(0) as be:
        for k in args.k:
            res = {"k": k, "input": "uniform" if args.uniform else "markov3", "bases": int(len(codes)), "records": args.records, **host}
            runs = []
            for rep in range(args.reps + 1):
                t = time.time()
                table, st = be.build_lm(codes, offsets, k)
                wall = time.time() - t
                if rep:
                    runs.append({**st["stage_us"], "wall": wall * 1e6})
            med = {key: statistics.median(r[key] for r in runs) / 1e6 for key in runs[0]}
            lo = {key: min(r[key] for r in runs) / 1e6 for key in runs[0]}
            hi = {key: max(r[key] for r in runs) / 1e6 for key in runs[0]}
            res.update({"median_s": med, "count_min_max_s": [lo["count"], hi["count"]], "windows": st["windows"],
                        "count_windows_per_s": st["windows"] / med["count"]})
            print(f"k={k}: count {med['count'] * 1e3:.2f} ms [{lo['count'] * 1e3:.2f}, {hi['count'] * 1e3:.2f}] = "
                  f"{st['windows'] / med['count'] / 1e9:.2f} G windows/s; staging {med['staging']:.3f} s, upload {med['upload']:.3f} s, "
                  f"table {med['table'] * 1e3:.2f} ms, download {med['download']:.3f} s, call {med['wall']:.3f} s", flush=True)
            keep, seen = table, st["contexts_seen"]
            res["contexts_seen"] = seen
            if args.json_write:
                with tempfile.TemporaryDirectory() as d:
                    t = time.time()
                    rows, nbytes = lm.write_json(os.path.join(d, "m.json"), keep, k)
                    res["json_write_s"], res["json_bytes"] = time.time() - t, nbytes
                print(f"k={k} JSON write: {res['json_write_s']:.2f} s, {nbytes} bytes", flush=True)
            if not args.no_host and k == args.k[0]:
                import _lm_ref
                t = time.time()
                C = _lm_ref.counts(codes, offsets, k)
                res["cpu_restatement_count_s"] = time.time() - t
                table2, st2 = be.build_lm(codes, offsets, k, want_counts=True, want_table=False)
                assert np.array_equal(st2["counts"].astype(np.int64), C)
                print(f"k={k} CPU restatement count: {res['cpu_restatement_count_s']:.1f} s (equal counts)", flush=True)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
