#!/usr/bin/env python3
"""Slab tiles on / off (rd_set_conv_slab) in ONE process: the headline loop of bench.py (64 reads x 4096 samples per step, chunk 1024 / step
512, beam 10, pipelined on two lanes) with the search, and forward-only (rd_forward_reads_resident on one lane), alternating the two
settings.  Labels of both settings are compared first.  Prints the text report and, with --json, one JSON object on the last line.
usage: python tools/conv_slab_ab.py [--steps 40] [--rounds 5] [--lanes 2] [--json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radian_amd import Backend, synthetic, weights

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lanes", type=int, default=2)
ap.add_argument("--decode-group", type=int, default=8)
ap.add_argument("--json", action="store_true")
args = ap.parse_args()

READS, READ_LEN, CHUNK, STEP, BEAM, NB = 64, 4096, 1024, 512, 10, 4
NWIN = READS * ((READ_LEN - CHUNK) // STEP + 2)
be = Backend(0)
be.load_weights(weights.synthetic_weights(seed=1234))
be.set_decode_math("glibc")
batches = []
for b in range(NB):
    reads = synthetic.synthetic_reads(READS, READ_LEN, seed=b)
    norm = np.stack([synthetic.mad_normalise(r, 4) for r in reads]).astype(np.float32)
    d = be.dev_alloc(norm.nbytes)
    be.h2d(d, norm)
    batches.append(d)
read_off = np.arange(READS + 1, dtype=np.int64) * READ_LEN
be.pipe_config(args.decode_group)
be.pipe_set_lanes(args.lanes)
out = [(np.zeros((NWIN, CHUNK), dtype=np.uint8), np.full(NWIN, -1, dtype=np.int32)) for _ in range(2 * args.decode_group)]


def submit(i):
    lab, ln = out[i % len(out)]
    be.pipe_submit_reads(batches[i % NB], read_off, READS, CHUNK, STEP, BEAM, lab, ln)


def with_search(steps):
    for i in range(3):
        submit(i)
    be.pipe_flush()
    be.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        submit(i)
    be.pipe_flush()
    be.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def forward_only(steps):
    for i in range(3):
        be.forward_reads_resident(batches[i % NB], read_off, READS, CHUNK, STEP, "chunk", 0)
    be.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        be.forward_reads_resident(batches[i % NB], read_off, READS, CHUNK, STEP, "chunk", 0)
    be.sync()
    return (time.perf_counter() - t0) / steps * 1e3


labels, tiles = {}, {}
for on in (1, 0):
    be.set_conv_slab(on)
    submit(0)
    be.pipe_flush()
    labels[on] = (out[0][0].copy(), out[0][1].copy())
    tiles[on] = be.conv_slab_tiles()
same = bool(np.array_equal(labels[0][0], labels[1][0]) and np.array_equal(labels[0][1], labels[1][1]))
print(f"slab tiles of one forward: {tiles[1]} with set_conv_slab(1), {tiles[0]} with set_conv_slab(0)")
print("labels identical, slab vs per-tap staging:", same)
t_pre = time.perf_counter()
while time.perf_counter() - t_pre < 0.5:   # the first work on an idle GPU runs slower
    with_search(8)
res = {(k, on): [] for k in ("search", "forward") for on in (0, 1)}
for r in range(args.rounds):
    for on in (0, 1):
        be.set_conv_slab(on)
        res[("search", on)].append(with_search(args.steps))
        res[("forward", on)].append(forward_only(args.steps))
report = {"labels_identical": same, "slab_tiles": tiles[1], "steps": args.steps, "rounds": args.rounds, "lanes": args.lanes}
for k in ("search", "forward"):
    m = {on: float(np.median(res[(k, on)])) for on in (0, 1)}
    for on in (0, 1):
        print(f"{k:8s} conv_slab {on}: median {m[on]:.3f} ms per step   runs " + " ".join(f"{v:.3f}" for v in res[(k, on)]))
        report[f"{k}_ms_slab{on}"] = [round(v, 4) for v in res[(k, on)]]
    print(f"{k:8s} slab / per-tap: {m[1] / m[0]:.4f}  ({(m[0] / m[1] - 1) * 100:+.2f} % samples/s)")
    report[f"{k}_ratio"] = round(m[1] / m[0], 5)
be.close()
if args.json:
    print(json.dumps(report))
