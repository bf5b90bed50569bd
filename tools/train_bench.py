#!/usr/bin/env python3
"""Training cost: rd_train_step_resident (train.hip) at batch 32 and 256 -- forward, CTC gradient, backward, Adam and the image
refresh of one step -- on windows already in device memory, labels of L = 60, every row counted.

    python tools/train_bench.py [--batches 32,256] [--steps 20] [--out results.json]
    python tools/train_bench.py --stats kernel_stats.csv [--batches 32] [--steps 20]     # summarise a rocprofv3 run of this tool

Host clock around --steps calls (each ends in a stream synchronise) after two warm-up steps.  FLOPs per step count the matrix
products of the graph: 2 * rows * (K * N) for each conv / Dense in the forward, twice that in the backward (data and weight
gradients; block 0's one-channel conv and the 1x1 matching conv are left out, as are the last Dense's 5 columns).  The bound is
the fp32 MFMA peak, 157.3 TFLOP/s.  With --stats the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv --
python tools/train_bench.py --batches B --steps S` run are divided by the steps the run made (S + 2) and the three GEMM forms are set
against their own FLOPs."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.3e12
C, K, H = 256, 3, 128


def gemm_flops(n_windows, nblocks=6):
    """(forward, data-gradient, weight-gradient) FLOPs of the MFMA GEMM forms in one step"""
    R = n_windows * 1024
    conv = 2.0 * R * (K * C) * C
    fwd = conv * (2 * nblocks - 1) + 2.0 * R * C * H
    dx = conv * (2 * nblocks - 1) + 2.0 * R * H * C
    dw = conv * (2 * nblocks - 1) + 2.0 * R * C * H
    return fwd, dx, dw


def run(batches, steps, seed):
    from radian_amd import Backend, weights
    rng = np.random.default_rng(seed)
    out = {}
    with Backend(0) as be:
        be.load_weights(weights.keras_init_weights(seed))
        for n in batches:
            x = rng.normal(size=(n, 1024)).astype(np.float32)
            d = be.dev_alloc(x.nbytes)
            be.h2d(d, x)
            labs = [rng.integers(0, 4, size=60) for _ in range(n)]
            il = [1024] * n
            for _ in range(2):
                be.train_step(d, il, labs, resident_n=n)
            ts = []
            for _ in range(steps):
                t0 = time.perf_counter()
                be.train_step(d, il, labs, resident_n=n)
                ts.append(time.perf_counter() - t0)
            be.dev_free(d)
            med = float(np.median(ts))
            fl = sum(gemm_flops(n))
            out[str(n)] = {"ms_per_step": med * 1e3, "best_ms": min(ts) * 1e3, "steps_per_s": 1 / med, "windows_per_s": n / med,
                           "samples_per_s": n * 1024 / med, "gemm_gflop_per_step": fl / 1e9, "fraction_of_fp32_peak": fl / med / PEAK}
    return out


def summarise(path, n, calls):
    fwd, dx, dw = gemm_flops(n)
    per_form = {"gemm_kernel<0": fwd, "gemm_kernel<1": dx, "gemm_kernel<2": dw}   # forward, data gradient, weight gradient
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName")
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            rows.append((name, total_ns / calls / 1e6, int(r.get("Calls", 0)) / calls))
    rows.sort(key=lambda t: -t[1])
    step_ms = sum(t[1] for t in rows)
    res = {"windows": n, "kernel_ms_per_step": step_ms, "kernels": []}
    form_ms = {}
    for name, ms, launches in rows:
        res["kernels"].append({"name": name[:120], "ms_per_step": ms, "launches_per_step": launches})
        for k in per_form:
            if k in name:
                form_ms[k] = form_ms.get(k, 0.0) + ms
    res["gemm_forms"] = {k: {"ms_per_step": v, "fraction_of_fp32_peak": per_form[k] / (v * 1e-3) / PEAK} for k, v in form_ms.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    res = summarise(a.stats, batches[0], a.steps + 2) if a.stats else run(batches, a.steps, a.seed)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
