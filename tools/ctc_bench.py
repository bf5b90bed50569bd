#!/usr/bin/env python3
"""Model-evaluation cost: the CTC loss + greedy edit-distance kernels (rd_ctc_probs_resident, ctc.hip) against the forward of the same
batch (rd_forward_resident), 512 windows of 1024 rows, every row counted, labels of L = 25 and L = 63 (radian/model.py:10-13).

    python tools/ctc_bench.py [--windows 512] [--reps 20] [--out results.json]

Host clock around calls that end in a stream synchronise, after a warm-up call of each: forward = the forward kernels alone
(windows and rows resident); ctc = window metadata upload + ctc_alpha_kernel + ctc_greedy_ed_kernel + results copy-back.
state-steps = sum over windows of input_length * (2L + 1), the alpha recursion's work.  Median and best of --reps calls.
Kernel times alone come from a rocprofv3 --kernel-trace --stats run of this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from radian_amd import Backend, weights
    rng = np.random.default_rng(a.seed)
    n, T = a.windows, 1024
    win = rng.normal(size=(n, T)).astype(np.float32)
    il = np.full(n, T, dtype=np.int32)
    out = {"windows": n, "rows_per_window": T, "reps": a.reps, "timer": "host clock, call ends in hipStreamSynchronize"}
    with Backend(0) as be:
        be.load_weights(weights.synthetic_weights(seed=1234))
        d_win = be.dev_alloc(win.nbytes)
        d_probs = be.dev_alloc(n * T * 5 * 4)
        be.h2d(d_win, win)

        def fwd():
            be.forward_resident(d_win, n, T, d_probs)
            be.sync()

        out["forward_ms_median"], out["forward_ms_best"] = (x * 1e3 for x in _time(fwd, a.reps))
        for L in (25, 63):
            labs = rng.integers(0, 4, size=(n, L))
            res = {}

            def ctc():
                res["r"] = be.ctc_probs_resident(d_probs, n, il, labs, np.full(n, L))

            med, best = _time(ctc, a.reps)
            steps = float(il.astype(np.float64).sum() * (2 * L + 1))
            r = res["r"]
            out[f"L{L}"] = {
                "ctc_ms_median": med * 1e3, "ctc_ms_best": best * 1e3, "state_steps": steps,
                "state_steps_per_s_median": steps / med,
                "share_of_forward_plus_ctc_median": med / (med + out["forward_ms_median"] / 1e3),
                "loss_mean": float(np.mean(r.loss[np.isfinite(r.loss)])), "infeasible": int((r.status == 1).sum()),
                "greedy_len_mean": float(r.greedy_len.mean()), "edit_distance_mean": float(r.edit_distance.mean()),
            }
        be.dev_free(d_win)
        be.dev_free(d_probs)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
