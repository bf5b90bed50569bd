#!/usr/bin/env python3
"""Differential fuzz of the context's pipeline (rd_pipe_submit_raw_global / _chunk, rd_pipe_submit_reads, rd_pipe_submit,
rd_pipe_progress; csrc/pipe_reads.hip) against the blocking entry points on the GPU: random sequences of submits on ONE context -- form
(raw global / raw chunk / resident normalised reads / resident windows), geometry, beam width, LM on / off, thresholds, f16 logits, lanes,
group size, decode partition and precision change between rounds; read sets are ragged (1 .. 9000 samples, constant reads, reads around
the window length); progress is polled at random; blocking calls are interleaved.  Every delivered batch must equal the blocking call's
labels and status.   usage: fuzz_pipe.py [rounds] [seed]"""
import os, sys, time
from types import SimpleNamespace
import numpy as np
R = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from radian_amd import Backend, synthetic, weights



class Windows:
    """output arrays of a resident form's call (labels of window i at row i); a submit's are delivered once rd_pipe_progress reaches seq"""

    def __init__(self, be, n_windows, chunk):
        self.be = be
        self.labels = np.zeros((n_windows, chunk), dtype=np.uint8)
        self.lens = np.full(n_windows, -1, dtype=np.int32)

    def now(self):
        return [self.labels[i, : self.lens[i]].copy() for i in range(len(self.lens))]

    def wait(self):
        self.be.pipe_progress(self.seq)

    def result(self):
        self.wait()
        return self.now(), np.zeros(0, dtype=np.int32)   # (no per-read status)


def same(mode, a, b, status):
    if mode in ("reads", "windows"):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    if mode == "global":
        return all(st != 0 or np.array_equal(x, y) for x, y, st in zip(a, b, status))
    return all(st != 0 or (len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))) for x, y, st in zip(a, b, status))


def run(rounds=100, seed=0, max_len=9000, max_reads=30, log=print):
    """-> (batches delivered, mismatches against the blocking entry points)"""
    rng = np.random.default_rng(seed)
    be = Backend(0)
    w = weights.synthetic_weights(seed=1234).copy()
    w[-645:-5] *= np.float32(0.05)
    be.load_weights(w)
    be.load_lm(rng.dirichlet([0.3] * 4, size=4 ** 3), 3)

    def read_set(chunk, step):
        n = int(rng.integers(1, max_reads))
        out = []
        for _ in range(n):
            L = int(rng.choice([1, 2, chunk - 1, chunk, chunk + 1, chunk + step, 3 * step, int(rng.integers(1, max_len))]))
            if rng.random() < 0.05:
                out.append(np.full(max(L, 2), 7, dtype=np.int16))
            else:
                out.append(synthetic.synthetic_reads(1, L, seed=int(rng.integers(1 << 30)))[0])
        return out

    def resident_set(mode, reads, chunk, step):
        """the reads that normalise, as a resident form's device input: normalised reads (rd_pipe_submit_reads) or their windows
        (rd_pipe_submit)"""
        norm, status = be.normalise_reads(reads, 4)
        ok = [i for i in range(len(reads)) if status[i] == 0]
        if not ok:   # (every read constant or too short: one ordinary read instead)
            reads = [synthetic.synthetic_reads(1, chunk, seed=int(rng.integers(1 << 30)))[0]]
            norm, ok = be.normalise_reads(reads, 4)[0], [0]
        x = SimpleNamespace()
        if mode == "reads":
            sig = np.concatenate([norm[i] for i in ok])
            off = np.zeros(len(ok) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(norm[i]) for i in ok])
            x.n = sum(be.count_windows(len(norm[i]), chunk, step) for i in ok)
            x.call = lambda fn, W, lab, ln: fn(x.d, off, len(ok), chunk, step, W, lab, ln)
        else:
            sig, valid = synthetic.reads_to_windows([reads[i] for i in ok], chunk, step)[:2]
            x.n = sig.shape[0]
            x.call = lambda fn, W, lab, ln: fn(x.d, x.n, chunk, valid, W, lab, ln)
        x.d = be.dev_alloc(sig.nbytes)
        be.h2d(x.d, sig)
        return x

    def blocking(mode, chunk, step, W, lm, thr, reads):
        """-> (labels, status) of the blocking entry point; the resident forms have no per-read status"""
        if mode == "global":
            return be.basecall_raw_global(reads, 4, chunk, step, W, lm, *thr)
        if mode == "chunk":
            return be.basecall_raw_chunk(reads, 4, chunk, step, W)
        out = Windows(be, reads.n, chunk)
        reads.call(be.basecall_reads_chunk_resident if mode == "reads" else be.basecall_chunk_resident, W, out.labels, out.lens)
        return out.now(), np.zeros(0, dtype=np.int32)

    def submit(mode, chunk, step, W, lm, thr, reads):
        if mode in ("global", "chunk"):
            return be.pipe_submit_raw(mode, reads, 4, chunk, step, W, lm, *thr) if mode == "global" else be.pipe_submit_raw(mode, reads, 4, chunk, step, W)
        t = Windows(be, reads.n, chunk)
        reads.call(be.pipe_submit_reads if mode == "reads" else be.pipe_submit, W, t.labels, t.lens)
        t.seq = be.pipe_submitted()
        return t

    t0 = time.time()
    n_fail = n_batches = 0
    for rd in range(rounds):
        be.pipe_flush()
        be.pipe_config(int(rng.integers(1, 7)))
        be.pipe_set_lanes(int(rng.integers(1, 5)))
        be.set_decode_partition(int(rng.choice([-1, 0, 1, 4])))
        be.set_logits("f16" if rng.random() < 0.2 else "f32")
        be.set_precision("bf16x3" if rng.random() < 0.15 else "fp32")
        chunk = int(rng.choice([256, 512, 1024]))
        plan = []
        for _ in range(int(rng.integers(2, 9))):
            mode = str(rng.choice(["chunk", "global", "reads", "windows"], p=[0.3, 0.5, 0.1, 0.1]))
            step = int(rng.choice([chunk, chunk // 2, chunk // 4, max(1, chunk - 252), max(1, chunk - 253), int(rng.integers(chunk // 8, chunk + 1))]))
            # (mostly the lane kernels' common widths; now and then their upper forms -- W 26..51, 52..64 -- and the general kernel above 64)
            W = int(rng.choice([1, 3, 6, 7, 10, 12, 13, 25])) if rng.random() < 0.9 else int(rng.choice([40, 52, 64, 65, 100, 128, 130, 256, 260]))
            lm = bool(mode == "global" and rng.random() < 0.5)
            thr = (float(rng.choice([0.0, 0.3, 0.6])), float(rng.choice([0.2, 0.9, 5.0])))
            reads = read_set(chunk, step)
            plan.append((mode, step, W, lm, thr, resident_set(mode, reads, chunk, step) if mode in ("reads", "windows") else reads))
        ref = [blocking(mode, chunk, step, W, lm, thr, reads) for mode, step, W, lm, thr, reads in plan]
        tickets = []
        for i, (mode, step, W, lm, thr, reads) in enumerate(plan):
            tickets.append(submit(mode, chunk, step, W, lm, thr, reads))
            r = rng.random()
            if r < 0.2:
                be.pipe_progress(0)
            elif r < 0.3:
                tickets[int(rng.integers(0, len(tickets)))].wait()
            elif r < 0.4:      # a blocking call in between shares the context's workspaces
                j = int(rng.integers(0, len(plan)))
                m2, s2, W2, lm2, thr2, reads2 = plan[j]
                again = blocking(m2, chunk, s2, W2, lm2, thr2, reads2)
                if not (np.array_equal(again[1], ref[j][1]) and same(m2, again[0], ref[j][0], ref[j][1])):
                    n_fail += 1
                    log(f"MISMATCH (interleaved blocking call) round={rd} batch={j}")
        if rng.random() < 0.5:
            be.pipe_flush()
        for i, t in enumerate(tickets):
            got, status = t.result()
            n_batches += 1
            if not (np.array_equal(status, ref[i][1]) and same(plan[i][0], got, ref[i][0], status)):
                n_fail += 1
                mode, step, W, lm, thr, reads = plan[i]
                lens = [len(r) for r in reads] if mode in ("global", "chunk") else reads.n
                log(f"MISMATCH round={rd} batch={i} mode={mode} chunk={chunk} step={step} W={W} lm={lm} thr={thr} lens={lens}")
        for mode, step, W, lm, thr, reads in plan:
            if mode in ("reads", "windows"):
                be.dev_free(reads.d)
        if rd % 10 == 9:
            log(f"{rd + 1} rounds, {n_batches} batches, {n_fail} failures, {time.time() - t0:.0f}s")
    be.close()
    return n_batches, n_fail


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]]
    n_batches, n_fail = run(*a, log=lambda m: print(m, flush=True))
    print(f"done: {n_batches} batches, {n_fail} failures")
    sys.exit(1 if n_fail else 0)
