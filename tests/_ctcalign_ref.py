"""Plain-Python restatement of the forced CTC alignment contract (include/radian_hip.h, rd_ctc_align_batch):
what tests/test_gpu_ctcalign.py and tests/test_gpu_fastq.py compare the GPU with, bit for bit.

    states   s = 0 .. 2L; even = blank (class 4), odd 2i+1 = label i
    lp       math.log(float(P[t][c])) per element (the machine's libm, as the decode tests rely on); log 0 = -inf
    start    V[0][0] = lp[0][4], V[0][1] = lp[0][c_0], the rest -inf
    step     V[t][s] = lp[t][cls(s)] + max(V[t-1][s], V[t-1][s-1], V[t-1][s-2]); the third only for odd s >= 3 with c_i != c_{i-1};
             a predecessor replaces the best so far only if STRICTLY greater, tried in the order s, s-1, s-2
    end      2L, or 2L-1 if V[T-1][2L-1] is strictly greater

`align` is the restatement: a Python list of floats per row, one comparison at a time.  `align_fast` does the same row step on
numpy float64 vectors (IEEE add and compare per element: the same bits) for the cases of thousands of states;
tests/test_ctcalign_ref_cpu.py holds the two to each other."""
import math

import numpy as np

NEG = float("-inf")
OK, NO_PATH, TOO_LARGE = 0, 1, 2
THRESHOLDS = [10.0 ** (-k / 10) for k in range(1, 51)]


class Result:
    __slots__ = ("score", "status", "first_step", "last_step", "qual", "margin")

    def __init__(self, score, status, first_step, last_step, qual, margin):
        self.score, self.status, self.first_step, self.last_step, self.qual, self.margin = score, status, first_step, last_step, qual, margin


def log_rows(P):
    return [[math.log(float(x)) if float(x) > 0 else NEG for x in row] for row in P]


def _finish(P, lab, T, L, V_end, V_end1, bp_of):
    """end state, traceback (bp_of(t, s) -> 0, 1, 2), steps and qualities"""
    end = 2 * L
    if L and V_end1 > V_end:
        end = 2 * L - 1
    score = V_end1 if end == 2 * L - 1 else V_end
    if score == NEG:
        return Result(score, NO_PATH, [-1] * L, [-1] * L, [0] * L, 1.0)
    s = end
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t:
            s -= bp_of(t, s)
    assert path[0] in (0, 1)
    first, last = [-1] * L, [-1] * L
    for t, s in enumerate(path):
        if s % 2:
            i = s // 2
            if first[i] < 0:
                first[i] = t
            last[i] = t
    assert all(f >= 0 for f in first), "a base without a step"
    qual, margin = [], 1.0
    for i in range(L):
        assert all(path[t] == 2 * i + 1 for t in range(first[i], last[i] + 1))
        p = max(float(P[t][lab[i]]) for t in range(first[i], last[i] + 1))
        e = 1.0 - p
        qual.append(sum(1 for th in THRESHOLDS if e <= th))
        margin = min(margin, min(abs(e - th) / th for th in THRESHOLDS))
    return Result(score, OK, first, last, qual, margin)


def align(P, lab):
    """P: [T,5] (numpy float32 / float64, or nested lists); lab: L labels in 0..3.  -> Result; margin is the smallest relative distance of
    any e = 1 - p to a quality threshold (1.0 when there is no base)."""
    lab = [int(c) for c in lab]
    T, L = len(P), len(lab)
    if T == 0:
        raise ValueError("T = 0 is an argument error")
    S = 2 * L + 1
    lp = log_rows(P)
    cls = [4 if s % 2 == 0 else lab[s // 2] for s in range(S)]
    V = [NEG] * S
    V[0] = lp[0][4]
    if L:
        V[1] = lp[0][lab[0]]
    bp = [None] * T
    for t in range(1, T):
        N = [NEG] * S
        row = bytearray(S)
        for s in range(S):
            best, b = V[s], 0
            if s >= 1 and V[s - 1] > best:
                best, b = V[s - 1], 1
            if s >= 3 and s % 2 == 1 and lab[s // 2] != lab[s // 2 - 1] and V[s - 2] > best:
                best, b = V[s - 2], 2
            N[s] = lp[t][cls[s]] + best
            row[s] = b
        V = N
        bp[t] = row
    return _finish(P, lab, T, L, V[S - 1], V[S - 2] if L else NEG, lambda t, s: bp[t][s])


def align_fast(P, lab):
    """`align` with the states of a row as one numpy float64 vector (the same operations per element)"""
    lab = [int(c) for c in lab]
    T, L = len(P), len(lab)
    if T == 0:
        raise ValueError("T = 0 is an argument error")
    S = 2 * L + 1
    lp = np.array(log_rows(P), dtype=np.float64)
    cls = np.full(S, 4, dtype=np.int64)
    cls[1::2] = lab
    can_skip = np.zeros(S, dtype=bool)
    for i in range(1, L):
        can_skip[2 * i + 1] = lab[i] != lab[i - 1]
    V = np.full(S, NEG)
    V[0] = lp[0][4]
    if L:
        V[1] = lp[0][lab[0]]
    bp = np.zeros((T, S), dtype=np.uint8)
    for t in range(1, T):
        best = V.copy()
        b = bp[t]
        a1 = np.full(S, NEG)
        a1[1:] = V[:-1]
        m = a1 > best
        best[m] = a1[m]
        b[m] = 1
        a2 = np.full(S, NEG)
        a2[2:] = V[:-2]
        m = can_skip & (a2 > best)
        best[m] = a2[m]
        b[m] = 2
        V = lp[t][cls] + best
    return _finish(P, lab, T, L, float(V[S - 1]), float(V[S - 2]) if L else NEG, lambda t, s: int(bp[t, s]))


def workspace_bytes(T, L):
    """the documented workspace formula: each term rounded up to 256 bytes"""
    up = lambda x: (x + 255) // 256 * 256
    return up(64 * T) + up(4 * T * ((2 * L + 1 + 15) // 16)) + up(16 * T)


def peaky(T, lab, rng, dtype):
    """blank-heavy softmax rows, every label boosted at one of len(lab) increasing rows"""
    z = rng.normal(0, 1.0, (T, 5))
    z[:, 4] += 2.5
    if len(lab) <= T:
        pos = np.sort(rng.choice(T, len(lab), replace=False))
        for i, t in enumerate(pos):
            z[t, lab[i]] += 4.0
    e = np.exp(z - z.max(1, keepdims=True))
    return np.ascontiguousarray((e / e.sum(1, keepdims=True)).astype(dtype))
