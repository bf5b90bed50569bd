"""The fit cases that tests/test_gpu_label_build.py runs under every score set, and the means by which tests/test_label_build_cpu.py
shows that they tell a wrongly written tie comparison of fit_kernel from the right one.  Test infrastructure only."""
import numpy as np

import _fit_ref as fr


def mutate(rng, seq, rate):
    """substitutions, deletions and insertions at `rate` in all, a third each"""
    out = []
    for c in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(int(rng.integers(0, 4)) if r < 2 * rate / 3 else int(c))
        if rng.random() < rate / 3:
            out.append(int(rng.integers(0, 4)))
    return np.array(out if out else [int(rng.integers(0, 4))], dtype=np.uint8)


def fit_cases_small():
    """_fit_cases without the 20 000-code reference and with one query per length: every launch class {B, G} of fit.hip (m <= 16, 32,
    64, 128, 256, 512, 1024 and the lengths on either side), short references (n < m among them), the tie cases and code 4"""
    rng = np.random.default_rng(21)
    refs, queries, qref = [], [], []

    def add_ref(r):
        refs.append(np.asarray(r, dtype=np.uint8))
        return len(refs) - 1

    def add(r, q):
        q = np.asarray(q, dtype=np.uint8)
        assert 1 <= len(q) <= 1024 and q.max() <= 3
        queries.append(q)
        qref.append(r)

    def sub(r, m, rate):
        ref = refs[r]
        ref = np.where(ref == 4, rng.integers(0, 4, size=len(ref)), ref)
        lo = int(rng.integers(0, max(1, len(ref) - m + 1)))
        return mutate(rng, ref[lo: lo + m], rate)[:1024]

    r0 = add_ref(rng.integers(0, 4, size=1500))
    for k, m in enumerate((1, 2, 8, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 513, 1024)):
        lo = int(rng.integers(0, 1500 - m + 1))
        add(r0, refs[r0][lo: lo + m] if k % 3 == 0 else sub(r0, m, (0.04, 0.15)[k % 2]))   # exact lengths and mutated ones
    add(r0, rng.integers(0, 4, size=1024))                                                 # unrelated
    add(r0, rng.integers(0, 4, size=16))
    for n in (0, 1, 63, 64, 65):
        r = add_ref(rng.integers(0, 4, size=n))
        for m in (1, 5, 64, 65, 100):
            add(r, rng.integers(0, 4, size=m))
        if n >= 8:
            add(r, sub(r, n, 0.1))
    rh = add_ref(np.zeros(300, dtype=np.uint8))
    for m in (1, 2, 10, 65, 300, 320):
        add(rh, np.zeros(m, dtype=np.uint8))
    add(rh, [0] * 10 + [1] + [0] * 10)
    add(rh, [1] * 12)
    rd = add_ref(np.tile([0, 1], 200))
    for k in (1, 5, 33, 128):
        add(rd, np.tile([0, 1], k))
        add(rd, np.tile([1, 0], k))
        add(rd, np.tile([0, 1], k)[:-1])
    add(rd, list(np.tile([0, 1], 20)) + [0] + list(np.tile([0, 1], 20)))
    add(rd, list(np.tile([0, 1], 20)) + [2, 2] + list(np.tile([0, 1], 20)))
    rt = add_ref(np.tile([0, 0, 1], 100))
    add(rt, np.tile([0, 1], 30))
    add(rt, np.tile([0, 0, 1], 21)[1:])
    r4 = rng.integers(0, 4, size=800)
    r4[rng.random(800) < 0.05] = 4
    r4 = add_ref(r4)
    for m, rate in ((10, 0.0), (30, 0.1), (64, 0.1), (200, 0.0)):
        add(r4, sub(r4, m, rate))
    add(add_ref(np.full(50, 4)), rng.integers(0, 4, size=20))
    for r, q in TIE_CASES:
        add(add_ref(r), q)
    return refs, queries, np.array(qref, dtype=np.int32)


# Small cases over two or three letters in which the traceback meets a tie of "extend" and "close" inside a gap run whose two branches
# lead to different spans or counts: found by searching random cases with the restatement's traceback deciding that tie the other way
# (trace_tie_flipped below).  With them every score set of SMALL_SETS tells a kernel with `ee >= eo` or `fe >= fo` written `>` from
# the right one (tests/test_label_build_cpu.py checks that of the whole case list).
TIE_CASES = (
    ([0, 0, 0, 2, 0, 0, 0, 2, 0, 2, 1, 1], [2, 2, 2, 2, 1, 1, 0, 1, 2, 1, 0]),
    ([0, 2, 1, 2, 1, 2, 0, 0, 1], [1, 0, 1, 1, 1, 2, 0, 2, 1, 0, 2, 1, 2, 0, 2, 0, 1, 0, 0, 0, 1, 2, 2]),
    ([2, 2, 1, 2, 0, 1, 2, 0, 2, 1, 1, 2, 0, 0, 2, 0, 1, 1, 2, 1, 1, 2, 0, 2], [1, 1, 1, 2, 1, 1, 1, 1, 0, 1, 2, 1, 1, 0, 2]),
    ([0, 1, 0, 0, 1, 2, 0, 0, 2, 0, 0, 2, 2, 2, 2, 0, 1, 2, 2, 1, 2, 1, 0, 0, 1, 2, 0, 1, 0, 1, 2, 0, 0],
     [1, 1, 0, 1, 1, 0, 2, 1, 1, 0, 1, 0, 1, 1, 2, 2, 0, 0, 0, 2, 1, 1]),
    ([1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1], [1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0]),
    ([0, 0, 2, 2, 1, 1, 2, 0, 0, 2, 1, 2, 1, 1, 2, 2, 1, 0, 0, 0, 2, 2, 2, 0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1],
     [2, 1, 0, 2, 0, 0, 1, 2, 1, 0, 0, 0, 2]),
    ([0, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1],
     [0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0]),
    ([2, 1, 1, 2, 1, 0, 1, 0, 1, 1, 1, 2, 2, 1], [1, 1, 2, 2, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 2, 2, 2, 2, 2]),
    ([0, 0, 2, 1, 2, 0, 1, 0, 2, 1, 2, 2, 0, 0, 2, 2, 2, 0, 1, 0, 1, 1, 2, 2, 2, 2, 1, 2, 0, 0, 2, 0, 1, 2], [0, 2, 1, 2, 0, 0, 2, 0, 1, 0, 0, 1, 0, 0]),
)


def trace_tie_flipped(H, E, F, ref, query, scores, flip):
    """NOT the contract: fr._trace with the tie of "extend" and "close" inside a deletion run (flip "E") or an insertion run (flip "F")
    decided the other way, close first -- what a kernel with `ee >= eo` / `fe >= fo` written `>` would report.  Only for showing that
    the cases above tell the two apart."""
    _, _, go, ge = scores
    n, m = len(ref), len(query)
    col = [int(H[i][m]) for i in range(n + 1)]
    score = max(col)
    end = col.index(score)
    i, j, state = end, m, "H"
    n_match = n_sub = n_ins = n_del = 0
    while j > 0:
        if state == "H":
            if i == 0:
                state = "F"
            elif H[i][j] == H[i - 1][j - 1] + fr._sub(ref[i - 1], query[j - 1], scores):
                if ref[i - 1] == query[j - 1]:
                    n_match += 1
                else:
                    n_sub += 1
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = "E"
            else:
                state = "F"
        elif state == "E":
            n_del += 1
            if (E[i][j] == H[i - 1][j] + go) if flip == "E" else (E[i][j] != E[i - 1][j] + ge):
                state = "H"
            i -= 1
        else:
            n_ins += 1
            if (F[i][j] == H[i][j - 1] + go) if flip == "F" else (F[i][j] != F[i][j - 1] + ge):
                state = "H"
            j -= 1
    return {"score": int(score), "ref_start": i, "ref_end": end, "counts": (n_match, n_sub, n_ins, n_del)}
