"""A plain restatement of rd_fit_batch's contract (include/radian_hip.h) with its traceback, and of
radian_amd.label_build's selection rules on top of it.  Test infrastructure: nothing here is shared with the library or the command.

fit(ref, query, scores)        the contract cell by cell, in Python ints (any scores)
fit_rows(ref, query, scores)   the same matrices filled a reference row at a time with NumPy, for the long cases.  Needs
                               gap_open <= gap_extend: opening a gap out of a cell that a gap reached is then never better than
                               extending that gap, so F of a row is a running maximum over max(diagonal, E).  tests/test_label_build_cpu.py
                               checks the two against each other.
brute(ref, query, scores)      every (start, end) span against the whole query with an ordinary global affine-gap alignment
Codes: queries 0..3, references 0..4; code 4 equals nothing, itself included."""
import numpy as np

from _align_ref import ACCEPTED_SETS, BOUND_SETS, REFUSED_SET, SMALL_SETS   # the score sets the tests run besides the default

NEG = -(1 << 40)
NEG32 = -(1 << 29)   # fit_rows' stored -inf: far below any score, and NEG32 + a gap score still fits
SCORES = (2, -4, -4, -2)   # match, mismatch, gap open, gap extend


def _sub(a, b, scores):
    return scores[0] if (a == b and a < 4) else scores[1]


def _matrices(ref, query, scores):
    _, _, go, ge = scores
    n, m = len(ref), len(query)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    for j in range(1, m + 1):
        H[0][j] = F[0][j] = go + (j - 1) * ge
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(H[i - 1][j] + go, E[i - 1][j] + ge)
            F[i][j] = max(H[i][j - 1] + go, F[i][j - 1] + ge)
            H[i][j] = max(H[i - 1][j - 1] + _sub(ref[i - 1], query[j - 1], scores), E[i][j], F[i][j])
    return H, E, F


def _matrices_rows(ref, query, scores):
    ma, mi, go, ge = scores
    assert go <= ge, "fit_rows needs gap_open <= gap_extend"
    ref = np.asarray(ref, dtype=np.int64)
    query = np.asarray(query, dtype=np.int64)
    n, m = len(ref), len(query)
    H = np.zeros((n + 1, m + 1), dtype=np.int32)   # (int32 storage: the 20 000-row cases; a row is computed in int64)
    E = np.full((n + 1, m + 1), NEG32, dtype=np.int32)
    F = np.full((n + 1, m + 1), NEG32, dtype=np.int32)
    j = np.arange(1, m + 1)
    H[0, 1:] = F[0, 1:] = go + (j - 1) * ge
    jj = np.arange(m + 1)
    for i in range(1, n + 1):
        up = H[i - 1].astype(np.int64)
        e = np.maximum(up[1:] + go, E[i - 1, 1:].astype(np.int64) + ge)
        a = ref[i - 1]
        s = np.where((query == a) & (a < 4), ma, mi)
        hat = np.empty(m + 1, dtype=np.int64)   # max(diagonal, E); column 0 is H(i, 0) = 0
        hat[0] = 0
        hat[1:] = np.maximum(up[:-1] + s, e)
        # F(i, j) = max over k < j of hat(k) + go + (j - k - 1) * ge
        run = np.maximum.accumulate(hat - jj * ge)
        f = run[:-1] + go - ge + j * ge
        E[i, 1:] = e
        F[i, 1:] = f
        H[i, 1:] = np.maximum(hat[1:], f)
    return H, E, F


def _trace(H, E, F, ref, query, scores):
    _, _, go, ge = scores
    n, m = len(ref), len(query)
    col = [int(H[i][m]) for i in range(n + 1)]
    score = max(col)
    end = col.index(score)   # the smallest row that attains it
    i, j, state = end, m, "H"
    n_match = n_sub = n_ins = n_del = 0
    while j > 0:
        if state == "H":
            if i == 0:
                state = "F"   # H(0, j) = F(0, j): a run of insertions
            elif H[i][j] == H[i - 1][j - 1] + _sub(ref[i - 1], query[j - 1], scores):
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
            if E[i][j] != E[i - 1][j] + ge:   # extend before close
                state = "H"
            i -= 1
        else:
            n_ins += 1
            if F[i][j] != F[i][j - 1] + ge:
                state = "H"
            j -= 1
    return {"score": int(score), "ref_start": i, "ref_end": end, "counts": (n_match, n_sub, n_ins, n_del)}


def fit(ref, query, scores=SCORES):
    ref, query = [int(c) for c in ref], [int(c) for c in query]
    assert len(query) >= 1
    return _trace(*_matrices(ref, query, scores), ref, query, scores)


def fit_rows(ref, query, scores=SCORES):
    ref, query = [int(c) for c in ref], [int(c) for c in query]
    assert len(query) >= 1
    return _trace(*_matrices_rows(ref, query, scores), ref, query, scores)


def _global(a, b, scores):
    """ordinary global affine-gap score of a against b (end gaps penalised)"""
    _, _, go, ge = scores
    n, m = len(a), len(b)
    gap = lambda L: 0 if L == 0 else go + (L - 1) * ge
    M = [[NEG] * (m + 1) for _ in range(n + 1)]
    X = [[NEG] * (m + 1) for _ in range(n + 1)]   # ends in a gap in b (consumes a)
    Y = [[NEG] * (m + 1) for _ in range(n + 1)]   # ends in a gap in a (consumes b)
    M[0][0] = 0
    for i in range(1, n + 1):
        X[i][0] = gap(i)
    for j in range(1, m + 1):
        Y[0][j] = gap(j)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            best = max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1])
            M[i][j] = best + _sub(a[i - 1], b[j - 1], scores)
            X[i][j] = max(max(M[i - 1][j], Y[i - 1][j]) + go, X[i - 1][j] + ge)
            Y[i][j] = max(max(M[i][j - 1], X[i][j - 1]) + go, Y[i][j - 1] + ge)
    return max(M[n][m], X[n][m], Y[n][m])


def brute(ref, query, scores=SCORES):
    """(best score over every span, the smallest end of a span that attains it)"""
    ref, query = [int(c) for c in ref], [int(c) for c in query]
    best, best_end = None, None
    for end in range(len(ref) + 1):
        for start in range(end + 1):
            s = _global(ref[start:end], query, scores)
            if best is None or s > best:
                best, best_end = s, end
    return best, best_end


# ---- the selection rules of radian_amd.label_build, restated ----
def ctc_need(label):
    """rows a CTC path of the label needs: its length plus its adjacent repeats"""
    label = [int(c) for c in label]
    return len(label) + sum(1 for k in range(1, len(label)) if label[k] == label[k - 1])


def chain(starts):
    """indices of the longest subsequence with non-decreasing starts; of the longest ones, the lexicographically earliest indices"""
    n = len(starts)
    tail = [1] * n   # the longest chain that begins at k
    for k in range(n - 1, -1, -1):
        for l in range(k + 1, n):
            if starts[l] >= starts[k]:
                tail[k] = max(tail[k], 1 + tail[l])
    out, want, floor = [], max(tail, default=0), None
    for k in range(n):
        if want and tail[k] == want and (floor is None or starts[k] >= floor):
            out.append(k)
            floor, want = starts[k], want - 1
    return out


def select(calls, signal_lengths, ref_dec, min_identity=0.9, min_call=8, max_label_len=255, scores=SCORES, fit_fn=None):
    """statuses and spans of one read's windows: [(status, fit or None)] in window order; ref_dec = the reference in decode order"""
    fit_fn = fit_fn or fit_rows
    rows = []
    for call, sl in zip(calls, signal_lengths):
        if len(call) == 0:
            rows.append(["short", None])
            continue
        r = fit_fn(ref_dec, call, scores)
        nm, ns, ni, nd = r["counts"]
        label = [int(c) for c in ref_dec[r["ref_start"]:r["ref_end"]]]
        if len(call) < min_call:
            st = "short"
        elif nm / (nm + ns + ni + nd) < min_identity:
            st = "low-identity"
        elif len(label) == 0:
            st = "low-identity"
        elif 4 in label:
            st = "has-N"
        elif len(label) > max_label_len:
            st = "too-long"
        elif ctc_need(label) > sl:
            st = "infeasible"
        else:
            st = "kept"
        rows.append([st, r])
    cand = [k for k, (st, _) in enumerate(rows) if st == "kept"]
    on = set(cand[c] for c in chain([rows[k][1]["ref_start"] for k in cand]))
    for k in cand:
        if k not in on:
            rows[k][0] = "off-chain"
    return [tuple(r) for r in rows]
