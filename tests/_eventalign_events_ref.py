"""The contract of eventalign on event rows (include/radian_hip.h, rd_eventalign_events) restated from its text: a
plain-Python version (Python ints, lists, the three-way strict tie-break) and a NumPy int64 twin for the large cases.  The sample rule,
the k-mer rule and the cell's cost are _eventalign_ref's restatements; nothing is shared with the library or with radian_amd.eventalign.

A read's events are a dict of equally long sequences start, sum, sumsq, min, max (rd_segment's records); T is the window's length."""
import numpy as np

from _eventalign_ref import CAP, EMPTY, INF, MAD_ZERO, MAX_T, NO_PATH, OK, TOO_LONG, ZMAX, Model, cost, kmer, quant, state_models  # noqa: F401

STAY, ADV, SKIP = 0, 1, 2
PEN_MAX = 256
FIELDS = ("row_first", "row_last", "start", "end", "sum", "sumsq", "min", "max")


def events_of(x, starts):
    """the records of the samples x cut at starts (starts[0] == 0, strictly increasing): what rd_segment returns for those cuts"""
    x = np.asarray(x, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    assert len(x) and starts[0] == 0 and (np.diff(starts) > 0).all() and starts[-1] < len(x)
    return dict(start=starts.astype(np.int32), sum=np.add.reduceat(x, starts), sumsq=np.add.reduceat(x * x, starts),
                min=np.minimum.reduceat(x, starts).astype(np.int16), max=np.maximum.reduceat(x, starts).astype(np.int16))


def row_mean(total, n):
    """floor((2 sum + n) / (2 n)): the mean, rounded half up"""
    return (2 * int(total) + int(n)) // (2 * int(n))


def status_of(T, E, L, d4, pen):
    if T == 0 or E == 0:
        return EMPTY
    if T > MAX_T:
        return TOO_LONG
    if d4 == 0:
        return MAD_ZERO
    if (E if pen < 0 else 2 * E - 1) < L:
        return NO_PATH
    return OK


def _blank(status, L):
    return dict(status=status, score=0, n_skipped=0, row_first=[-1] * L, row_last=[-1] * L, start=[-1] * L, end=[-1] * L, sum=[0] * L,
                sumsq=[0] * L, min=[0] * L, max=[0] * L, sums=[0] * 5)


def _rows(ev, T):
    start = [int(v) for v in ev["start"]]
    n = [b - a for a, b in zip(start, start[1:] + [T])]
    return start, n


def _walk(code, E, L, s, out):
    """the path back from state s at row E - 1; code(e, s) is the back-pointer.  -> {base: the row at which the path jumped over it}"""
    first, last, jumped = out["row_first"], out["row_last"], {}
    if 1 <= s <= L:
        last[s - 1] = E - 1
    for e in range(E - 1, 0, -1):
        c = code(e, s)
        if c == STAY:
            continue
        if s <= L:
            first[s - 1] = e
        if c == SKIP:
            assert 1 <= s - 1 <= L
            jumped[s - 2] = e
        if s - c >= 1:
            last[s - c - 1] = e - 1
        s -= c
    if s == 1 and L >= 1:
        first[0] = 0
    assert s in (0, 1)
    return jumped


def _finish(out, jumped, ev, T, codes, model, off):
    """per-base records and fit sums of an OK read from its rows"""
    L = len(codes)
    start, _ = _rows(ev, T)
    E = len(start)
    out["n_skipped"] = len(jumped)
    for b in range(L):
        if b in jumped:
            assert out["row_first"][b] == -1 and out["row_last"][b] == -1
            out["start"][b] = out["end"][b] = start[jumped[b]] + off
            continue
        f, l = out["row_first"][b], out["row_last"][b]
        assert 0 <= f <= l < E
        out["start"][b] = start[f] + off
        out["end"][b] = (start[l + 1] if l + 1 < E else T) + off
        out["sum"][b] = sum(int(v) for v in ev["sum"][f:l + 1])
        out["sumsq"][b] = sum(int(v) for v in ev["sumsq"][f:l + 1])
        out["min"][b] = min(int(v) for v in ev["min"][f:l + 1])
        out["max"][b] = max(int(v) for v in ev["max"][f:l + 1])
        lv = model.lvl[kmer(codes, b, model.k)]
        n = out["end"][b] - out["start"][b]
        for i, v in enumerate((n, n * lv, n * lv * lv, out["sum"][b], out["sum"][b] * lv)):
            out["sums"][i] += v
    return out


def align_plain(ev, T, codes, model, m2, d4, pen, off=0):
    """one read, Python ints and lists only -> dict of every output field"""
    assert -1 <= pen <= PEN_MAX
    E, L = len(ev["start"]), len(codes)
    st = status_of(T, E, L, d4, pen)
    if st != OK:
        return _blank(st, L)
    start, n = _rows(ev, T)
    assert start[0] == 0 and all(v >= 1 for v in n)
    zq = [quant(row_mean(ev["sum"][e], n[e]), m2, d4) for e in range(E)]
    sm = state_models(codes, model)
    S = L + 2
    V = [INF] * S
    V[0], V[1] = n[0] * cost(zq[0], sm[0]), n[0] * cost(zq[0], sm[1])
    codes_rows = [[0] * S]
    for e in range(1, E):
        W, row = [INF] * S, [0] * S
        for s in range(min(2 * e + 1 if pen >= 0 else e + 1, S - 1) + 1):
            best, c = V[s], STAY
            if s >= 1 and V[s - 1] < best:                      # the advance only if STRICTLY smaller than stay
                best, c = V[s - 1], ADV
            if pen >= 0 and s >= 2 and V[s - 2] + pen < best:   # the skip only if STRICTLY smaller than the best of the two
                best, c = V[s - 2] + pen, SKIP
            assert best < 3 * (1 << 28)                         # a reachable cell: below 0.75 * 2^30
            W[s], row[s] = n[e] * cost(zq[e], sm[s]) + best, c
        V = W
        codes_rows.append(row)
    s = L + 1 if V[L + 1] < V[L] else L
    out = _blank(OK, L)
    out["score"] = V[s]
    jumped = _walk(lambda e, s: codes_rows[e][s], E, L, s, out)
    return _finish(out, jumped, ev, T, codes, model, off)


def align_numpy(ev, T, codes, model, m2, d4, pen, off=0):
    """the int64 twin: a row at a time over all states"""
    E, L = len(ev["start"]), len(codes)
    st = status_of(T, E, L, d4, pen)
    if st != OK:
        return _blank(st, L)
    S = L + 2
    start = np.asarray(ev["start"], dtype=np.int64)
    n = np.diff(np.concatenate([start, [T]]))
    tot = np.asarray(ev["sum"], dtype=np.int64)
    x = np.floor_divide(2 * tot + n, 2 * n)
    zq = np.clip(np.floor_divide(2 * 512 * (2 * x - m2) + d4, 2 * d4), -ZMAX, ZMAX)
    c = np.asarray(codes, dtype=np.int64)
    idx = np.zeros(L, dtype=np.int64)
    for j in range(-(model.k // 2), model.k // 2 + 1):
        idx = idx * 4 + (c[np.clip(np.arange(L) + j, 0, L - 1)] if L else c)
    tab = [np.asarray(a, dtype=np.int64) for a in (model.lvl, model.w, model.bias)]
    lvl, w, bias = (np.concatenate([[model.bg[i]], tab[i][idx], [model.bg[i]]]).astype(np.int64) for i in range(3))

    def costs(z):
        d = z - lvl
        return np.minimum((d * d * w) >> 32, CAP) + bias

    V = np.full(S, INF, dtype=np.int64)
    V[:2] = n[0] * costs(zq[0])[:2]
    bp = np.zeros((E, S), dtype=np.uint8)
    adv, skp = np.full(S, INF, dtype=np.int64), np.full(S, 2 * INF, dtype=np.int64)
    for e in range(1, E):
        adv[1:] = V[:-1]
        take = adv < V
        best = np.where(take, adv, V)
        code = take.astype(np.uint8)
        if pen >= 0:
            skp[2:] = V[:-2] + pen
            jump = skp < best
            best = np.where(jump, skp, best)
            code[jump] = SKIP
        V = n[e] * costs(zq[e]) + best
        V[(2 * e + 1 if pen >= 0 else e + 1) + 1:] = INF          # the cells above are unreachable
        bp[e] = code
    s = L + 1 if V[L + 1] < V[L] else L
    out = _blank(OK, L)
    out["score"] = int(V[s])
    jumped = _walk(lambda e, s: int(bp[e, s]), E, L, s, out)
    return _finish(out, jumped, ev, T, codes, model, off)


def assert_read_equal(res, r, want, what=""):
    """read r of a backend EvalRowsResult against a restatement dict, every field"""
    for f, got in (("status", res.status[r]), ("score", res.score[r]), ("n_skipped", res.n_skipped[r])):
        assert int(got) == want[f], (what, r, f, int(got), want[f])
    assert [int(v) for v in res.fit_sums[r]] == want["sums"], (what, r, "sums", list(res.fit_sums[r]), want["sums"])
    got = dict(row_first=res.row_first[r], row_last=res.row_last[r], start=res.events.start[r], end=res.events.end[r], sum=res.events.sum[r],
               sumsq=res.events.sumsq[r], min=res.events.min[r], max=res.events.max[r])
    for f in FIELDS:
        g = [int(v) for v in got[f]]
        if g != want[f]:
            bad = [i for i, (a, b) in enumerate(zip(g, want[f])) if a != b]
            raise AssertionError((what, r, f, len(g), len(want[f]), bad[:5], [g[i] for i in bad[:5]], [want[f][i] for i in bad[:5]]))
