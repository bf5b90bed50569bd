"""The eventalign contract (include/radian_hip.h, rd_eventalign) restated from its text: a plain-Python version (Python ints, lists, the
strict tie-break) and a NumPy int64 twin for the large cases.  Neither shares code with the library or with radian_amd.eventalign."""
import numpy as np

OK, EMPTY, TOO_LONG, MAD_ZERO, NO_PATH, TOO_LARGE = 0, 1, 2, 3, 4, 5
INF = 1 << 30
MAX_T = 1 << 19
ZMAX = 1 << 14
CAP = 1024


class Model:
    """k; lvl, w, bias: lists of 4^k Python ints; bg = (lvl, w, bias)"""

    def __init__(self, k, lvl, w, bias, bg):
        self.k, self.lvl, self.w, self.bias = int(k), [int(v) for v in lvl], [int(v) for v in w], [int(v) for v in bias]
        self.bg = tuple(int(v) for v in bg)


def window_scale(x):
    """m2 = the sum of the two middle order statistics; d4 = the same of |2x - m2|"""
    T = len(x)
    s = sorted(int(v) for v in x)
    m2 = s[(T - 1) // 2] + s[T // 2]
    d = sorted(abs(2 * int(v) - m2) for v in x)
    return m2, d[(T - 1) // 2] + d[T // 2]


def quant(x, m2, d4):
    u = 512 * (2 * int(x) - m2)
    return max(-ZMAX, min(ZMAX, (2 * u + d4) // (2 * d4)))   # Python's // is the floor


def kmer(codes, b, k):
    L, idx = len(codes), 0
    for j in range(-(k // 2), k // 2 + 1):
        idx = idx * 4 + int(codes[min(max(b + j, 0), L - 1)])
    return idx


def state_models(codes, model):
    """[(lvl, w, bias)] of the states 0 .. L + 1"""
    mid = [(model.lvl[i], model.w[i], model.bias[i]) for i in (kmer(codes, b, model.k) for b in range(len(codes)))]
    return [model.bg] + mid + [model.bg]


def cost(z, st):
    d = z - st[0]
    return min((d * d * st[1]) >> 32, CAP) + st[2]


def _blank(status, L, m2=0, d4=0):
    return dict(status=status, score=0, m2=m2, d4=d4, first=[-1] * L, last=[-1] * L, start=[-1] * L, end=[-1] * L, sum=[0] * L, sumsq=[0] * L,
                min=[0] * L, max=[0] * L, sums=[0] * 5)


def _finish(out, raw, codes, model):
    """events and fit sums of an OK read from its steps"""
    L = len(codes)
    first, last = out["first"], out["last"]
    for b in range(L):
        s, e = first[b], (first[b + 1] if b + 1 < L else last[L - 1] + 1)
        seg = [int(v) for v in raw[s:e]]
        out["start"][b], out["end"][b], out["sum"][b], out["sumsq"][b] = s, e, sum(seg), sum(v * v for v in seg)
        out["min"][b], out["max"][b] = min(seg), max(seg)
        l = model.lvl[kmer(codes, b, model.k)]
        n = e - s
        for i, v in enumerate((n, n * l, n * l * l, out["sum"][b], out["sum"][b] * l)):
            out["sums"][i] += v
    return out


def _walk(bit, T, L, s, t_lo, out):
    """the path back from state s at row T - 1; bit(t, s) is the back-pointer"""
    first, last = out["first"], out["last"]
    if 1 <= s <= L:
        last[s - 1] = T - 1 + t_lo
    for t in range(T - 1, 0, -1):
        if bit(t, s):
            if s <= L:
                first[s - 1] = t + t_lo
            if s - 1 >= 1:
                last[s - 2] = t - 1 + t_lo
            s -= 1
    if s == 1 and L >= 1:
        first[0] = t_lo
    assert s in (0, 1)


def align_plain(raw, codes, model, t_lo=0, t_hi=None, m2=0, d4=0):
    """one read, Python ints and lists only -> dict of every output field"""
    t_hi = len(raw) if t_hi is None else t_hi
    x = [int(v) for v in raw[t_lo:t_hi]]
    T, L = len(x), len(codes)
    if T == 0:
        return _blank(EMPTY, L)
    if T > MAX_T:
        return _blank(TOO_LONG, L)
    if d4 == 0:
        m2, d4 = window_scale(x)
        if d4 == 0:
            return _blank(MAD_ZERO, L, m2, d4)
    if T < L:
        return _blank(NO_PATH, L, m2, d4)
    st = state_models(codes, model)
    S = L + 2
    zq = [quant(v, m2, d4) for v in x]
    V = [INF] * S
    V[0], V[1] = cost(zq[0], st[0]), cost(zq[0], st[1])
    bits = [[0] * S]
    for t in range(1, T):
        W, row = [INF] * S, [0] * S
        for s in range(min(t + 1, S - 1) + 1):
            best = V[s]
            if s > 0 and V[s - 1] < best:     # the advance only if STRICTLY smaller
                best, row[s] = V[s - 1], 1
            assert best < INF
            W[s] = cost(zq[t], st[s]) + best
        V = W
        bits.append(row)
    s = L + 1 if V[L + 1] < V[L] else L
    out = _blank(OK, L, m2, d4)
    out["score"] = V[s]
    _walk(lambda t, s: bits[t][s], T, L, s, t_lo, out)
    return _finish(out, raw, codes, model)


def align_numpy(raw, codes, model, t_lo=0, t_hi=None, m2=0, d4=0):
    """the int64 twin: a row at a time"""
    t_hi = len(raw) if t_hi is None else t_hi
    x = np.asarray(raw[t_lo:t_hi], dtype=np.int64)
    T, L = len(x), len(codes)
    if T == 0:
        return _blank(EMPTY, L)
    if T > MAX_T:
        return _blank(TOO_LONG, L)
    if d4 == 0:
        s = np.sort(x)
        m2 = int(s[(T - 1) // 2] + s[T // 2])
        d = np.sort(np.abs(2 * x - m2))
        d4 = int(d[(T - 1) // 2] + d[T // 2])
        if d4 == 0:
            return _blank(MAD_ZERO, L, m2, d4)
    if T < L:
        return _blank(NO_PATH, L, m2, d4)
    S = L + 2
    c = np.asarray(codes, dtype=np.int64)
    idx = np.zeros(L, dtype=np.int64)
    for j in range(-(model.k // 2), model.k // 2 + 1):
        idx = idx * 4 + (c[np.clip(np.arange(L) + j, 0, L - 1)] if L else c)
    tab = [np.asarray(a, dtype=np.int64) for a in (model.lvl, model.w, model.bias)]
    lvl, w, bias = (np.concatenate([[model.bg[i]], tab[i][idx], [model.bg[i]]]).astype(np.int64) for i in range(3))
    zq = np.clip(np.floor_divide(2 * 512 * (2 * x - m2) + d4, 2 * d4), -ZMAX, ZMAX)

    def costs(z):
        d = z - lvl
        return np.minimum((d * d * w) >> 32, CAP) + bias       # d^2 < 2^30, w < 2^32: below 2^62

    V = np.full(S, INF, dtype=np.int64)
    V[:2] = costs(zq[0])[:2]
    bp = np.zeros((T, (S + 7) // 8), dtype=np.uint8)
    adv = np.full(S, INF, dtype=np.int64)
    B = 256                                                    # rows whose costs are worked out at once
    for t0 in range(1, T, B):
        C = costs(zq[t0:t0 + B, None])
        took = np.zeros((len(C), S), dtype=bool)
        for i in range(len(C)):
            t = t0 + i
            adv[1:] = V[:-1]
            take = adv < V
            V = C[i] + np.where(take, adv, V)
            V[t + 2:] = INF                                    # cells with s > t + 1 are unreachable
            took[i] = take
        bp[t0:t0 + len(C)] = np.packbits(took, axis=1, bitorder="little")
    s = L + 1 if V[L + 1] < V[L] else L
    out = _blank(OK, L, m2, d4)
    out["score"] = int(V[s])
    _walk(lambda t, s: (int(bp[t, s >> 3]) >> (s & 7)) & 1, T, L, s, t_lo, out)
    return _finish_numpy(out, raw, idx, model)


def _finish_numpy(out, raw, idx, model):
    L = len(idx)
    if L == 0:
        return out
    x = np.asarray(raw, dtype=np.int64)
    first = np.asarray(out["first"], dtype=np.int64)
    ends = np.concatenate([first[1:], [out["last"][L - 1] + 1]])
    cs, cq = np.concatenate([[0], np.cumsum(x)]), np.concatenate([[0], np.cumsum(x * x)])
    out["start"], out["end"] = [int(v) for v in first], [int(v) for v in ends]
    sums, sq = cs[ends] - cs[first], cq[ends] - cq[first]
    out["sum"], out["sumsq"] = [int(v) for v in sums], [int(v) for v in sq]
    out["min"] = [int(v) for v in np.minimum.reduceat(x, first)]   # events are back to back: a segment ends where the next starts ...
    out["max"] = [int(v) for v in np.maximum.reduceat(x, first)]
    out["min"][L - 1], out["max"][L - 1] = int(x[first[L - 1]:ends[L - 1]].min()), int(x[first[L - 1]:ends[L - 1]].max())   # ... but the last
    l = np.asarray(model.lvl, dtype=np.int64)[idx]
    n = ends - first
    out["sums"] = [int(v) for v in (n.sum(), (n * l).sum(), (n * l * l).sum(), sums.sum(), (sums * l).sum())]
    return out


FIELDS = ("first", "last", "start", "end", "sum", "sumsq", "min", "max")


def assert_read_equal(res, r, want, what=""):
    """read r of a backend EvalResult against a restatement dict, every field"""
    assert int(res.status[r]) == want["status"], (what, r, "status", int(res.status[r]), want["status"])
    assert int(res.score[r]) == want["score"], (what, r, "score", int(res.score[r]), want["score"])
    assert (int(res.m2[r]), int(res.d4[r])) == (want["m2"], want["d4"]), (what, r, "scale", int(res.m2[r]), int(res.d4[r]), want["m2"], want["d4"])
    assert [int(v) for v in res.fit_sums[r]] == want["sums"], (what, r, "sums", list(res.fit_sums[r]), want["sums"])
    got = dict(first=res.first_step[r], last=res.last_step[r], start=res.events.start[r], end=res.events.end[r], sum=res.events.sum[r],
               sumsq=res.events.sumsq[r], min=res.events.min[r], max=res.events.max[r])
    for f in FIELDS:
        g = [int(v) for v in got[f]]
        if g != want[f]:
            bad = [i for i, (a, b) in enumerate(zip(g, want[f])) if a != b]
            raise AssertionError((what, r, f, len(g), len(want[f]), bad[:5], [g[i] for i in bad[:5]], [want[f][i] for i in bad[:5]]))


def as_ref_model(m):
    """a backend EvalModel as the restatement's Model"""
    return Model(m.k, m.lvl.tolist(), m.w.tolist(), m.bias.tolist(), m.bg)
