"""The banded eventalign contract (include/radian_hip.h, rd_eventalign_banded) restated from its text: a plain-Python version (Python
ints and lists: the window, the two masked predecessors, the strict tie-break, OFF_BAND, n_edge) and a NumPy int64 twin for the large
cases.  What the contract takes over from rd_eventalign unchanged (the sample rule, the cost, the k-mer rule, the walk, the events) is
_eventalign_ref's restatement of it.  Nothing here shares code with the library or with radian_amd.eventalign."""
import numpy as np

import _eventalign_ref as ref
from _eventalign_ref import EMPTY, INF, MAD_ZERO, MAX_T, NO_PATH, OK, TOO_LARGE, TOO_LONG   # noqa: F401

OFF_BAND = 6
W = 64
FINITE = 3 << 28


def lo_of(g, L):
    """the window's lowest state where g bases have guide <= the row's sample"""
    return min(max(g - 31, 0), max(L + 2 - W, 0))


def window_rows(guide, L, t_lo, T):
    """lo(t) for t in 0 .. T - 1: g(t) = #{b : guide[b] <= t_lo + t}"""
    out, g = [], 0
    for t in range(T):
        while g < L and int(guide[g]) <= t_lo + t:
            g += 1
        out.append(lo_of(g, L))
    return out


def _blank(status, L, m2=0, d4=0):
    return dict(ref._blank(status, L, m2, d4), n_edge=0)


def _head(x, L, m2, d4, scale):
    """the statuses before any row -> (a blank output or None, m2, d4)"""
    T = len(x)
    if T == 0:
        return _blank(EMPTY, L), m2, d4
    if T > MAX_T:
        return _blank(TOO_LONG, L), m2, d4
    if d4 == 0:
        m2, d4 = scale(x)
        if d4 == 0:
            return _blank(MAD_ZERO, L, m2, d4), m2, d4
    if T < L:
        return _blank(NO_PATH, L, m2, d4), m2, d4
    return None, m2, d4


def _end(v_trail, v_last):
    s_is_trail = v_trail < v_last
    return s_is_trail, (v_trail if s_is_trail else v_last)


def _edges(out, lo, L, t_lo):
    return sum(1 for b in range(L) if lo[out["last"][b] - t_lo] == b + 1 or lo[out["first"][b] - t_lo] + W - 1 == b + 1)


def align_plain(raw, codes, guide, model, t_lo=0, t_hi=None, m2=0, d4=0):
    """one read, Python ints and lists only -> dict of every output field"""
    t_hi = len(raw) if t_hi is None else t_hi
    x = [int(v) for v in raw[t_lo:t_hi]]
    T, L = len(x), len(codes)
    assert len(guide) == L and all(int(guide[b]) <= int(guide[b + 1]) for b in range(L - 1))
    out, m2, d4 = _head(x, L, m2, d4, ref.window_scale)
    if out is not None:
        return out
    st = ref.state_models(codes, model)
    S = L + 2
    zq = [ref.quant(v, m2, d4) for v in x]
    lo = window_rows(guide, L, t_lo, T)
    win = [range(lo[t], min(lo[t] + W - 1, S - 1) + 1) for t in range(T)]
    V = {s: (ref.cost(zq[0], st[s]) if s <= 1 else INF) for s in win[0]}     # a state outside the row's window has no entry
    bits = [{}]
    for t in range(1, T):
        Wn, row = {}, {}
        for s in win[t]:
            stay = V.get(s, INF)                                             # s in win(t-1), else 2^30
            adv = V.get(s - 1, INF) if s - 1 >= lo[t] else INF               # s - 1 >= lo(t) and in win(t-1), else 2^30
            best, row[s] = stay, 0
            if adv < stay:                                                   # the advance only if STRICTLY smaller
                best, row[s] = adv, 1
            Wn[s] = ref.cost(zq[t], st[s]) + best
            assert Wn[s] <= (5 << 27) or (7 << 27) <= Wn[s] < (1 << 31)      # finite up to 0.625 2^30, or from 0.875 2^30 to 2^31
        V = Wn
        bits.append(row)
    trail, end = _end(V.get(L + 1, INF), V.get(L, INF))
    if end >= FINITE:
        return _blank(OFF_BAND, L, m2, d4)
    out = _blank(OK, L, m2, d4)
    out["score"] = end
    ref._walk(lambda t, s: bits[t][s], T, L, L + 1 if trail else L, t_lo, out)
    out["n_edge"] = _edges(out, lo, L, t_lo)
    return ref._finish(out, raw, codes, model)


def align_numpy(raw, codes, guide, model, t_lo=0, t_hi=None, m2=0, d4=0):
    """the int64 twin: a row at a time over the 64 states of the row's window"""
    t_hi = len(raw) if t_hi is None else t_hi
    x = np.asarray(raw[t_lo:t_hi], dtype=np.int64)
    T, L = len(x), len(codes)

    def scale(x):
        s = np.sort(x)
        m2 = int(s[(T - 1) // 2] + s[T // 2])
        d = np.sort(np.abs(2 * x - m2))
        return m2, int(d[(T - 1) // 2] + d[T // 2])

    out, m2, d4 = _head(x, L, m2, d4, scale)
    if out is not None:
        return out
    S = L + 2
    c = np.asarray(codes, dtype=np.int64)
    idx = np.zeros(L, dtype=np.int64)
    for j in range(-(model.k // 2), model.k // 2 + 1):
        idx = idx * 4 + (c[np.clip(np.arange(L) + j, 0, L - 1)] if L else c)
    tab = [np.asarray(a, dtype=np.int64) for a in (model.lvl, model.w, model.bias)]
    pad = np.zeros(W, dtype=np.int64)                                        # states past L + 1 do not exist: their values stay 2^30 + 0
    lvl, w, bias = (np.concatenate([[model.bg[i]], tab[i][idx], [model.bg[i]], pad]).astype(np.int64) for i in range(3))
    zq = np.clip(np.floor_divide(2 * 512 * (2 * x - m2) + d4, 2 * d4), -ref.ZMAX, ref.ZMAX)
    g = np.searchsorted(np.asarray(guide, dtype=np.int64), t_lo + np.arange(T, dtype=np.int64), side="right")
    lo = np.minimum(np.maximum(g - 31, 0), max(S - W, 0))
    assert (np.diff(lo) >= 0).all()
    # full[s] holds V of state s where s is in the current window; everything else is 2^30 (left behind, or not yet reached)
    full = np.full(S + 2 * W, INF, dtype=np.int64)
    l0 = int(lo[0])
    d0 = zq[0] - lvl[:2]
    first_costs = np.minimum((d0 * d0 * w[:2]) >> 32, ref.CAP) + bias[:2]
    for s in (0, 1):
        if l0 <= s <= min(l0 + W - 1, S - 1):
            full[s] = first_costs[s]
    bp = np.zeros(T, dtype=np.uint64)
    prev = l0
    for t in range(1, T):
        a = int(lo[t])
        if a != prev:
            full[prev:a] = INF                                               # a state that has left the window is gone at once
            prev = a
        hi = min(a + W, S)                                                   # states a .. hi - 1
        cur = full[a:hi]
        adv = np.empty_like(cur)
        adv[0] = INF                                                         # the window's lowest state has no advance edge
        adv[1:] = cur[:-1]
        take = adv < cur
        d = zq[t] - lvl[a:hi]
        full[a:hi] = np.minimum((d * d * w[a:hi]) >> 32, ref.CAP) + bias[a:hi] + np.where(take, adv, cur)
        rot = (np.arange(a, hi) & (W - 1)).astype(np.uint64)
        bp[t] = np.bitwise_or.reduce(np.where(take, np.uint64(1) << rot, np.uint64(0))) if hi > a else 0
    a = int(lo[T - 1])
    in_win = lambda s: a <= s <= min(a + W - 1, S - 1)
    trail, end = _end(int(full[L + 1]) if in_win(L + 1) else INF, int(full[L]) if in_win(L) else INF)
    if end >= FINITE:
        return _blank(OFF_BAND, L, m2, d4)
    out = _blank(OK, L, m2, d4)
    out["score"] = end
    ref._walk(lambda t, s: (int(bp[t]) >> (s & (W - 1))) & 1, T, L, L + 1 if trail else L, t_lo, out)
    out["n_edge"] = _edges(out, [int(v) for v in lo], L, t_lo)
    return ref._finish_numpy(out, raw, idx, model)


def interior(first, last, L, guide, t_lo, T):
    """the identity's condition on a full-DP path given by its steps: at every row lo(t) == 0 or s(t) > lo(t), and s(t) <= lo(t) + 63"""
    t = t_lo + np.arange(T, dtype=np.int64)
    g = np.searchsorted(np.asarray(guide, dtype=np.int64), t, side="right")
    lo = np.minimum(np.maximum(g - 31, 0), max(L + 2 - W, 0))
    if L:
        s = np.searchsorted(np.asarray(first, dtype=np.int64), t, side="right")
        s = np.where(t > last[L - 1], L + 1, s)
    else:
        s = np.zeros(T, dtype=np.int64)    # (lead and trail are one background: no step tells them apart, and L + 2 <= 64 anyway)
    return bool((((lo == 0) | (s > lo)) & (s <= lo + W - 1)).all())


def assert_read_equal(res, r, want, what=""):
    """read r of a backend EvalBandedResult against a restatement dict, every field"""
    ref.assert_read_equal(res, r, want, what)
    assert int(res.n_edge[r]) == want["n_edge"], (what, r, "n_edge", int(res.n_edge[r]), want["n_edge"])
