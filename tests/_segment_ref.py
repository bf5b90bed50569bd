"""The event-detection contract (include/radian_hip.h, rd_segment) restated twice, independently of the library:
`segment` in plain Python ints and lists, straight from the contract's text, and `segment_np`, a NumPy twin for larger reads (int64
prefix sums; the cross-multiplications pass 63 bits, so they run on object arrays of Python ints, one array operation per shift of the
suppression window).  Both return the same dict."""
import numpy as np

from _polya_ref import scale   # m2, d4 of a window: the order statistics rd_eventalign and rd_polya_segment share

OK, EMPTY, TOO_LONG, TOO_LARGE = 0, 1, 2, 3
MAX_T = 1 << 30
PARAMS = ("w1", "w2", "th1", "th2", "v0")
EVENT_FIELDS = ("start", "sum", "sumsq", "min", "max", "src")


def params(w1=4, w2=12, th1=144, th2=576, v0=1):
    return dict(w1=w1, w2=w2, th1=th1, th2=th2, v0=v0)


def params_ok(p):
    return 2 <= p["w1"] <= 32 and (p["w2"] == 0 or p["w1"] < p["w2"] <= 64) and 0 <= p["th1"] < (1 << 32) and 0 <= p["th2"] < (1 << 32) and 1 <= p["v0"] <= (1 << 16)


def max_events(T, w1):
    return T // (w1 + 1) + 1


def workspace_bytes(T, w1):
    return 8 * T + T // 32 + 32 * max_events(T, w1) + 8 * (T // 2048 + 1) + 8192


def event_row(total, n):
    """the row sigmap --events hands to rd_sigmap: the event's mean, rounded half up"""
    return (2 * total + n) // (2 * n)


# ------------------------------------------------------------------------------------------------------------------ plain
def tstat(x, w, v0):
    """N, D of every sample for a detector of window w (w == 0: the detector is off)"""
    T = len(x)
    N, D = [0] * T, [1] * T
    if w == 0:
        return N, D
    for i in range(w, T - w + 1):
        a, b = [int(v) for v in x[i - w:i]], [int(v) for v in x[i:i + w]]
        S1, Q1, S2, Q2 = sum(a), sum(v * v for v in a), sum(b), sum(v * v for v in b)
        N[i] = w * (S1 - S2) ** 2
        D[i] = w * Q1 - S1 ** 2 + w * Q2 - S2 ** 2 + 2 * w * w * v0
    return N, D


def peaks(N, D, w, th):
    T = len(N)
    out = [0] * T
    if w == 0:
        return out
    for i in range(T):
        if not (N[i] > 0 and 16 * N[i] >= th * D[i]):
            continue
        before = all(N[j] * D[i] < N[i] * D[j] for j in range(max(i - w, 0), i))
        behind = all(N[j] * D[i] <= N[i] * D[j] for j in range(i + 1, min(i + w, T - 1) + 1))
        out[i] = int(before and behind)
    return out


def flags(x, p):
    """per sample bit 0: peak of detector 1, bit 1: peak of detector 2; and the (N, D) lists of both detectors"""
    t1, t2 = tstat(x, p["w1"], p["v0"]), tstat(x, p["w2"], p["v0"])
    k1, k2 = peaks(*t1, p["w1"], p["th1"]), peaks(*t2, p["w2"], p["th2"])
    return [a | (b << 1) for a, b in zip(k1, k2)], (t1, t2)


def boundaries(fl, w2):
    """[(sample, detector)]"""
    T = len(fl)
    out = []
    for i in range(T):
        if fl[i] & 1:
            out.append((i, 1))
        elif fl[i] & 2 and not any(fl[j] & 1 for j in range(max(i - w2 + 1, 0), min(i + w2 - 1, T - 1) + 1)):
            out.append((i, 2))
    return out


def _events(x, starts, srcs):
    T = len(x)
    ev = {f: [] for f in EVENT_FIELDS}
    for k, s in enumerate(starts):
        seg = [int(v) for v in x[s:(starts[k + 1] if k + 1 < len(starts) else T)]]
        for f, v in zip(EVENT_FIELDS, (s, sum(seg), sum(v * v for v in seg), min(seg), max(seg), srcs[k])):
            ev[f].append(v)
    return ev


def segment(x, p, scale_window=None):
    """-> dict(status, n_events, m2, d4, start, sum, sumsq, min, max, src)"""
    T = len(x)
    out = dict(status=EMPTY if T == 0 else TOO_LONG if T > MAX_T else OK, n_events=0, m2=0, d4=0, **{f: [] for f in EVENT_FIELDS})
    if out["status"] != OK:
        return out
    if scale_window is not None and scale_window[1] > scale_window[0]:
        out["m2"], out["d4"] = scale(x[scale_window[0]:scale_window[1]])
    b = boundaries(flags(x, p)[0], p["w2"])
    out.update(_events(x, [0] + [i for i, _ in b], [0] + [d for _, d in b]))
    out["n_events"] = len(out["start"])
    return out


# ------------------------------------------------------------------------------------------------------------------ NumPy twin
def tstat_np(x, w, v0):
    T = len(x)
    N, D = np.zeros(T, np.int64), np.ones(T, np.int64)
    if w == 0 or T < 2 * w:
        return N, D
    v = np.asarray(x, np.int64)
    P, PQ = np.concatenate([[0], np.cumsum(v)]), np.concatenate([[0], np.cumsum(v * v)])
    i = np.arange(w, T - w + 1)
    S1, S2, Q1, Q2 = P[i] - P[i - w], P[i + w] - P[i], PQ[i] - PQ[i - w], PQ[i + w] - PQ[i]
    N[i] = w * (S1 - S2) ** 2
    D[i] = w * Q1 - S1 * S1 + w * Q2 - S2 * S2 + 2 * w * w * v0
    return N, D


def peaks_np(N, D, w, th):
    T = len(N)
    if w == 0 or T == 0:
        return np.zeros(T, bool)
    No, Do = N.astype(object), D.astype(object)
    keep = (N > 0) & np.array(16 * No >= th * Do, dtype=bool)
    for d in range(1, min(w, T - 1) + 1):
        # j = i - d must be strictly below, j = i + d not above
        keep[d:] &= np.array(No[:-d] * Do[d:] < No[d:] * Do[:-d], dtype=bool)        # t(i - d) < t(i), i = d .. T - 1
        keep[:T - d] &= np.array(No[d:] * Do[:-d] <= No[:-d] * Do[d:], dtype=bool)   # t(i + d) <= t(i), i = 0 .. T - d - 1
    return keep


def segment_np(x, p, scale_window=None):
    T = len(x)
    out = dict(status=EMPTY if T == 0 else TOO_LONG if T > MAX_T else OK, n_events=0, m2=0, d4=0, **{f: [] for f in EVENT_FIELDS})
    if out["status"] != OK:
        return out
    if scale_window is not None and scale_window[1] > scale_window[0]:
        out["m2"], out["d4"] = scale(x[scale_window[0]:scale_window[1]])
    k1 = np.flatnonzero(peaks_np(*tstat_np(x, p["w1"], p["v0"]), p["w1"], p["th1"]))
    k2 = np.flatnonzero(peaks_np(*tstat_np(x, p["w2"], p["v0"]), p["w2"], p["th2"]))
    if len(k1) and len(k2):
        at = np.searchsorted(k1, k2)
        near = np.minimum(np.abs(k1[np.clip(at, 0, len(k1) - 1)] - k2), np.abs(k1[np.clip(at - 1, 0, len(k1) - 1)] - k2))
        k2 = k2[near >= p["w2"]]
    starts = np.concatenate([[0], k1, k2]).astype(np.int64)
    srcs = np.concatenate([[0], np.full(len(k1), 1), np.full(len(k2), 2)]).astype(np.int64)
    order = np.argsort(starts, kind="stable")
    starts, srcs = starts[order], srcs[order]
    v = np.asarray(x, np.int64)
    out.update(start=starts.tolist(), src=srcs.tolist(), sum=np.add.reduceat(v, starts).tolist(), sumsq=np.add.reduceat(v * v, starts).tolist(),
               min=np.minimum.reduceat(v, starts).tolist(), max=np.maximum.reduceat(v, starts).tolist(), n_events=len(starts))
    return out
