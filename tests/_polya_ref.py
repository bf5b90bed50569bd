"""Plain-Python restatement of the poly(A) flat-segment contract (include/radian_hip.h, rd_polya_segment): what
rd_polya_segment, rd_polya_segment_host and rd_polya_diag_windows are held to, for EQUALITY.  Loops over Python ints; sorted() for the order
statistics.  Nothing here is shared with the code under test.

A read of T int16 samples x; integer parameters win, flat_q, use_level, lo_q, hi_q, max_gap, min_samples, search_limit:
  scale     m2 = the sum of the two middle order statistics of x (ranks (T-1)//2 and T//2); d4 = the same of |2x - m2|.
            status, in this order: T == 0 EMPTY; d4 == 0 MAD_ZERO; T < win SHORT
  windows   nw = T // win; window j = x[j win : (j+1) win]; S = sum, Q = sum of squares, V = win Q - S^2
  flat      A = win flat_q d4; thr = min(A^2 // 2^20, 2^64 - 1); flat iff V <= thr and (not use_level or
            lo_q d4 win <= 512 (2 S - win m2) <= hi_q d4 win)
  segments  flat windows i < j with no flat window between them are joined iff j - i <= max_gap + 1; segment [a, b] is a candidate iff
            (b - a + 1) win >= min_samples and (search_limit == 0 or a win < search_limit)
  choice    the longest candidate (b - a + 1), the earliest on a tie
  outputs   status, tail_start = a win, tail_end = (b + 1) win, n_flat, sum / sumsq over x[tail_start : tail_end], m2, d4, n_candidates;
            not OK: -1, -1 and zeros, m2 and d4 whenever T > 0"""
OK, NONE, MAD_ZERO, SHORT, EMPTY, TOO_LARGE = 0, 1, 2, 3, 4, 5
FIELDS = ("status", "tail_start", "tail_end", "n_flat", "sum", "sumsq", "m2", "d4", "n_candidates")
PARAMS = ("win", "flat_q", "use_level", "lo_q", "hi_q", "max_gap", "min_samples", "search_limit")


def params(win=32, flat_q=46, use_level=0, lo_q=0, hi_q=0, max_gap=2, min_samples=None, search_limit=0):
    return dict(win=win, flat_q=flat_q, use_level=use_level, lo_q=lo_q, hi_q=hi_q, max_gap=max_gap,
                min_samples=win if min_samples is None else min_samples, search_limit=search_limit)


def middle2(values):
    s = sorted(values)
    return s[(len(s) - 1) // 2] + s[len(s) // 2]


def scale(x):
    """(m2, d4) of a non-empty read"""
    x = [int(v) for v in x]
    m2 = middle2(x)
    return m2, middle2([abs(2 * v - m2) for v in x])


def threshold(win, flat_q, d4):
    A = win * flat_q * d4
    return min(A * A >> 20, (1 << 64) - 1)


def windows(x, p):
    """(m2, d4, thr, [(S, Q, flat)] per window) of a non-empty read, whatever its status"""
    x = [int(v) for v in x]
    m2, d4 = scale(x)
    win = p["win"]
    thr = threshold(win, p["flat_q"], d4)
    out = []
    for j in range(len(x) // win):
        w = x[j * win:(j + 1) * win]
        S, Q = sum(w), sum(v * v for v in w)
        flat = win * Q - S * S <= thr
        if flat and p["use_level"]:
            flat = p["lo_q"] * d4 * win <= 512 * (2 * S - win * m2) <= p["hi_q"] * d4 * win
        out.append((S, Q, 1 if flat else 0))
    return m2, d4, thr, out


def segments_of(flags, max_gap):
    """[(a, b, n_flat)] of a list of 0/1 flags, in order"""
    segs = []
    for j, f in enumerate(flags):
        if not f:
            continue
        if segs and j - segs[-1][1] <= max_gap + 1:
            segs[-1][1] = j
            segs[-1][2] += 1
        else:
            segs.append([j, j, 1])
    return [tuple(s) for s in segs]


def segment(x, p):
    """the outputs of one read as a dict over FIELDS"""
    x = [int(v) for v in x]
    T, win = len(x), p["win"]
    out = dict(status=EMPTY, tail_start=-1, tail_end=-1, n_flat=0, sum=0, sumsq=0, m2=0, d4=0, n_candidates=0)
    if T == 0:
        return out
    m2, d4, thr, wins = windows(x, p)
    out["m2"], out["d4"] = m2, d4
    if d4 == 0:
        out["status"] = MAD_ZERO
        return out
    if T < win:
        out["status"] = SHORT
        return out
    cands = [(a, b, n) for a, b, n in segments_of([w[2] for w in wins], p["max_gap"])
             if (b - a + 1) * win >= p["min_samples"] and (p["search_limit"] == 0 or a * win < p["search_limit"])]
    out["n_candidates"] = len(cands)
    if not cands:
        out["status"] = NONE
        return out
    a, b, n = min(cands, key=lambda s: (-(s[1] - s[0] + 1), s[0]))
    tail = x[a * win:(b + 1) * win]
    out.update(status=OK, tail_start=a * win, tail_end=(b + 1) * win, n_flat=n, sum=sum(tail), sumsq=sum(v * v for v in tail))
    return out
