"""TEST INFRASTRUCTURE: the two-sample site comparison's contract (include/radian_hip.h, rd_site_compare) restated in
plain Python over sorted lists and bisect.  Nothing here is shared with the library: no key packing, no segment walk, no kernel constant
but the DEEP limit.  numpy.searchsorted stands in for bisect in `compare_deep` only (a site of 2^20 events and more)."""
from bisect import bisect_left, bisect_right

import numpy as np

OK, ONE_SIDED, DEEP, TOO_LARGE = 0, 1, 2, 3
DEEP_LIMIT = 1 << 20
FIELDS = ("out_site", "status", "n", "sum", "sumsq", "vmin", "vmax", "med2", "u2", "ks_num", "ks_x", "tie")
DTYPES = {"out_site": np.uint32, "status": np.int32, "n": np.int64, "sum": np.int64, "sumsq": np.int64, "vmin": np.int32, "vmax": np.int32,
          "med2": np.int32, "u2": np.int64, "ks_num": np.int64, "ks_x": np.int32, "tie": np.int64}


def status_of(n0, n1):
    return ONE_SIDED if n0 == 0 or n1 == 0 else DEEP if n0 + n1 > DEEP_LIMIT else OK


def _sample(v):
    """(n, sum, sumsq, min, max, med2) of one sorted sample; zeros when it is absent"""
    n = len(v)
    if n == 0:
        return 0, 0, 0, 0, 0, 0
    return n, sum(v), sum(x * x for x in v), v[0], v[-1], v[(n - 1) // 2] + v[n // 2]


def rank_fields(a, b):
    """(u2, ks_num, ks_x, tie) of two sorted, non-empty lists of Python ints"""
    n0, n1 = len(a), len(b)
    u2 = sum(2 * bisect_left(b, x) + (bisect_right(b, x) - bisect_left(b, x)) for x in a)
    ks_num, ks_x, tie = -1, None, 0
    for x in sorted(set(a) | set(b)):
        d = abs(bisect_right(a, x) * n1 - bisect_right(b, x) * n0)
        if d > ks_num:                      # ascending x and a strict comparison: the smallest x that attains the maximum
            ks_num, ks_x = d, x
        t = bisect_right(a, x) - bisect_left(a, x) + bisect_right(b, x) - bisect_left(b, x)
        tie += t ** 3 - t
    return u2, ks_num, ks_x, tie


def site_entry(site, a, b):
    """one site's output entry as a dict of Python ints and pairs; a / b: the values of sample 0 / 1 in any order"""
    a, b = sorted(int(x) for x in a), sorted(int(x) for x in b)
    sa, sb = _sample(a), _sample(b)
    st = status_of(len(a), len(b))
    u2, ks_num, ks_x, tie = rank_fields(a, b) if st == OK else (0, 0, 0, 0)
    return dict(out_site=site, status=st, n=(sa[0], sb[0]), sum=(sa[1], sb[1]), sumsq=(sa[2], sb[2]), vmin=(sa[3], sb[3]), vmax=(sa[4], sb[4]),
                med2=(sa[5], sb[5]), u2=u2, ks_num=ks_num, ks_x=ks_x, tie=tie)


def by_site(site, cond, value):
    """{site: ([values of sample 0], [values of sample 1])} in the events' order"""
    out = {}
    for s, c, v in zip(np.asarray(site).tolist(), np.asarray(cond).tolist(), np.asarray(value).tolist()):
        out.setdefault(s, ([], []))[c].append(v)
    return out


def compare(site, cond, value):
    """the entries of rd_site_compare, ascending by site, as a list of dicts"""
    groups = by_site(site, cond, value)
    return [site_entry(s, *groups[s]) for s in sorted(groups)]


def compare_deep(site, cond, value):
    """`compare` for inputs with very deep sites: the same definitions through numpy.sort / numpy.searchsorted and exact Python sums"""
    site, cond, value = np.asarray(site), np.asarray(cond), np.asarray(value).astype(np.int64)
    out = []
    for s in np.unique(site).tolist():
        sel = site == s
        a, b = np.sort(value[sel & (cond == 0)]), np.sort(value[sel & (cond == 1)])
        n0, n1 = len(a), len(b)
        st = status_of(n0, n1)
        e = dict(out_site=s, status=st, n=(n0, n1), u2=0, ks_num=0, ks_x=0, tie=0)
        for name, f in (("sum", lambda v: int(v.sum())), ("sumsq", lambda v: int((v * v).sum())), ("vmin", lambda v: int(v[0])),
                        ("vmax", lambda v: int(v[-1])), ("med2", lambda v: int(v[(len(v) - 1) // 2] + v[len(v) // 2]))):
            e[name] = tuple(f(v) if len(v) else 0 for v in (a, b))
        if st == OK:
            lb, ub = np.searchsorted(b, a, "left"), np.searchsorted(b, a, "right")
            e["u2"] = int((lb + ub).sum())
            xs = np.union1d(a, b)
            d = np.abs(np.searchsorted(a, xs, "right") * n1 - np.searchsorted(b, xs, "right") * n0)
            e["ks_num"], e["ks_x"] = int(d.max()), int(xs[int(np.argmax(d))])      # argmax: the first (smallest x) maximum
            t = (np.searchsorted(a, xs, "right") - np.searchsorted(a, xs, "left") + np.searchsorted(b, xs, "right") - np.searchsorted(b, xs, "left"))
            e["tie"] = sum(int(v) ** 3 - int(v) for v in t.tolist())
        out.append(e)
    return out


def as_arrays(entries):
    """the entries in the layout and dtypes of Backend.site_compare's SiteResult: {field: array}"""
    return {f: np.array([e[f] for e in entries], dtype=DTYPES[f]).reshape((len(entries), 2) if f in ("n", "sum", "sumsq", "vmin", "vmax", "med2")
                                                                          else (len(entries),)) for f in FIELDS}


def segments(site, cond, value):
    """(sorted keys as Python ints, [(site, start, split, end)]) of rd_site_diag_segments: events ordered by (site, cond, value)"""
    ev = sorted(zip(np.asarray(site).tolist(), np.asarray(cond).tolist(), np.asarray(value).tolist()))
    keys = [s * 131072 + c * 65536 + v + 32768 for s, c, v in ev]
    segs, i = [], 0
    while i < len(ev):
        j = i
        while j < len(ev) and ev[j][0] == ev[i][0]:
            j += 1
        split = i + sum(1 for e in ev[i:j] if e[1] == 0)
        segs.append((ev[i][0], i, split, j))
        i = j
    return keys, segs
