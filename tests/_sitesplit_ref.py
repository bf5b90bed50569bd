"""TEST INFRASTRUCTURE: the two-cluster split's contract (include/radian_hip.h, rd_site_split) restated in plain Python
over sorted lists, bisect and Python integers: they are unbounded, so the comparison of two scores by cross-multiplication is exact by
construction.  Nothing here is shared with the library: no key, no prefix array, no chunk.  numpy stands in for the lists in `split_deep`
only (a site of 2^16 events and more)."""
from bisect import bisect_right

import numpy as np

OK, ONE_SIDED, DEEP, TOO_LARGE, NONE = 0, 1, 2, 3, 4
DEEP_LIMIT = 1 << 16
FIELDS = ("out_site", "status", "n", "sum", "sumsq", "cut", "n_cuts", "n_lo", "sum_lo", "sumsq_lo")
DTYPES = {"out_site": np.uint32, "status": np.int32, "n": np.int64, "sum": np.int64, "sumsq": np.int64, "cut": np.int32, "n_cuts": np.int32,
          "n_lo": np.int64, "sum_lo": np.int64, "sumsq_lo": np.int64}
PAIRS = ("n", "sum", "sumsq", "n_lo", "sum_lo", "sumsq_lo")


def cuts(a, b, min_frac_q16):
    """[(cut, D, n_lo, n_hi)] of the admissible cuts of two lists of Python ints, ascending by cut"""
    pooled = sorted(a + b)
    N, total = len(pooled), sum(pooled)
    out = []
    for c in sorted(set(pooled))[:-1]:                    # every value present but the pooled maximum
        n_lo = bisect_right(pooled, c)
        n_hi = N - n_lo
        s_lo = sum(pooled[:n_lo])
        if n_lo >= 1 and n_hi >= 1 and 65536 * n_lo >= min_frac_q16 * N and 65536 * n_hi >= min_frac_q16 * N:
            out.append((c, s_lo * n_hi - (total - s_lo) * n_lo, n_lo, n_hi))
    return out


def best_cut(cands):
    """the candidate of the largest D^2 / (n_lo n_hi); ascending cuts and a strict comparison: the smallest cut among equals"""
    best = None
    for c in cands:
        if best is None or c[1] ** 2 * (best[2] * best[3]) > best[1] ** 2 * (c[2] * c[3]):
            best = c
    return best


def site_entry(site, a, b, min_frac_q16=0):
    """one site's output entry as a dict of Python ints and pairs; a / b: the values of sample 0 / 1 in any order"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    e = dict(out_site=site, status=OK, n=(len(a), len(b)), sum=(sum(a), sum(b)), sumsq=(sum(x * x for x in a), sum(x * x for x in b)), cut=0, n_cuts=0,
             n_lo=(0, 0), sum_lo=(0, 0), sumsq_lo=(0, 0))
    if not a or not b:
        e["status"] = ONE_SIDED
    elif len(a) + len(b) > DEEP_LIMIT:
        e["status"] = DEEP
    else:
        cands = cuts(a, b, min_frac_q16)
        if not cands:
            e["status"] = NONE
        else:
            cut = best_cut(cands)[0]
            lo = [[x for x in v if x <= cut] for v in (a, b)]
            e.update(cut=cut, n_cuts=len(cands), n_lo=tuple(len(v) for v in lo), sum_lo=tuple(sum(v) for v in lo),
                     sumsq_lo=tuple(sum(x * x for x in v) for v in lo))
    return e


def by_site(site, cond, value):
    """{site: ([values of sample 0], [values of sample 1])} in the events' order"""
    out = {}
    for s, c, v in zip(np.asarray(site).tolist(), np.asarray(cond).tolist(), np.asarray(value).tolist()):
        out.setdefault(s, ([], []))[c].append(v)
    return out


def split(site, cond, value, min_frac_q16=0):
    """the entries of rd_site_split, ascending by site, as a list of dicts"""
    groups = by_site(site, cond, value)
    return [site_entry(s, *groups[s], min_frac_q16) for s in sorted(groups)]


def split_deep(site, cond, value, min_frac_q16=0):
    """`split` for inputs with very deep sites: the same definitions through numpy.sort / cumsum for the counts and sums (int64 holds
    them: |S| <= 2^31), the scores and their comparison in Python integers"""
    site, cond, value = np.asarray(site), np.asarray(cond), np.asarray(value).astype(np.int64)
    out = []
    for s in np.unique(site).tolist():
        sel = site == s
        a, b = value[sel & (cond == 0)], value[sel & (cond == 1)]
        e = dict(out_site=s, status=OK, n=(len(a), len(b)), sum=(int(a.sum()), int(b.sum())), sumsq=(int((a * a).sum()), int((b * b).sum())), cut=0,
                 n_cuts=0, n_lo=(0, 0), sum_lo=(0, 0), sumsq_lo=(0, 0))
        N = len(a) + len(b)
        if not len(a) or not len(b):
            e["status"] = ONE_SIDED
        elif N > DEEP_LIMIT:
            e["status"] = DEEP
        else:
            pooled = np.sort(np.concatenate([a, b]))
            xs, first = np.unique(pooled, return_index=True)
            n_lo = np.append(first[1:], N)[:-1]                      # the values <= xs[i], for every value but the maximum
            s_lo = np.cumsum(pooled)[n_lo - 1]
            total = int(pooled.sum())
            cands = [(int(c), int(sl) * (N - int(nl)) - (total - int(sl)) * int(nl), int(nl), N - int(nl)) for c, nl, sl in zip(xs[:-1], n_lo, s_lo)
                     if 65536 * int(nl) >= min_frac_q16 * N and 65536 * (N - int(nl)) >= min_frac_q16 * N]
            if not cands:
                e["status"] = NONE
            else:
                cut = best_cut(cands)[0]
                lo = [v[v <= cut] for v in (a, b)]
                e.update(cut=cut, n_cuts=len(cands), n_lo=tuple(len(v) for v in lo), sum_lo=tuple(int(v.sum()) for v in lo),
                         sumsq_lo=tuple(int((v * v).sum()) for v in lo))
        out.append(e)
    return out


def as_arrays(entries):
    """the entries in the layout and dtypes of Backend.site_split's SplitResult: {field: array}"""
    return {f: np.array([e[f] for e in entries], dtype=DTYPES[f]).reshape((len(entries), 2) if f in PAIRS else (len(entries),)) for f in FIELDS}
