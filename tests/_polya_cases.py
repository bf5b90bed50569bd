"""The seeded cases of the poly(A) tests (tests/test_polya_cpu.py asserts every case's defining condition without a GPU;
tests/test_gpu_polya.py runs them on the device).  A GROUP is a set of reads that share one parameter set (one call):
{"name", "p": _polya_ref.params(...), "reads": [int16 arrays], "flags": [designed 0/1 window flags or None], "cond": {read index:
callable(out, wins) -> bool}} where out is _polya_ref.segment's dict and wins _polya_ref.windows' list.

read_from_flags builds a read whose window flags are GIVEN: a flat window is constant (V = 0) at a level of its own, a non-flat window
alternates level +- 4000 (sd 4000, far above flat_q / 256 MAD for the flat_q used here); the levels differ from window to window, so
the read's MAD is not zero whatever the pattern."""
import numpy as np

import _polya_ref as ref

SEG_CHUNK = 256   # windows per chunk of the segment kernel's sweep (polya.hip PA_SEG)


def read_from_flags(flags, win, rng, rem=0):
    out = np.empty(len(flags) * win + rem, dtype=np.int16)
    alt = np.where(np.arange(win) % 2 == 0, -4000, 4000)
    for j, f in enumerate(flags):
        level = int(rng.integers(-2000, 2001))
        out[j * win:(j + 1) * win] = level if f else level + alt
    out[len(flags) * win:] = rng.integers(-2000, 2001, rem)
    return out


def _runs(*parts):
    """flags from (flag, count) runs"""
    return [f for f, n in parts for _ in range(n)]


def shape_group():
    """window counts around the window kernel's block (64) and the segment kernel's chunk (256), a long read, the short and degenerate
    reads -- one parameter set, so the whole group is also the batch of the grouping test"""
    rng = np.random.default_rng(71)
    win = 8
    p = ref.params(win=win, max_gap=1, min_samples=2 * win)
    reads, flags, cond = [], [], {}

    def add(x, fl=None, c=None):
        if c is not None:
            cond[len(reads)] = c
        reads.append(np.ascontiguousarray(x, dtype=np.int16))
        flags.append(fl)

    add(rng.integers(-500, 500, win), None, lambda o, w: o["status"] in (ref.OK, ref.NONE) and len(w) == 1)            # T = win
    add(np.zeros(0), None, lambda o, w: o["status"] == ref.EMPTY and o["m2"] == 0)                                      # T = 0 (EMPTY between good ones)
    add(rng.integers(-500, 500, win - 1), None, lambda o, w: o["status"] == ref.SHORT and o["d4"] > 0 and len(w) == 0)  # T = win - 1
    add(rng.integers(-500, 500, 2 * win - 1), None, lambda o, w: len(w) == 1)                                           # T = 2 win - 1
    for nw in (63, 64, 65, 255, 256, 257, 5003):
        fl = [int(v) for v in rng.random(nw) < 0.55]
        add(read_from_flags(fl, win, rng, rem=int(rng.integers(0, win))), fl,
            lambda o, w, nw=nw: len(w) == nw and o["status"] == ref.OK and o["n_candidates"] > 1)
        if nw == 64:
            add(np.full(100, 77), None, lambda o, w: o["status"] == ref.MAD_ZERO and o["m2"] == 154 and o["d4"] == 0)   # MAD_ZERO between good ones
    # a segment that straddles the first chunk boundary of the segment kernel, a longer one over the second, sparse flats elsewhere
    fl = _runs((0, 100), (1, 1), (0, 149), (1, 12), (0, 238), (1, 30), (0, 70))
    add(read_from_flags(fl, win, rng), fl,
        lambda o, w: (o["tail_start"], o["tail_end"]) == (500 * win, 530 * win) and o["n_candidates"] == 2 and 500 < 2 * SEG_CHUNK < 530 and 250 < SEG_CHUNK < 262)
    # ... and the one over the first boundary is chosen when it is the longer
    fl = _runs((0, 250), (1, 12), (0, 238), (1, 5), (0, 95))
    add(read_from_flags(fl, win, rng), fl, lambda o, w: (o["tail_start"], o["tail_end"], o["n_flat"]) == (250 * win, 262 * win, 12))
    # one segment from window 0 to window nw - 1, held together by gaps of exactly max_gap (301 windows: over a chunk boundary)
    fl = [1, 0] * 150 + [1]
    add(read_from_flags(fl, win, rng), fl,
        lambda o, w: (o["tail_start"], o["tail_end"], o["n_candidates"], o["n_flat"]) == (0, 301 * win, 1, 151) and len(w) == 301)
    return {"name": "shapes", "p": p, "reads": reads, "flags": flags, "cond": cond}


def gap_groups():
    """a gap of exactly max_gap (merged) and of max_gap + 1 (split); two candidates of equal length; search_limit at a win = limit - 1
    and a win = limit; min_samples met exactly and missed by one window"""
    rng = np.random.default_rng(72)
    win, g = 16, 3
    out = []
    merged = _runs((0, 4), (1, 3), (0, g), (1, 3), (0, 5))
    split = _runs((0, 4), (1, 3), (0, g + 1), (1, 4), (0, 5))
    out.append({"name": "gap", "p": ref.params(win=win, max_gap=g, min_samples=3 * win),
                "reads": [read_from_flags(merged, win, rng, 5), read_from_flags(split, win, rng, 0)], "flags": [merged, split],
                "cond": {0: lambda o, w: (o["tail_start"], o["tail_end"], o["n_flat"], o["n_candidates"]) == (4 * win, (10 + g) * win, 6, 1),
                         1: lambda o, w: (o["tail_start"], o["tail_end"], o["n_flat"], o["n_candidates"]) == ((8 + g) * win, (12 + g) * win, 4, 2)}})
    tie = _runs((0, 2), (1, 5), (0, 9), (1, 5), (0, 3), (1, 4), (0, 1))
    out.append({"name": "tie", "p": ref.params(win=win, max_gap=0, min_samples=win), "reads": [read_from_flags(tie, win, rng, 3)], "flags": [tie],
                "cond": {0: lambda o, w: (o["tail_start"], o["tail_end"], o["n_candidates"]) == (2 * win, 7 * win, 3)}})
    lim = _runs((0, 3), (1, 4), (0, 6), (1, 9), (0, 2))    # segments at windows 3 (4 long) and 13 (9 long)
    x = read_from_flags(lim, win, rng, 1)
    for name, limit, want in (("limit-in", 13 * win + 1, (13 * win, 22 * win, 2)), ("limit-out", 13 * win, (3 * win, 7 * win, 1))):
        out.append({"name": name, "p": ref.params(win=win, max_gap=0, min_samples=win, search_limit=limit), "reads": [x], "flags": [lim],
                    "cond": {0: lambda o, w, want=want: (o["tail_start"], o["tail_end"], o["n_candidates"]) == want}})
    for name, ms, want in (("min-met", 9 * win, (ref.OK, 1)), ("min-missed", 10 * win, (ref.NONE, 0))):
        out.append({"name": name, "p": ref.params(win=win, max_gap=0, min_samples=ms), "reads": [x], "flags": [lim],
                    "cond": {0: lambda o, w, want=want: (o["status"], o["n_candidates"]) == want and (o["tail_end"] == -1) == (want[0] == ref.NONE)}})
    return out


def _spread(w, win):
    return win * sum(int(v) ** 2 for v in w) - sum(int(v) for v in w) ** 2


def threshold_groups():
    """V == thr and V == thr + 1 in one read (found by a search); 2^64 <= A^2 < 2^84; the largest A the ranges allow and the largest V
    (samples alternating -32768 / 32767 at win = 256); both level-band bounds at equality.
    A^2 >= 2^84 cannot be reached through the C ABI: A <= 256 * 32767 * 262142 < 2^41 (test_polya_cpu asserts the bound); the saturation
    of the threshold rule itself is exercised by tests/asan_polya.cpp, which calls it directly."""
    out = []
    # ---- V == thr, V == thr + 1.  win = 8: V = 8 sum e^2 - (sum e)^2 for offsets e from the window's level, so V is 0, 4 or 7 mod 8 and the
    # pair (thr, thr + 1) needs thr = 7 mod 8.  Windows 0 and 1 sit at level 20000, far above median + MAD: their offsets change no order statistic
    win = 8
    a, b, c = np.meshgrid(np.arange(0, 81), np.arange(-120, 121), np.arange(-120, 121), indexing="ij")
    V = (8 * (a * a + b * b + c * c) - (a + b + c) ** 2).ravel()
    order = np.argsort(V, kind="stable")
    Vs = V[order]
    found = None
    for seed in range(100, 160):
        rng = np.random.default_rng(seed)
        fl = [1, 1] + [0] * 38
        x = read_from_flags(fl, win, rng, 0)
        x[:2 * win] = 20000
        m2, d4 = ref.scale(x)
        for flat_q in range(1, 6):
            thr = ref.threshold(win, flat_q, d4)
            i0, i1 = np.searchsorted(Vs, thr), np.searchsorted(Vs, thr + 1)
            if thr % 8 == 7 and i0 < len(Vs) and Vs[i0] == thr and i1 < len(Vs) and Vs[i1] == thr + 1:
                found = (x, flat_q, thr, [np.unravel_index(order[i], a.shape) for i in (i0, i1)])
                break
        if found:
            break
    assert found, "no (seed, flat_q) with thr and thr + 1 both representable"
    x, flat_q, thr, idx = found
    for k, (ia, ib, ic) in enumerate(idx):
        x[k * win: k * win + 3] += np.array([ia, ib - 120, ic - 120], dtype=np.int16)
    out.append({"name": "v-equals-thr", "p": ref.params(win=win, flat_q=flat_q, max_gap=0, min_samples=win), "reads": [x], "flags": [[1] + [0] * 39],
                "cond": {0: lambda o, w, thr=thr, x=x: _spread(x[:win], win) == thr and _spread(x[win:2 * win], win) == thr + 1 and
                         ref.threshold(win, flat_q, o["d4"]) == thr and (o["tail_start"], o["tail_end"]) == (0, win)}})
    # ---- the high word of A^2 is non-zero and thr does not saturate: win 256, flat_q 32767, 512 <= d4 < 1024; one window of the largest V
    rng = np.random.default_rng(73)
    x = np.round(rng.normal(100, 280, 9 * 256 + 17)).astype(np.int16)
    x[3 * 256:4 * 256] = np.where(np.arange(256) % 2 == 0, -32768, 32767)
    out.append({"name": "a2-high-word", "p": ref.params(win=256, flat_q=32767, max_gap=0, min_samples=256), "reads": [x], "flags": [[1, 1, 1, 0, 1, 1, 1, 1, 1]],
                "cond": {0: lambda o, w: (1 << 64) <= (256 * 32767 * o["d4"]) ** 2 < (1 << 84) and 256 * w[3][1] - w[3][0] ** 2 > (1 << 45)
                         and (o["tail_start"], o["tail_end"]) == (4 * 256, 9 * 256)}})
    # ---- the largest V everywhere, and the largest A such a read gives (A^2 about 2^80: the quotient still fits)
    x = np.where(np.arange(5 * 256 + 4) % 2 == 0, -32768, 32767).astype(np.int16)   # (T even: m2 = -1, d4 = 2 * 65535)
    out.append({"name": "largest-v", "p": ref.params(win=256, flat_q=32767, max_gap=0, min_samples=256), "reads": [x], "flags": [[1] * 5],
                "cond": {0: lambda o, w: o["d4"] == 131070 and all(256 * q - s * s == 256 * 128 * (32768 ** 2 + 32767 ** 2) - 128 ** 2 for s, q, _ in w)
                         and (256 * 32767 * o["d4"]) ** 2 >> 20 < (1 << 64) and o["tail_end"] == 5 * 256}})
    # ---- the level band at equality.  T odd, so m2 is even; window 0 is constant at c = m2 / 2 + d4 (median + 4 MAD, above median + MAD as
    # its placeholder was): 512 (2 S - win m2) = 512 * 16 * d4 = 1024 d4 win
    rng = np.random.default_rng(74)
    fl = [1] + [int(v) for v in rng.random(40) < 0.5]
    x = read_from_flags(fl, win, rng, 1)
    x[:win] = 20000
    m2, d4 = ref.scale(x)
    assert m2 % 2 == 0 and m2 // 2 + d4 < 20000
    x[:win] = m2 // 2 + d4
    eq = lambda o, w, m2=m2, d4=d4: (o["m2"], o["d4"]) == (m2, d4) and 512 * (2 * w[0][0] - win * m2) == 1024 * d4 * win
    for name, lo, hi, hit in (("level-both-equal", 1024, 1024, True), ("level-lo-above", 1025, 4096, False), ("level-hi-below", -4096, 1023, False)):
        flags = [1 if (j == 0 and hit) else 0 for j in range(41)]
        if not hit:   # the other flat windows may fall inside the wider band: take the flags from the restatement's level rule, asserted on window 0
            flags = None
        out.append({"name": name, "p": ref.params(win=win, use_level=1, lo_q=lo, hi_q=hi, max_gap=0, min_samples=win), "reads": [x], "flags": [flags],
                    "cond": {0: lambda o, w, hit=hit, eq=eq: eq(o, w) and w[0][2] == int(hit) and (not hit or (o["tail_start"], o["tail_end"]) == (0, win))}})
    return out


def all_groups():
    return [shape_group()] + gap_groups() + threshold_groups()


def refusal_cases():
    """(good keyword arguments, [(name, keyword arguments)]) of raw_call: every argument refusal of rd_polya_segment / _host"""
    good = dict(raw=np.arange(40, dtype=np.int16), off=[0, 40], p=ref.params(win=8))
    bad = [("null raw", dict(good, raw=None)), ("null offsets", dict(good, off=None)), ("null output", dict(good, null_out=4)),
           ("negative n_reads", dict(good, n_reads=-1)), ("negative offset", dict(good, off=[-1, 40])),
           ("offsets not monotone", dict(good, raw=np.arange(80, dtype=np.int16), off=[0, 50, 40]))]
    for name, kw in (("win 7", dict(win=7)), ("win 257", dict(win=257, min_samples=257)), ("flat_q 0", dict(flat_q=0)), ("flat_q 32768", dict(flat_q=32768)),
                     ("use_level 2", dict(use_level=2)), ("lo_q below", dict(lo_q=-(1 << 20) - 1)), ("hi_q above", dict(hi_q=(1 << 20) + 1)),
                     ("lo_q > hi_q", dict(lo_q=5, hi_q=4)), ("max_gap -1", dict(max_gap=-1)), ("max_gap 1025", dict(max_gap=1025)),
                     ("min_samples < win", dict(min_samples=7)), ("search_limit -1", dict(search_limit=-1))):
        bad.append((name, dict(good, p=dict(ref.params(win=8), **kw))))
    return good, bad


def raw_call(fn, raw, off, p, n_reads=None, null_out=None, outs=None, budget=None):
    """fn(raw, off, n_reads, params..., [budget], nine outputs) on exact buffers; -> return code (outs: the nine arrays to use)"""
    import ctypes
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    off_a = None if off is None else np.asarray(off, dtype=np.int64)
    n = (len(off) - 1 if off is not None else 1) if n_reads is None else n_reads
    if outs is None:
        outs = [np.zeros(max(n, 1), dtype=np.int64 if f in ("tail_start", "tail_end", "sum", "sumsq") else np.int32) for f in ref.FIELDS]
    ptrs = [None if null_out == i else ptr(o) for i, o in enumerate(outs)]
    args = [p[k] for k in ref.PARAMS] + ([budget] if budget is not None else [])
    return fn(ptr(raw), ptr(off_a), n, *args, *ptrs)


def same(got, r, exp, fields=ref.FIELDS):
    for f in fields:
        assert int(getattr(got, f)[r]) == exp[f], (f, r, int(getattr(got, f)[r]), exp[f])
