"""The seeded cases of the event-detection tests (tests/test_segment_cpu.py asserts every case's defining condition without a GPU;
tests/test_gpu_segment.py runs them on the device).  A GROUP is a set of reads that share one parameter set (one call):
{"name", "p": _segment_ref.params(...), "reads": [int16 arrays], "cond": {read index: callable(out, x) -> bool}} where out is
_segment_ref.segment's dict.

The peak kernel takes tiles of TILE samples of one read and recomputes a halo: a peak at i reads t to i +- w and samples to i +- 2 w."""
import numpy as np

import _segment_ref as ref

TILE = 2048   # samples per workgroup of the peak kernel (segment.hip SG_TILE)


def levels(rng, T, dwell=(8, 40), span=300, noise=4):
    """a piecewise constant signal with uniform noise"""
    n = T // dwell[0] + 2
    lv = np.repeat(rng.integers(-span, span + 1, n), rng.integers(dwell[0], dwell[1] + 1, n))[:T]
    return (lv + rng.integers(-noise, noise + 1, T)).astype(np.int16)


def steps_at(T, at, rng, height=400, noise=3):
    """level 0 with noise, raised by `height` from every second position of `at` to the next"""
    x = rng.integers(-noise, noise + 1, T).astype(np.int64)
    edges = list(at) + [T]
    for k in range(0, len(at), 2):
        x[edges[k]:edges[k + 1]] += height
    return x.astype(np.int16)


def _group(name, p, items):
    return {"name": name, "p": p, "reads": [np.ascontiguousarray(x, dtype=np.int16) for x, _ in items],
            "cond": {r: c for r, (_, c) in enumerate(items) if c is not None}}


def length_group():
    """T = 0, 1, 2 w1 - 1, 2 w1, 2 w1 + 1 with a step in the middle; T around one and two tiles; mixed lengths in one batch (this group is
    the batch of the grouping tests); a constant read and one clean step"""
    rng = np.random.default_rng(271)
    w1 = 4
    p = ref.params(w1=w1, w2=12)
    step = lambda T: np.array([0] * w1 + [100] * (T - w1))
    many = lambda T: (lambda o, x: o["status"] == ref.OK and len(x) == T and 20 < o["n_events"] <= ref.max_events(T, w1))
    items = [(levels(rng, 300), lambda o, x: o["status"] == ref.OK and 1 < o["n_events"] < 64),
             (np.zeros(0), lambda o, x: o["status"] == ref.EMPTY and o["n_events"] == 0),
             (np.array([7]), lambda o, x: o["n_events"] == 1 and (o["sum"], o["min"], o["max"], o["src"]) == ([7], [7], [7], [0])),
             (step(2 * w1 - 1), lambda o, x: o["n_events"] == 1 and o["sum"] == [300]),          # no sample has both windows inside the read
             (step(2 * w1), lambda o, x: o["start"] == [0, w1] and o["src"] == [0, 1]),          # exactly one has
             (step(2 * w1 + 1), lambda o, x: o["start"] == [0, w1] and o["sum"] == [0, 500])]
    for T in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1):
        items.append((levels(rng, T), many(T)))
    items.append((np.full(5000, 123), lambda o, x: o["n_events"] == 1 and o["sum"] == [123 * 5000] and o["sumsq"] == [123 * 123 * 5000]))
    items.append((np.array([0] * 50 + [10] * 50), lambda o, x: o["start"] == [0, 50] and o["src"] == [0, 1]))   # detector 2 peaks at 50 too: shadowed
    return _group("lengths", p, items)


def halo_group():
    """a clean step exactly on a tile's first sample, on its last, and at w1, 2 w1, w2, 2 w2 and w2 + 2 w1 to either side of a tile edge --
    the halo's reach -- at both inner edges of a read of three tiles"""
    rng = np.random.default_rng(272)
    p = ref.params(w1=4, w2=12)
    items = []
    for o in (0, -1, 4, -4, 8, -8, 12, -12, 24, -24, 20, -20):
        at = [TILE + o, 2 * TILE + o]
        items.append((steps_at(3 * TILE, at, rng), lambda out, x, at=at: all(a in out["start"] and out["src"][out["start"].index(a)] == 1 for a in at)))
    return _group("halo", p, items)


def tie_groups():
    """a pulse of w1 samples: its two edges have equal t and lie w1 apart, the smaller index wins; of w1 + 1 samples: both stay"""
    w1, a = 5, 40
    out = []
    for name, n, want in (("tie-w1", w1, [0, a]), ("tie-w1+1", w1 + 1, [0, a, a + w1 + 1])):
        x = np.array([0] * a + [10] * n + [0] * 40)
        out.append(_group(name, ref.params(w1=w1, w2=0, th1=160), [(x, lambda o, x, want=want: o["start"] == want)]))
    return out


def shadow_group():
    """w1 = 2, w2 = 3 on small random reads (found by a search over seeds): a peak of detector 2 whose nearest peak of detector 1 is at
    w2 - 1 (dropped) and at w2 (kept)"""
    p = ref.params(w1=2, w2=3, th1=64, th2=24)
    items = []
    for seed, i, dist, kept in ((12, 17, 2, False), (1, 28, 3, True)):
        x = np.random.default_rng(seed).integers(0, 6, 40).astype(np.int16)

        def cond(o, x, i=i, dist=dist, kept=kept):
            fl = ref.flags(x, p)[0]
            near = min(abs(i - j) for j, f in enumerate(fl) if f & 1)
            return fl[i] == 2 and near == dist and ((i in o["start"]) == kept) and (not kept or o["src"][o["start"].index(i)] == 2)
        items.append((x, cond))
    return _group("shadow", p, items)


def extreme_groups():
    """samples alternating +-32767 around one step from -32768 to 32767, windows of 32 and 64: the largest N and D the contract allows,
    products beyond 2^64; v0 = 1 and 2^16; th = 0 and 2^32 - 1; detector 2 off on a noisy read"""
    out = []
    alt = np.where(np.arange(200) % 2 == 0, -32767, 32767)
    x = np.concatenate([alt, np.full(64, -32768), np.full(64, 32767), alt])

    def big(o, x):
        (N1, D1), (N2, D2) = ref.flags(x, ref.params(w1=32, w2=64, v0=1 << 16))[1]
        return max(N2) == 64 * (64 * 65535) ** 2 and max(D2) > (1 << 43) and max(N2) * max(D2) > (1 << 92) and 264 in o["start"]
    out.append(_group("largest", ref.params(w1=32, w2=64, v0=1 << 16), [(x, big)]))
    rng = np.random.default_rng(273)
    x = levels(rng, 1500, span=40, noise=6)
    n = {v0: ref.segment(x, ref.params(v0=v0))["n_events"] for v0 in (1, 1 << 16)}
    for v0 in (1, 1 << 16):
        out.append(_group(f"v0-{v0}", ref.params(v0=v0), [(x, lambda o, x, v0=v0: o["n_events"] == n[v0] and n[1] > n[1 << 16] >= 1)]))
    out.append(_group("th-0", ref.params(th1=0, th2=0), [(x, lambda o, x: o["n_events"] > n[1] + 50)]))   # every local maximum of t cuts
    out.append(_group("th-max", ref.params(th1=(1 << 32) - 1, th2=(1 << 32) - 1), [(x, lambda o, x: o["n_events"] == 1)]))
    out.append(_group("w2-off", ref.params(w2=0), [(x, lambda o, x: o["n_events"] > 10 and 2 not in o["src"])]))
    # small steps under a strict short test and a lenient long one: most boundaries come from detector 2
    x = levels(np.random.default_rng(274), 3 * TILE, dwell=(25, 50), span=10, noise=5)
    out.append(_group("detector-2", ref.params(th1=576, th2=144), [(x, lambda o, x: o["src"].count(2) > 50 and o["src"].count(1) > 5)]))
    return out


def all_groups():
    return [length_group(), halo_group()] + tie_groups() + [shadow_group()] + extreme_groups()


def same(got, r, exp):
    assert int(got.status[r]) == exp["status"] and int(got.n_events[r]) == exp["n_events"], (r, int(got.status[r]), int(got.n_events[r]), exp["n_events"])
    for f in ref.EVENT_FIELDS:
        assert got.events[r][f].tolist() == exp[f], (r, f)


def raw_call(fn, raw, off, p, ev_off=None, sc=None, null_out=None, n_reads=None, budget=None, fill=0):
    """fn(raw, off, n_reads, params..., sc_lo, sc_hi, ev_off, [budget], ten outputs) on exact buffers; -> (return code, outputs)"""
    import ctypes
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    off_a = None if off is None else np.asarray(off, dtype=np.int64)
    n = (len(off) - 1 if off is not None else 1) if n_reads is None else n_reads
    if ev_off is None and off is not None:
        ev_off = np.concatenate([[0], np.cumsum([ref.max_events(max(int(b - a), 0), p["w1"]) if b - a <= ref.MAX_T else 0 for a, b in zip(off[:-1], off[1:])])])
    ev_a = None if ev_off is None else np.asarray(ev_off, dtype=np.int64)
    cap = int(ev_a[-1]) if ev_a is not None and len(ev_a) else 0
    outs = [np.full(max(n, 1), fill, np.int32) for _ in range(4)] + [np.full(max(cap, 1), fill, dt) for dt in (np.int32, np.int64, np.int64, np.int16, np.int16, np.uint8)]
    ptrs = [None if null_out == i else ptr(o) for i, o in enumerate(outs)]
    sc_a = [None, None] if sc is None else [None if s is None else np.asarray(s, dtype=np.int64) for s in sc]
    args = [p[k] for k in ref.PARAMS] + [ptr(sc_a[0]), ptr(sc_a[1]), ptr(ev_a)] + ([budget] if budget is not None else [])
    return fn(ptr(None if raw is None else np.ascontiguousarray(raw, np.int16)), ptr(off_a), n, *args, *ptrs), outs


def refusal_cases():
    """(good keyword arguments, [(name, keyword arguments)]) of raw_call: every argument refusal of rd_segment / _host"""
    good = dict(raw=np.arange(40, dtype=np.int16), off=[0, 40], p=ref.params())
    bad = [("null raw", dict(good, raw=None)), ("null offsets", dict(good, off=None, ev_off=[0, 9], n_reads=1)), ("null status", dict(good, null_out=0)),
           ("null ev_src", dict(good, null_out=9)), ("negative n_reads", dict(good, n_reads=-1)), ("negative offset", dict(good, off=[-1, 40])),
           ("offsets not monotone", dict(good, raw=np.arange(80, dtype=np.int16), off=[0, 50, 40])),
           ("too few event slots", dict(good, ev_off=[0, ref.max_events(40, 4) - 1])), ("event offsets not monotone", dict(good, ev_off=[9, 0])),
           ("sc_lo alone", dict(good, sc=([0], None))), ("scale window outside the read", dict(good, sc=([0], [41]))),
           ("scale window out of order", dict(good, sc=([5], [4]))), ("scale window without m2", dict(good, sc=([0], [40]), null_out=2))]
    for name, kw in (("w1 1", dict(w1=1)), ("w1 33", dict(w1=33, w2=40)), ("w2 == w1", dict(w2=4)), ("w2 65", dict(w2=65)), ("v0 0", dict(v0=0)),
                     ("v0 65537", dict(v0=65537))):
        bad.append((name, dict(good, p=dict(ref.params(), **kw))))
    return good, bad
