"""Seeded inputs for the stage-by-stage checks of map.hip (tests/test_gpu_map_kernels.py) and the conditions they have to meet
(tests/test_map_cpu.py asserts them from the restatement alone, so that an edit here cannot quietly empty a case).

Chain calls: dicts {name, k, min_anchors, max_gap, bandwidth, segs}, segs a list of segments, a segment a list of (r, q) in strictly
ascending order.  arrays(call) gives the (t, r, q) that rd_map_diag_chain takes, segment s as transcript s.  steps(seg, ...) is
_map_ref.chain's loop with a record of every step.  Minimizer images: (name, records) per (k, w), records laid back to back with one
break code after each, as the library lays them."""
import functools
import itertools

import numpy as np

import _map_ref as mr

SMALL = dict(max_gap=50, bandwidth=10)      # limits that bind on coordinates of a few tens
LENGTHS = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 200)
SEGMENT_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)   # four waves per workgroup: the last workgroup full and partly filled
PLANTED_D = (1, 2, 31, 32, 33, 62, 63, 64, 65, 66)
BREAK = 255


# ---- chain segments ----------------------------------------------------------------------------------------------------------------
def lattice(rng, n, span):
    """n distinct points with r and q in 0..span-1, sorted: many valid predecessors, many equal candidates"""
    pts = set()
    while len(pts) < n:
        pts.add((int(rng.integers(0, span)), int(rng.integers(0, span))))
    return sorted(pts)


def planted(d, blocks=64):
    """(segment, probes): `blocks` blocks of target, d - 1 decoys, probe (and one more decoy where that makes the block's length odd, so
    that the probes of 64 blocks fall on every i mod 64).  Under SMALL the probe's only valid predecessor is its target, d anchors
    back: the decoys between them share one r and have q >= the probe's (dq <= 0), everything before the target is more than max_gap
    back in r.  The next block's target has the probe as its only valid predecessor, so for d <= 64 the whole segment is one chain of
    2 * blocks anchors that breaks where a probe misses its target; for d > 64 the target is out of the look-back and the chains are
    probe -> next target, two anchors each."""
    seg, probes = [], []
    R = Q = 0
    for _ in range(blocks):
        seg.append((R, Q))                                        # target
        seg.extend((R + 1, Q + 30 + j) for j in range(d - 1))     # decoys: dq = -j to the probe, |dr - dq| > bandwidth from the target
        probes.append(len(seg))
        seg.append((R + 30, Q + 30))                              # probe
        if (d + 1) % 2 == 0:
            seg.append((R + 31, Q + 230))                         # a decoy that shifts the next block by one
        R, Q = R + 60, Q + 60                                     # the next target: 30 from the probe, 60 from this target
    return seg, probes


def lanes(d, k, rows, hot):
    """rows x d anchors, row by row: the only valid predecessor of the anchor in row p, lane c is the one in row p - 1, lane c, exactly d
    anchors back (one row shares an r; lanes are 1000 apart in q).  Lane `hot` advances on the diagonal, the others pay a gap cost of 1
    per step, so the segment's best chain is the hot lane's."""
    assert mr.gap_cost(4, k) == 1
    return [(10 * p, 1000 * c + (10 if c == hot else 14) * p) for p in range(rows) for c in range(d)]


def pair(rng, dr, dq):
    r, q = int(rng.integers(0, 1000)), int(rng.integers(0, 1000))
    return [(r, q), (r + dr, q + dq)]


@functools.lru_cache(maxsize=None)
def chain_calls():
    rng = np.random.default_rng(4242)
    calls = []

    def add(name, k, segs, min_anchors=1, **p):
        calls.append(dict(dict(SMALL, **p), name=name, k=k, min_anchors=min_anchors, segs=segs))

    # dense lattices: every length, every segment count
    lengths = itertools.cycle(LENGTHS)
    for c, n_seg in enumerate(SEGMENT_COUNTS):
        add(f"lattice x{n_seg}", (8, 15)[c % 2], [lattice(rng, next(lengths), 60) for _ in range(n_seg)], min_anchors=(1, 3)[c % 2])
    for k in (8, 15):
        add(f"lattice k{k} min 65", k, [lattice(rng, n, 40) for n in LENGTHS], min_anchors=65)
    add("lattice bandwidth 0", 15, [lattice(rng, n, 30) for n in LENGTHS], min_anchors=3, bandwidth=0)
    add("lattice bandwidth 0 k8", 8, [lattice(rng, n, 30) for n in LENGTHS if n >= 63], bandwidth=0)
    # the defaults: a wide lattice (gap costs above f + k: candidates below zero) and pairs whose only candidate is below zero
    for k in (8, 15):
        add(f"defaults k{k}", k, [lattice(rng, n, 700) for n in LENGTHS] + [pair(rng, 400 + int(rng.integers(0, 90)), 1 + int(rng.integers(0, 5))) for _ in range(30)],
            min_anchors=3, max_gap=mr.DEFAULTS["max_gap"], bandwidth=mr.DEFAULTS["bandwidth"])
    # planted far winners
    for c, d in enumerate(PLANTED_D):
        add(f"planted d{d}", (8, 15)[c % 2], [planted(d)[0]])
    # every winner distance
    for k in (8, 15):
        add(f"lanes k{k}", k, [lanes(d, k, 20 // d + 2, int(rng.integers(0, d))) for d in range(1, 65)], min_anchors=2)
    # pairs at the limits, one segment each: dq, dr at max_gap and one past it; |dr - dq| at the bandwidth and one past it; every |dr - dq|
    # up to 10; a candidate of exactly k (f = k, min(dq, dr, k) = 1, gap cost 1)
    kinds = [(50, 50), (45, 50), (50, 45), (45, 51), (51, 45), (41, 51), (51, 41), (20, 30), (30, 20), (20, 31), (31, 20), (1, 5), (5, 1)]
    kinds += [(12, 12 + dd) for dd in range(1, 11)] + [(12 + dd, 12) for dd in range(1, 11)]
    for k in (8, 15):
        assert mr.gap_cost(4, k) == 1
        add(f"pairs k{k}", k, [pair(rng, dr, dq) for dr, dq in kinds for _ in range(12)], min_anchors=(1, 2)[k == 15])
    add("pairs bandwidth 0", 15, [pair(rng, dr, dq) for dr, dq in ((10, 10), (10, 11), (11, 10), (1, 1), (50, 50), (51, 51)) for _ in range(12)], bandwidth=0)
    return calls


def arrays(call):
    """(t, r, q) uint32 of the call's anchors, segment s as transcript s"""
    t = np.concatenate([np.full(len(s), i, dtype=np.uint32) for i, s in enumerate(call["segs"])])
    rq = np.array([a for s in call["segs"] for a in s], dtype=np.uint32).reshape(-1, 2)
    return t, np.ascontiguousarray(rq[:, 0]), np.ascontiguousarray(rq[:, 1])


def expected(call):
    """int32 [segments, 5]: start, score, first, count, end of every segment by _map_ref.chain; score = count = 0 below min_anchors"""
    out, at = [], 0
    for seg in call["segs"]:
        row = mr.chain(seg, call["k"], call["max_gap"], call["bandwidth"]) if len(seg) >= call["min_anchors"] else (0, 0, 0, 0)
        out.append((at,) + tuple(row))
        at += len(seg)
    return np.array(out, dtype=np.int32).reshape(-1, 5)


def steps(seg, k, max_gap, bandwidth):
    """_map_ref.chain's loop, recording per step i: `win` (the winner's distance i - j, None when the anchor starts a chain), `best` (the
    largest candidate of the look-back, None without a valid one), `tied` (the j that give it, when it extends), `beyond` (a candidate
    more than LOOKBACK back that beats both k and `best`), `valid` (valid predecessors in the look-back) and `pairs` ((dr, dq, valid)
    of every anchor of the look-back).  Returns (steps, chain result)."""
    f, first, cnt, out = [], [], [], []

    def cand(i, j):
        dr, dq = seg[i][0] - seg[j][0], seg[i][1] - seg[j][1]
        ok = 0 < dq <= max_gap and 0 < dr <= max_gap and abs(dr - dq) <= bandwidth
        return dr, dq, (f[j] + min(dq, dr, k) - mr.gap_cost(abs(dr - dq), k)) if ok else None

    for i in range(len(seg)):
        best, arg, top, pairs = k, None, None, []
        cands = {}
        for j in range(i - 1, max(-1, i - 1 - mr.LOOKBACK), -1):
            dr, dq, c = cand(i, j)
            pairs.append((dr, dq, c is not None))
            if c is None:
                continue
            cands[j] = c
            top = c if top is None else max(top, c)
            if c > best:
                best, arg = c, j
        far = []
        for j in range(i - 1 - mr.LOOKBACK, -1, -1):   # ascending r: nothing before the first anchor beyond max_gap is valid
            dr, dq, c = cand(i, j)
            if dr > max_gap:
                break
            if c is not None:
                far.append(c)
        out.append(dict(i=i, win=None if arg is None else i - arg, best=top, valid=len(cands), pairs=pairs,
                        tied=[j for j, c in cands.items() if c == best] if arg is not None else [],
                        beyond=bool(far) and max(far) > best))
        f.append(best)
        first.append(i if arg is None else first[arg])
        cnt.append(1 if arg is None else cnt[arg] + 1)
    end = f.index(max(f))
    return out, (f[end], first[end], cnt[end], end)


# ---- minimizer images ----------------------------------------------------------------------------------------------------------------
SEEDS = ((8, 1), (8, 64), (15, 1), (15, 8), (15, 64))
TILE = 1024   # positions one workgroup of the minimizer kernel decides; the compaction's block is two of them
SIZES = lambda k: (1, k - 1, k, 1023, 1024, 1025, 2047, 2048, 2049, 3072)


def flat_image(records):
    """(flat uint8, starts): the records back to back with one break code after each; record r starts at offsets[r] + r"""
    parts, starts, at = [], [], 0
    for rec in records:
        starts.append(at)
        parts += [np.asarray(rec, dtype=np.uint8), np.array([BREAK], dtype=np.uint8)]
        at += len(rec) + 1
    return np.concatenate(parts), starts


@functools.lru_cache(maxsize=None)
def minimizer_images(k, w):
    """[(name, records)] for one seed shape; the conditions are asserted by tests/test_map_cpu.py"""
    rng = np.random.default_rng(1000 * k + w)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    images = [(f"N {n}", [rnd(n - 1)]) for n in SIZES(k)]
    for edge in (TILE, 2 * TILE):
        for p in (edge - 1, edge, edge + 1):   # a record, hence a segment, starts at p: the break before it lies at p - 1
            images.append((f"segment starts at {p}", [rnd(p - 1), rnd(300)]))
        for p in (edge - 1, edge):             # a break inside a record
            codes = rnd(edge + 700)
            codes[p] = BREAK
            images.append((f"break at {p}", [codes]))
        if w > 1:                              # a segment of w - 1 k-mers across the edge, and one of a single k-mer
            for n_kmers in sorted({w - 1, 1}):
                codes, n = rnd(edge + 700), k + n_kmers - 1
                a = edge - n // 2
                codes[a - 1] = codes[a + n] = BREAK
                images.append((f"{n_kmers} k-mers across {edge}", [codes]))
        codes, half = rnd(edge + 700), w + k
        codes[edge - half: edge + half] = int(rng.integers(0, 4))
        images.append((f"homopolymer across {edge}", [codes]))
        codes = rnd(edge + 700)
        codes[edge - half: edge + half] = np.tile(np.array([1, 2], dtype=np.uint8), half)
        images.append((f"dinucleotide repeat across {edge}", [codes]))
    images.append(("all breaks", [np.full(1499, BREAK, dtype=np.uint8)]))
    images.append(("many short records", [rnd(int(n)) for n in rng.integers(0, 2 * k + w, size=60)]))
    if w == 1:
        images.append(("every k-mer flagged", [rnd(4999)]))
    return images
