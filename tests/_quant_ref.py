"""The quantification contract of include/radian_hip.h (rd_map_candidates, rd_quant_em) restated in plain Python integers from the
contract's text: a read's candidate chains on top of _map_ref's anchors and chains, one EM step, the EM.  Also the generator of the
accuracy condition that the CPU and GPU tests share."""
import numpy as np

import _map_ref as mr
import _quant_cases as qc

ONE = 1 << 20
FIELDS = ("t", "score", "n_anchors", "q0", "r0", "q1", "r1", "d3")


def candidates(read, index, lengths, k=14, w=8, max_occ=500, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, max_cand=16,
               min_frac_q10=922, max_3p=-1, **_):
    """{status, n_qual, n_cand, rows: [(t, score, n_anchors, q0, r0, q1, r1, d3)] of the first n_cand candidates}"""
    anc = mr.anchors(read, index, k, w, max_occ)
    if not anc:
        return dict(status=mr.NO_SEED, n_qual=0, n_cand=0, rows=[])
    by_t = {}
    for t, r, q in anc:
        by_t.setdefault(t, []).append((r, q))
    L = len(read)
    passing = []
    for t in sorted(by_t):
        seg = by_t[t]
        score, first, n, end = mr.chain(seg, k, max_gap, bandwidth)
        if n < min_anchors or score < min_score:
            continue
        (r0, q0), (r1, q1) = seg[first], seg[end]
        d3 = (lengths[t] - r1) - (L - q1)
        if max_3p >= 0 and d3 > max_3p:
            continue
        passing.append((t, score, n, q0, r0, q1, r1, d3))
    if not passing:
        return dict(status=mr.NO_CHAIN, n_qual=0, n_cand=0, rows=[])
    best = max(p[1] for p in passing)
    cand = sorted((p for p in passing if p[1] * 1024 >= best * min_frac_q10), key=lambda p: (-p[1], p[0]))
    return dict(status=mr.OK, n_qual=len(cand), n_cand=min(len(cand), max_cand), rows=cand[:max_cand])


def step(reads, c):
    """reads: [[(t, w)]] -> (c', [[share]], the largest shift any read took)"""
    out = [0] * len(c)
    shares, top = [], 0
    for cands in reads:
        if not cands:
            shares.append([])
            continue
        a = [c[t] * w for t, w in cands]
        S = sum(a)
        sh = max(0, S.bit_length() - 44)
        a = [x >> sh for x in a]
        S2 = sum(a)
        assert S2 > 0
        row = [(x << 20) // S2 for x in a]
        for (t, _), s in zip(cands, row):
            out[t] += s
        shares.append(row)
        top = max(top, sh)
    return out, shares, top


def em(reads, n_tx, max_iter, tol_q20, trace=None):
    """-> (count, shares per read, iterations run, last delta).  trace: a list that receives (c, largest shift) of every step"""
    c, shares, sh = step(reads, [1] * n_tx)
    if trace is not None:
        trace.append((c, sh))
    iters, last = 0, 0
    for _ in range(max_iter):
        cn, shares, sh = step(reads, c)
        last = max((abs(x - y) for x, y in zip(cn, c)), default=0)
        c = cn
        iters += 1
        if trace is not None:
            trace.append((c, sh))
        if last <= tol_q20:
            break
    return c, shares, iters, last


def stats(reads, count, iters, last):
    """rd_quant_em's stats[0..5]"""
    with_c = sum(1 for r in reads if r)
    return [iters, last, with_c * ONE - sum(count), len(reads) - with_c, sum(1 for r in reads if len(r) == 1), sum(len(r) for r in reads)]


def csr(reads):
    """[[(t, w)]] -> (cand_off int64, cand_t int32, cand_w uint16)"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    flat = [p for r in reads for p in r]
    return off, np.array([t for t, _ in flat], dtype=np.int32), np.array([w for _, w in flat], dtype=np.uint16)


def weights(rows, mode):
    """the command's weights of a read's candidate rows: `equal` 1, `score` max(1, score * 4096 // best)"""
    if mode == "equal":
        return [1] * len(rows)
    best = rows[0][1]
    return [max(1, r[1] * 4096 // best) for r in rows]


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
def assert_em_equal(res, c, what):
    """counts, shares and stats[0..5] of a QuantResult against the restatement's"""
    assert [int(v) for v in res.count] == c["count"], f"{what}: {c['name']}: counts"
    if res.share is not None:
        assert [int(v) for v in res.share] == [s for row in c["shares"] for s in row], f"{what}: {c['name']}: shares"
    exp = stats(c["reads"], c["count"], c["iters"], c["last"])
    got = [res.stats[k] for k in ("iterations", "last_delta", "lost", "reads_empty", "reads_single", "slots")]
    assert got == exp, f"{what}: {c['name']}: stats {got}, the restatement gives {exp}"


def refusals():
    """(name, cand_off, cand_t, cand_w, n_tx, max_iter) of every refused call with array arguments"""
    out = [(name,) + tuple(csr(reads)) + (n_tx, 5) for name, reads, n_tx in qc.REFUSALS]
    off, t, w = csr([[(0, 1)], [(1, 1), (2, 1)], [(0, 5)]])
    bad = off.copy()
    bad[2] = 0
    out.append(("decreasing offsets", bad, t, w, 3, 5))
    bad = off.copy()
    bad[0] = 1
    out.append(("offsets that do not start at 0", bad, t, w, 3, 5))
    out.append(("max_iter above 100000", off, t, w, 3, 100001))
    out.append(("negative max_iter", off, t, w, 3, -1))
    out.append(("n_tx = 2^24", off, t, w, 1 << 24, 5))
    return out


def call_raw(fn, ctx, off, t, w, n_reads, n_tx, max_iter, count, share, stats):
    import ctypes
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    args = (p(off), p(t), p(w), n_reads, n_tx, max_iter, 0, p(count), p(share), p(stats))
    return fn(*((ctx,) + args if ctx is not None else args))


def check_refusals(fn, ctx=None):
    """every refusal returns RD_ERR_ARG (-1) and leaves count, share and stats as they were"""
    n = 0
    for name, off, t, w, n_tx, max_iter in refusals():
        count, share, stats = np.full(80, 0x4D4D, np.uint64), np.full(80, 0x4D4D, np.uint32), np.full(16, 0x4D4D, np.int64)
        t2, w2 = (t if t.size else np.zeros(1, np.int32)), (w if w.size else np.zeros(1, np.uint16))
        assert call_raw(fn, ctx, off, t2, w2, len(off) - 1, n_tx, max_iter, count, share, stats) == -1, name
        assert (count == 0x4D4D).all() and (share == 0x4D4D).all() and (stats == 0x4D4D).all(), name
        n += 1
    off, t, w = csr([[(0, 1)], [(1, 1), (2, 1)]])
    for name, a in (("null cand_off", (None, t, w)), ("null cand_t", (off, None, w)), ("null cand_w", (off, t, None))):
        count, share, stats = np.full(8, 0x4D4D, np.uint64), np.full(8, 0x4D4D, np.uint32), np.full(16, 0x4D4D, np.int64)
        assert call_raw(fn, ctx, *a, 2, 3, 5, count, share, stats) == -1, name
        assert (count == 0x4D4D).all() and (share == 0x4D4D).all() and (stats == 0x4D4D).all(), name
        n += 1
    share, stats = np.full(8, 0x4D4D, np.uint32), np.full(16, 0x4D4D, np.int64)
    assert call_raw(fn, ctx, off, t, w, 2, 3, 5, None, share, stats) == -1, "null count"
    assert (share == 0x4D4D).all() and (stats == 0x4D4D).all()
    return n + 1


# ---- the generator of the accuracy condition ------------------------------------------------------------------------------------
ACCURACY_SETTINGS = (("random", 1), ("random", 2), ("3p", 1), ("3p", 2))


def accuracy_set(mode, seed, n_reads=400, rate=0.12):
    """(transcripts, reads, truth, true counts): 6 unrelated transcripts of 400..2000 bases, then 8 genes of 8 exons (100..500 bases)
    with three isoforms each, every isoform skipping one inner exon; isoforms at 1 : 2 : 9 in index order, the unrelated ones at 1;
    reads of 400..1500 bases at `rate` error from random positions (`random`) or ending at the transcript's 3' end (`3p`)"""
    rng = np.random.default_rng(1000 * seed + (7 if mode == "3p" else 0))
    transcripts = [rng.integers(0, 4, size=int(rng.integers(400, 2001)), dtype=np.uint8) for _ in range(6)]
    prop = [1.0] * 6
    for _ in range(8):
        exons = [rng.integers(0, 4, size=int(rng.integers(100, 501)), dtype=np.uint8) for _ in range(8)]
        for skip, p in zip(rng.choice(np.arange(1, 7), size=3, replace=False), (1.0, 2.0, 9.0)):
            transcripts.append(np.concatenate([e for j, e in enumerate(exons) if j != int(skip)]))
            prop.append(p)
    prop = np.array(prop) / sum(prop)
    reads, truth = [], []
    true = [0] * len(transcripts)
    for _ in range(n_reads):
        t = int(rng.choice(len(transcripts), p=prop))
        n = len(transcripts[t])
        length = int(rng.integers(400, min(n, 1500) + 1))
        start = n - length if mode == "3p" else int(rng.integers(0, n - length + 1))
        reads.append(mr.mutate(rng, transcripts[t][start: start + length], rate))
        truth.append(t)
        true[t] += 1
    return transcripts, reads, truth, true


ACCURACY_PARAMS = dict(max_cand=16, min_frac_q10=922, max_3p=-1, max_iter=1000, tol_q20=1024)


def l1_errors(true, count, best_hits):
    """(L1 of the best-hit counts, L1 of the EM's counts in reads) against the true counts"""
    hit = [0] * len(true)
    for t in best_hits:
        hit[t] += 1
    return sum(abs(a - b) for a, b in zip(hit, true)), sum(abs(c - t * ONE) for c, t in zip(count, true)) / ONE
