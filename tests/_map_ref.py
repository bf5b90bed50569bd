"""The mapping contract of include/radian_hip.h (rd_map_index, rd_map_batch, rd_map_minimizers) and the span rule of radian_amd.map,
restated in plain Python from the contract's text: seeds, index order, anchors, chains, best and second best, and the span with
_fit_ref.fit_rows for the two pieces.  Also the seeded simulated set the CPU and GPU tests share."""
import numpy as np

import _fit_ref

C1, C2 = 0x9E3779B1, 0x85EBCA6B   # RD_MAP_HASH_C1 / _C2
LOOKBACK = 64                     # RD_MAP_LOOKBACK
OK, NO_SEED, NO_CHAIN, TOO_LARGE, EMPTY_SPAN = 0, 1, 2, 3, 4
DEFAULTS = dict(k=14, w=8, max_occ=500, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, piece=512)


def kmer_hash(x, k):
    mask = (1 << (2 * k)) - 1
    for c in (C1, C2):
        x = (x * c) & mask
        x ^= x >> k
    return x


def kmers(codes, k):
    """[(position, hash)] of every k-mer that exists, per segment: [[...], [...]]"""
    codes = [int(c) for c in codes]
    segs, cur = [], []
    for p in range(len(codes) - k + 1):
        word = codes[p: p + k]
        if all(c <= 3 for c in word):
            x = 0
            for c in word:
                x = (x << 2) | c
            cur.append((p, kmer_hash(x, k)))
        elif cur:
            segs.append(cur)
            cur = []
    if cur:
        segs.append(cur)
    return segs


def minimizers(codes, k, w):
    """[(position, hash)] ascending: the distinct choices of every window of w consecutive k-mers of a segment, the single minimum of a
    segment with fewer than w"""
    chosen = {}
    for seg in kmers(codes, k):
        if len(seg) < w:
            windows = [seg]
        else:
            windows = [seg[s: s + w] for s in range(len(seg) - w + 1)]
        for win in windows:
            p, h = min(win, key=lambda ph: (ph[1], ph[0]))
            chosen[p] = h
    return sorted(chosen.items())


def build_index(transcripts, k, w):
    """{hash: [(t, r)] ascending}"""
    index = {}
    for t, codes in enumerate(transcripts):
        for r, h in minimizers(codes, k, w):
            index.setdefault(h, []).append((t, r))
    return index


def index_stats(index, max_occ):
    return {"entries": sum(len(v) for v in index.values()), "keys": len(index), "keys_dropped": sum(1 for v in index.values() if len(v) > max_occ)}


def anchors(read, index, k, w, max_occ):
    out = []
    for q, h in minimizers(read, k, w):
        entries = index.get(h, [])
        if len(entries) > max_occ:
            continue
        out.extend((t, r, q) for t, r in entries)
    return sorted(out)


def gap_cost(d, k):
    return 0 if d == 0 else ((d * k) >> 6) + ((d.bit_length() - 1) >> 1)


def chain(seg, k, max_gap, bandwidth):
    """seg: [(r, q)] in order -> (score, first index, anchors, end index)"""
    f, first, cnt = [], [], []
    for i, (ri, qi) in enumerate(seg):
        best, arg = k, None
        for j in range(i - 1, max(-1, i - 1 - LOOKBACK), -1):   # nearest first; only a greater candidate replaces
            dr, dq = ri - seg[j][0], qi - seg[j][1]
            if not (0 < dq <= max_gap and 0 < dr <= max_gap and abs(dr - dq) <= bandwidth):
                continue
            c = f[j] + min(dq, dr, k) - gap_cost(abs(dr - dq), k)
            if c > best:
                best, arg = c, j
        f.append(best)
        first.append(i if arg is None else first[arg])
        cnt.append(1 if arg is None else cnt[arg] + 1)
    end = f.index(max(f))
    return f[end], first[end], cnt[end], end


def map_read(read, index, k=14, w=8, max_occ=500, min_anchors=3, min_score=40, max_gap=1000, bandwidth=500, **_):
    """{status, t, score, score2, n_anchors, q0, r0, q1, r1, chains: {t: (score, anchors)} of the qualifying chains}"""
    zero = dict(t=0, score=0, score2=0, n_anchors=0, q0=0, r0=0, q1=0, r1=0, chains={})
    anc = anchors(read, index, k, w, max_occ)
    if not anc:
        return dict(zero, status=NO_SEED)
    by_t = {}
    for t, r, q in anc:
        by_t.setdefault(t, []).append((r, q))
    best, chains = None, {}
    for t in sorted(by_t):
        seg = by_t[t]
        score, first, n, end = chain(seg, k, max_gap, bandwidth)
        if n < min_anchors or score < min_score:
            continue
        chains[t] = (score, n)
        if best is None or score > best[1]:
            best = (t, score, n, seg[first], seg[end])
    if best is None:
        return dict(zero, status=NO_CHAIN)
    t, score, n, (r0, q0), (r1, q1) = best
    score2 = max([s for u, (s, _) in chains.items() if u != t], default=0)
    return dict(status=OK, t=t, score=score, score2=score2, n_anchors=n, q0=q0, r0=r0, q1=q1, r1=r1, chains=chains)


FIELDS = ("t", "score", "score2", "n_anchors", "q0", "r0", "q1", "r1")


def map_reads(reads, transcripts, **params):
    p = dict(DEFAULTS, **params)
    index = build_index(transcripts, p["k"], p["w"])
    return [map_read(r, index, **p) for r in reads], index


def ref_codes(codes):
    """transcript codes as the fit takes them: 0..3, anything else 4"""
    c = np.asarray(codes, dtype=np.uint8).copy()
    c[c > 3] = 4
    return c


def span(read, transcript, hit, k=14, piece=512, fit_fn=None):
    """(S, E) of a mapped read: its head and tail pieces fitted into the transcript around the chain's first and last anchors"""
    fit_fn = fit_fn or _fit_ref.fit_rows
    read = np.asarray(read, dtype=np.uint8)
    tr = ref_codes(transcript)
    L, n = len(read), len(tr)
    q0, r0, q1, r1 = hit["q0"], hit["r0"], hit["q1"], hit["r1"]
    c = max(0, q0 + k - piece)
    head = read[c: q0 + k]
    w0 = max(0, r0 + k - 2 * len(head))
    fh = fit_fn(tr[w0: r0 + k], head)
    S = max(0, w0 + fh["ref_start"] - c)
    tail = read[q1: min(L, q1 + piece)]
    ft = fit_fn(tr[r1: min(n, r1 + 2 * len(tail))], tail)
    E = min(n, r1 + ft["ref_end"] + (L - q1 - len(tail)))
    return S, E


# ---- the simulated set ----------------------------------------------------------------------------------------------------------
def mutate(rng, seq, rate):
    """substitutions, deletions and insertions at `rate` in all, a third each (the _mutate of tests/test_gpu_label_build.py)"""
    out = []
    for c in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(int(rng.integers(0, 4)) if r < 2 * rate / 3 else int(c))
        if rng.random() < rate / 3:
            out.append(int(rng.integers(0, 4)))
    return np.array(out if out else [int(rng.integers(0, 4))], dtype=np.uint8)


def simulate(seed=2026, n_reads=300, rate=0.12, n_unrelated=30, n_genes=10):
    """(transcripts, reads, truth): n_unrelated random transcripts of 400..4000 bases, then n_genes genes of 8 exons with three
    isoforms each, every isoform skipping one exon of its own; reads of at least 400 bases from random positions, mutated at `rate`.
    truth[i] = (transcript, start, end) of read i before the mutation."""
    rng = np.random.default_rng(seed)
    transcripts = [rng.integers(0, 4, size=int(rng.integers(400, 4001)), dtype=np.uint8) for _ in range(n_unrelated)]
    for _ in range(n_genes):
        exons = [rng.integers(0, 4, size=int(rng.integers(100, 501)), dtype=np.uint8) for _ in range(8)]
        for skip in rng.choice(np.arange(1, 7), size=3, replace=False):
            transcripts.append(np.concatenate([e for j, e in enumerate(exons) if j != int(skip)]))
    reads, truth = [], []
    for _ in range(n_reads):
        t = int(rng.integers(0, len(transcripts)))
        n = len(transcripts[t])
        length = int(rng.integers(400, min(n, 1500) + 1))
        start = int(rng.integers(0, n - length + 1))
        reads.append(mutate(rng, transcripts[t][start: start + length], rate))
        truth.append((t, start, start + length))
    return transcripts, reads, truth
