"""CPU restatement of the read-accuracy contract (radian/align.py) for the tests: Gotoh's affine-gap global alignment with the
library's fixed tie-break (include/radian_hip.h, rd_align_batch), the number of co-optimal alignments, and the command line's main
(radian/align.py:59-109) written out again on top of them.

The dynamic program runs over anti-diagonals, vectorised over the cells of a diagonal and over a batch of pairs (numpy), so a few
thousand pairs of a few hundred bases take seconds.  Co-optimal counts saturate at 2 (only "unique or not" is used)."""
import numpy as np

NEG = -(1 << 30)
SCORES = (2, -4, -4, -2)


def _gap(L, sc):
    return np.where(L == 0, 0, sc[2] + (L - 1) * sc[3])


def gotoh_batch(refs, reads, sc=SCORES):
    """refs / reads: lists of bytes.  Returns (scores int64 [P], n_optimal [P] in {1, 2 (= 2 or more)}, dirs uint8 [P, N+1, M+1]):
    dirs bits 0-1 the source of H (0 diagonal, 1 E = deletion, 2 F = insertion; ties in that order), bit 2 E opened (strictly better
    than extending), bit 3 F opened."""
    P = len(refs)
    N = max([len(r) for r in refs] + [0])
    M = max([len(q) for q in reads] + [0])
    A = np.full((P, max(N, 1)), -1, dtype=np.int16)
    B = np.full((P, max(M, 1)), -2, dtype=np.int16)
    for p in range(P):
        A[p, : len(refs[p])] = np.frombuffer(refs[p], dtype=np.uint8)
        B[p, : len(reads[p])] = np.frombuffer(reads[p], dtype=np.uint8)
    match, mis, o, e = sc
    dirs = np.zeros((P, N + 1, M + 1), dtype=np.uint8)
    shape = (P, N + 1)
    H2 = np.full(shape, NEG, dtype=np.int64)   # diagonal d - 2, indexed by i
    H1, E1, F1 = (np.full(shape, NEG, dtype=np.int64) for _ in range(3))
    c2 = np.zeros(shape, dtype=np.int64)
    cH1, cE1, cF1 = (np.zeros(shape, dtype=np.int64) for _ in range(3))
    score = np.zeros(P, dtype=np.int64)
    nopt = np.zeros(P, dtype=np.int64)
    n_of = np.array([len(r) for r in refs])
    m_of = np.array([len(q) for q in reads])
    for d in range(N + M + 1):
        H, E, F = (np.full(shape, NEG, dtype=np.int64) for _ in range(3))
        cH, cE, cF = (np.zeros(shape, dtype=np.int64) for _ in range(3))
        if d <= M:   # i = 0, j = d
            H[:, 0] = _gap(np.int64(d), sc)
            cH[:, 0] = 1
            if d > 0:
                F[:, 0] = H[:, 0]
                cF[:, 0] = 1
        if 1 <= d <= N:   # j = 0, i = d
            H[:, d] = E[:, d] = _gap(np.int64(d), sc)
            cH[:, d] = cE[:, d] = 1
        lo, hi = max(1, d - M), min(N, d - 1)
        if lo <= hi:
            i = np.arange(lo, hi + 1)
            j = d - i
            s = np.where(A[:, i - 1] == B[:, j - 1], match, mis)
            hd = H2[:, lo - 1: hi] + s
            eo, ee = H1[:, lo - 1: hi] + o, E1[:, lo - 1: hi] + e
            fo, fe = H1[:, lo: hi + 1] + o, F1[:, lo: hi + 1] + e
            en, fn = np.maximum(eo, ee), np.maximum(fo, fe)
            ce = np.minimum((eo == en) * cH1[:, lo - 1: hi] + (ee == en) * cE1[:, lo - 1: hi], 2)
            cf = np.minimum((fo == fn) * cH1[:, lo: hi + 1] + (fe == fn) * cF1[:, lo: hi + 1], 2)
            hn = np.maximum(hd, np.maximum(en, fn))
            ch = np.minimum((hd == hn) * c2[:, lo - 1: hi] + (en == hn) * ce + (fn == hn) * cf, 2)
            src = np.where(hd == hn, 0, np.where(en == hn, 1, 2))
            dirs[:, i, j] = (src | (eo > ee) << 2 | (fo > fe) << 3).astype(np.uint8)
            H[:, lo: hi + 1], E[:, lo: hi + 1], F[:, lo: hi + 1] = hn, en, fn
            cH[:, lo: hi + 1], cE[:, lo: hi + 1], cF[:, lo: hi + 1] = ch, ce, cf
        done = (n_of + m_of) == d
        if done.any():
            idx = np.nonzero(done)[0]
            score[idx] = H[idx, n_of[idx]]
            nopt[idx] = cH[idx, n_of[idx]]
        H2, c2 = H1, cH1
        H1, E1, F1, cH1, cE1, cF1 = H, E, F, cH, cE, cF
    return score, nopt, dirs


def traceback(dirs, ref, read):
    """column ops (bytes of M / X / D / I) of the tie-broken alignment, walking one pair's direction bits from (n, m)"""
    i, j, st = len(ref), len(read), 0
    out = []
    while i > 0 or j > 0:
        if i == 0:
            out.append("I")
            j -= 1
            continue
        if j == 0:
            out.append("D")
            i -= 1
            continue
        dv = int(dirs[i, j])
        if st == 0:
            st = dv & 3
            if st == 0:
                out.append("M" if ref[i - 1] == read[j - 1] else "X")
                i -= 1
                j -= 1
        elif st == 1:
            out.append("D")
            st = 0 if dv & 4 else 1
            i -= 1
        else:
            out.append("I")
            st = 0 if dv & 8 else 2
            j -= 1
    return "".join(reversed(out)).encode()


def rescore(ops, ref, read, sc=SCORES):
    """score of an alignment given as column ops; also checks that the ops consume both sequences exactly"""
    match, mis, o, e = sc
    i = j = tot = 0
    prev = None
    for c in ops.decode():
        if c in "MX":
            assert (ref[i] == read[j]) == (c == "M"), "M / X disagrees with the bytes"
            tot += match if c == "M" else mis
            i += 1
            j += 1
        elif c == "D":
            tot += e if prev == "D" else o
            i += 1
        elif c == "I":
            tot += e if prev == "I" else o
            j += 1
        else:
            raise AssertionError(f"op {c!r}")
        prev = c
    assert i == len(ref) and j == len(read), f"ops consume {i} x {j} of {len(ref)} x {len(read)}"
    return tot


# ---- score sets other than the default (match, mismatch, gap open, gap extend) ----
# accepted: gap_open <= gap_extend.  Linear gaps (open == extend: every "opened" comparison is a tie), a zero match score, a mismatch
# score of zero and a positive one, free extension, an expensive opening.
SMALL_SETS = (SCORES, (1, -1, -1, -1), (2, -3, -2, -2), (2, -4, 0, 0), (0, -1, -1, -1), (1, 0, -1, -1), (3, 1, -5, -2), (2, -4, -4, 0),
              (5, -4, -10, -1))
BOUND_SETS = ((65535, -65535, -65535, -65535), (1, -65535, -3, -1))   # the largest |score| the entry points take
ACCEPTED_SETS = SMALL_SETS + BOUND_SETS
REFUSED_SET = (1, -2, -1, -3)   # open > extend: the recurrence reopens adjacent gaps (tests/test_align_cpu.py keeps the counter-example)


def can_substitute(sc):
    """whether an optimal alignment can hold an X column at all: a D column followed by an I column (two openings) replaces it"""
    return sc[1] >= 2 * sc[2]


def three_state(ref, read, sc=SCORES):
    """The optimal global score under "a gap of length L costs open + (L - 1) * extend", by a model that is not Gotoh's recurrence:
    three matrices of alignments that END in a pair column (M), a deletion (X) or an insertion (Y), and a gap is ENTERED only from one
    of the other two states -- so two gaps of one kind are never adjacent, whatever the scores.  Plain Python ints, byte equality."""
    match, mis, go, ge = sc
    n, m = len(ref), len(read)
    none = -(1 << 62)
    M = [[none] * (m + 1) for _ in range(n + 1)]
    X = [[none] * (m + 1) for _ in range(n + 1)]
    Y = [[none] * (m + 1) for _ in range(n + 1)]
    M[0][0] = 0
    for i in range(1, n + 1):
        X[i][0] = go + (i - 1) * ge
    for j in range(1, m + 1):
        Y[0][j] = go + (j - 1) * ge
    for i in range(1, n + 1):
        a = ref[i - 1]
        Mi, Xi, Yi, Mu, Xu, Yu = M[i], X[i], Y[i], M[i - 1], X[i - 1], Y[i - 1]
        for j in range(1, m + 1):
            Mi[j] = max(Mu[j - 1], Xu[j - 1], Yu[j - 1]) + (match if a == read[j - 1] else mis)
            Xi[j] = max(max(Mu[j], Yu[j]) + go, Xu[j] + ge)
            Yi[j] = max(max(Mi[j - 1], Xi[j - 1]) + go, Yi[j - 1] + ge)
    return max(M[n][m], X[n][m], Y[n][m])


def _mutate(rng, s, letters, p=0.12):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < p / 3:
            continue
        out.append(c if r > p else int(rng.choice(list(letters))))
        if rng.random() < p / 3:
            out.append(int(rng.choice(list(letters))))
    return bytes(out)


def tie_pairs(rng):
    """pairs with very many co-optimal alignments, a pair with N (a byte like any other here), and the three empty cases"""
    def rnd(n, letters=b"AC"):
        return bytes(rng.choice(list(letters), n).astype(np.uint8))

    x = rnd(90)
    return [(b"A" * 70, b"A" * 40), (b"A" * 40, b"A" * 66), (b"AC" * 35, b"CA" * 33), (b"AAC" * 30, b"AC" * 40), (rnd(100), rnd(80)),
            (x, _mutate(rng, x, b"AC", 0.2)), (b"ACGTN" * 20, b"ACGT" * 26), (b"ACNNGT" * 11, b"ACNGT" * 13), (b"", rnd(10)), (rnd(10), b""),
            (b"", b"")]


def edge_pairs(rng, lengths_n=(1, 2, 3, 63, 64, 65, 127, 128, 129), lengths_m=(1, 2, 3, 63, 64, 65, 127, 128, 129)):
    """lengths around the forward kernel's 64-row tile and 64-column chunk on both sides: a mutated copy (its length moves a little) and
    an unrelated read of the exact length for every (n, m)"""
    def rnd(n):
        return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))

    pairs = []
    for n in lengths_n:
        for m in lengths_m:
            a = rnd(n)
            pairs.append((a, _mutate(rng, a, b"ACGT") if n > 8 and abs(n - m) <= 2 else rnd(m)))
            pairs.append((rnd(n), rnd(m)))
    return pairs


def score_set_pairs():
    """the pairs the GPU tests align under every score set of SMALL_SETS (seeded: the same everywhere)"""
    rng = np.random.default_rng(41)
    return edge_pairs(rng) + tie_pairs(rng)


def small_pairs():
    """20 pairs of 1..140 bases for the pure-Python model: edges at 63 / 64 / 65, homopolymer and dinucleotide pairs"""
    rng = np.random.default_rng(42)

    def rnd(n, letters=b"ACGT"):
        return bytes(rng.choice(list(letters), n).astype(np.uint8))

    pairs = [(b"A", b"C"), (b"A", b"AAAA"), (rnd(5), rnd(2)), (b"A" * 64, b"A" * 40), (b"A" * 30, b"A" * 65), (b"AC" * 32, b"CA" * 30),
             (b"AAC" * 21, b"AC" * 32), (rnd(63, b"AC"), rnd(65, b"AC")), (b"ACGTN" * 13, b"ACGT" * 16)]
    for n, m in ((63, 64), (64, 63), (65, 65), (64, 20), (20, 64), (140, 100), (100, 140)):
        pairs.append((rnd(n), rnd(m)))
    for n in (63, 64, 65, 140):
        a = rnd(n)
        pairs.append((a, _mutate(rng, a, b"ACGT", 0.15)))
    assert len(pairs) == 20 and all(1 <= len(a) <= 140 and 1 <= len(b) <= 140 for a, b in pairs)
    return pairs


def longest_run(ops, c):
    """length of the longest run of byte c in any of the op strings"""
    best = 0
    for o in ops:
        run = 0
        for x in o:
            run = run + 1 if x == c else 0
            best = max(best, run)
    return best


def align_cpu(refs, reads, sc=SCORES, cells_per_batch=48 << 20):
    """score, n_optimal and tie-broken ops of every pair (batches of similar sizes, largest first)"""
    refs = [r.encode() if isinstance(r, str) else bytes(r) for r in refs]
    reads = [q.encode() if isinstance(q, str) else bytes(q) for q in reads]
    P = len(refs)
    score = np.zeros(P, dtype=np.int64)
    nopt = np.zeros(P, dtype=np.int64)
    ops = [None] * P
    order = sorted(range(P), key=lambda p: -(len(refs[p]) + 1) * (len(reads[p]) + 1))
    k = 0
    while k < P:
        batch = [order[k]]
        n0, m0 = len(refs[order[k]]) + 1, len(reads[order[k]]) + 1
        k += 1
        while k < P and (len(batch) + 1) * n0 * m0 <= cells_per_batch:
            batch.append(order[k])
            k += 1
        s, c, dirs = gotoh_batch([refs[p] for p in batch], [reads[p] for p in batch], sc)
        for t, p in enumerate(batch):
            score[p], nopt[p] = s[t], c[t]
            ops[p] = traceback(dirs[t], refs[p], reads[p])
    return score, nopt, ops


def reference_main(fasta, tsv, clip_count, out_file):
    """radian/align.py's main restated on the CPU aligner: returns the stdout text; writes the TSV.  clip_count(ops, ref, read)
    -> ((n_match, n_sub, n_ins, n_del), status)."""
    read_ref = {}
    with open(tsv) as f:
        for i, line in enumerate(f):
            if i == 0:
                continue
            read, txt, seq = line.strip("\n").split("\t")
            read_ref[read] = seq
    recs, title, lines = [], None, []
    with open(fasta) as f:
        for line in f:
            if line.startswith(">"):
                if title is not None:
                    recs.append((title.split()[0], "".join(lines)))
                title, lines = line[1:].rstrip(), []
            else:
                lines.append(line.rstrip())
    if title is not None:
        recs.append((title.split()[0], "".join(lines)))
    refs = [read_ref[r] for r, _ in recs]
    seqs = [s.replace("U", "T") for _, s in recs]
    _, _, ops = align_cpu(refs, seqs)
    stats = []
    with open(out_file, "w") as out:
        out.write("read_id\tn_match\tn_ins\tn_del\tn_sub\n")
        for k, (rid, _) in enumerate(recs):
            (n_match, n_sub, n_ins, n_del), st = clip_count(ops[k], refs[k], seqs[k])
            assert st == 0
            acc = n_match / (n_match + n_sub + n_ins + n_del) * 100
            p_ins = n_ins / (n_match + n_sub + n_ins + n_del) * 100
            p_del = n_del / (n_match + n_sub + n_ins + n_del) * 100
            p_sub = n_sub / (n_match + n_sub + n_ins + n_del) * 100
            p_err = (n_ins + n_del + n_sub) / (n_match + n_sub + n_ins + n_del) * 100
            stats.append([acc, p_ins, p_del, p_sub, p_err])
            out.write(f"{rid}\t{n_match}\t{n_ins}\t{n_del}\t{n_sub}\n")
    stats = np.asarray(stats)
    txt = ""
    for name, c, tail in (("Accuracy", 0, ""), ("Insertions", 1, ""), ("Deletions", 2, ""), ("Substitutions", 3, "\n"), ("Total error", 4, "\n")):
        txt += f"{name}\tMEDIAN: {np.median(stats[:, c]):.2f}\tMEAN: {np.mean(stats[:, c]):.2f}\n{tail}"
    return txt
