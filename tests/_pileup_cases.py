"""Seeded cases of the pileup tests (tests/test_pileup_cpu.py asserts that each is what its name says; tests/test_gpu_pileup.py runs them on
the GPU).  A case is a dict: ops (list of bytes, None where the pairs are to be aligned), spans, reads (lists of bytes), site0, n_sites."""
import numpy as np

BASES = b"ACGT"
GRID = (0, 1, 2, 5, 63, 64, 65, 127, 128, 129, 200)


def rand_seq(rng, n):
    return bytes(BASES[i] for i in rng.integers(0, 4, size=n))


def mutate(rng, seq, rate=0.08):
    """substitutions at rate / 2, deletions and insertions at rate / 4 each"""
    out = bytearray()
    for b in seq:
        u = rng.random()
        if u < rate / 2:
            out.append(BASES[(BASES.index(b) + int(rng.integers(1, 4))) % 4])
        elif u < rate * 3 / 4:
            continue
        elif u < rate:
            out.append(b)
            out.append(BASES[int(rng.integers(0, 4))])
        else:
            out.append(b)
    return bytes(out)


def length_grid(seed=11):
    """every (n, m) of GRID x GRID, to be aligned: the read is a mutated copy of the span cut or filled up to m; equal lengths 64, 65 and
    200 are exact copies (alignments of exactly 64, 65 and 200 columns); disjoint spans"""
    rng = np.random.default_rng(seed)
    spans, reads, site0, at = [], [], [], 0
    for n in GRID:
        for m in GRID:
            s = rand_seq(rng, n)
            r = s if n == m and n in (64, 65, 200) else (mutate(rng, s) + rand_seq(rng, m))[:m]
            spans.append(s)
            reads.append(r)
            site0.append(at)
            at += n
    return dict(name="length_grid", ops=None, spans=spans, reads=reads, site0=site0, n_sites=at + 3)


def from_ops(rng, ops, equal_x=False, span=None):
    """a span and a read that the column string consumes exactly: the read byte of an M column equals the span byte, that of an X column
    differs (equal_x: it is equal all the same)"""
    ops = bytes(ops)
    n = sum(o != ord("I") for o in ops)
    span = rand_seq(rng, n) if span is None else span
    read, i = bytearray(), 0
    for o in ops:
        if o == ord("I"):
            read.append(BASES[int(rng.integers(0, 4))])
        elif o == ord("D"):
            i += 1
        else:
            b = span[i]
            if o == ord("X") and not equal_x:
                b = BASES[(BASES.index(b) + 1) % 4] if b in BASES else ord("A")
            read.append(b)
            i += 1
    return span, bytes(read)


def column_strings():
    """name -> ops: column strings no aligner would produce among them"""
    M, I, D = b"M", b"I", b"D"
    ctx = bytearray(M * 12)
    for i in (0, 1, 2, 9, 11):
        ctx[i] = ord("X")
    return {
        "ins_62_66": M * 62 + I * 5 + M * 10,
        "del_62_66": M * 62 + D * 5 + M * 10,
        "ins_run_70": M * 3 + I * 70 + M * 3,
        "del_run_70": M * 3 + D * 70 + M * 3,
        "ins_run_64": M * 3 + I * 64 + M * 3,
        "del_run_64": M * 3 + D * 64 + M * 3,
        "ins_run_63": M * 1 + I * 63 + M * 3,
        "ins_from_col_64": M * 64 + I * 3 + M * 2,
        "del_run_140": M * 60 + D * 140 + M * 5,
        "ins_run_whole_chunk": M * 64 + I * 64 + M * 64,
        "lead_i": I * 3 + M * 4,
        "lead_d": D * 2 + M * 3,
        "trail_i": M * 3 + I * 2,
        "trail_d": M * 3 + D * 2,
        "lead_trail_mixed": I + D + I + D + M * 3 + D + I + M + D + I + D + I,
        "lead_70_mixed": (I + D) * 35 + M * 5 + (D + I) * 35,
        "del_then_ins": M * 2 + D * 3 + I * 2 + M * 2,
        "ins_then_del": M * 2 + I * 2 + D * 3 + M * 2,
        "all_i": I * 4,
        "all_d": D * 3,
        "all_i_d": I * 2 + D * 2,
        "all_i_70": I * 70,
        "empty": b"",
        "single_m": M,
        "single_x": b"X",
        "x_equal_bytes": b"MXXMXM",
        "non_acgt": M * 3 + D + M * 2 + I * 2 + M * 6 + b"X" + M * 3,
        "contexts": bytes(ctx),
        "contexts_del_ins": M + D + M + I + M * 6 + I + M + D + M,
    }


def ops_cases(seed=12):
    """the column strings through rd_pileup_add_ops, on overlapping spans of one table"""
    rng = np.random.default_rng(seed)
    names, ops, spans, reads, site0 = [], [], [], [], []
    for k, (name, o) in enumerate(column_strings().items()):
        span = None
        n = sum(c != ord("I") for c in o)
        if name == "non_acgt":
            span = bytearray(rand_seq(rng, n))
            span[1], span[3], span[8] = ord("N"), ord("n"), ord("U")   # under an M column, under the D column, inside 5-mers
            span = bytes(span)
        s, r = from_ops(rng, o, equal_x=name == "x_equal_bytes", span=span)
        if name == "non_acgt":
            r = bytearray(r)
            r[0], r[6] = ord("N"), ord("a")   # an M column's read byte, an inserted byte
            r = bytes(r)
        names.append(name)
        ops.append(bytes(o))
        spans.append(s)
        reads.append(r)
        site0.append((k * 7) % 50)
    return dict(name="ops_cases", names=names, ops=ops, spans=spans, reads=reads, site0=site0, n_sites=50 + 210)


def hot(seed=13, n_pairs=300):
    """300 reads on one 40-base span: same-address atomics, several workgroups flush one profile"""
    rng = np.random.default_rng(seed)
    span = rand_seq(rng, 40)
    return dict(name="hot", ops=None, spans=[span] * n_pairs, reads=[mutate(rng, span) for _ in range(n_pairs)], site0=[5] * n_pairs, n_sites=50)


def disjoint(seed=14, n_pairs=300):
    rng = np.random.default_rng(seed)
    spans = [rand_seq(rng, 40) for _ in range(n_pairs)]
    return dict(name="disjoint", ops=None, spans=spans, reads=[mutate(rng, s) for s in spans], site0=[40 * p for p in range(n_pairs)], n_sites=40 * n_pairs)


def sparse(seed=15):
    """a table of 10^6 sites, 50 of them covered: five single-column pairs each on ten distant sites"""
    rng = np.random.default_rng(seed)
    site0 = sorted(int(s) for s in rng.choice(10 ** 6, size=50, replace=False))
    spans = [rand_seq(rng, 1) for _ in site0]
    return dict(name="sparse", ops=[b"M"] * 50, spans=spans, reads=list(spans), site0=site0, n_sites=10 ** 6)


# ---------------------------------------------------------------------------------------------- the command line's data set
CLI_SEED = 21
PLANTED = (1, 150)   # transcript index, position


def cli_case(seed=CLI_SEED, n_reads=120):
    """three transcripts; about 120 reads derived from them with substitutions and indels at about 8 %; 80 % of the reads of transcript 1
    carry one planted substitution at PLANTED; the matching PAF.  Among the reads: lower case and U, flanks outside [qstart, qend), a read
    absent from the PAF, a read with two PAF lines, a line on the minus strand.  Returns (names, seqs, reads [(name, seq)], paf lines,
    planted base)."""
    rng = np.random.default_rng(seed)
    names = ["tx_a|gene_a", "tx_b|gene_b", "tx_c|gene_c"]
    seqs = [rand_seq(rng, L).decode() for L in (260, 320, 200)]
    pt, pp = PLANTED
    ref_b = seqs[pt][pp]
    alt = "ACGT"[("ACGT".index(ref_b) + 2) % 4]
    reads, paf = [], []
    for r in range(n_reads):
        t = r % 3
        L = len(seqs[t])
        if t == pt:
            ts, te = int(rng.integers(0, 100)), int(rng.integers(200, L + 1))
        else:
            ts = int(rng.integers(0, L - 80))
            te = int(rng.integers(ts + 60, L + 1))
        part = bytearray(seqs[t][ts:te].encode())
        if t == pt and (r // 3) % 5 != 0:
            part[pp - ts] = ord(alt)
        body = mutate(rng, bytes(part)).decode()
        head = rand_seq(rng, int(rng.integers(0, 6))).decode() if r % 4 == 0 else ""
        tail = rand_seq(rng, int(rng.integers(0, 6))).decode() if r % 5 == 0 else ""
        seq = head + body + tail
        if r % 7 == 0:
            seq = seq.replace("T", "U")
        if r % 11 == 0:
            seq = seq.lower()
        name = f"read_{r:03d}"
        reads.append((name, seq))
        line = "\t".join(str(c) for c in (name, len(seq), len(head), len(head) + len(body), "+", names[t], L, ts, te, te - ts, te - ts, 255))
        if r == 17:
            continue                      # absent from the PAF
        if r == 23:
            paf.append("\t".join(str(c) for c in (name, len(seq), 0, len(seq), "-", names[t], L, ts, te, te - ts, te - ts, 255)))
            continue                      # its only line is on the minus strand
        paf.append(line)
        if r == 31:
            paf.append("\t".join(str(c) for c in (name, len(seq), 0, 10, "+", names[0], len(seqs[0]), 0, 10, 10, 10, 255)))   # a second line
    return names, seqs, reads, paf, alt
