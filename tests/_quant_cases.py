"""Seeded cases of the quantification tests (tests/test_quant_cpu.py, tests/test_gpu_quant.py).  An EM case is a dict: name, reads
([[(t, w)]]), n_tx, max_iter, tol_q20 and `cond`, the condition that defines it, as a function of (case, trace) -- trace being the
restatement's [(c, largest shift)] per step -- that returns True when the case really is what its name says.  The candidate cases are
transcripts, reads and the parameter sets to run them under, with the same kind of condition on the restatement's result."""
import numpy as np

import _map_ref as mr

ONE = 1 << 20


def _case(name, reads, n_tx, max_iter, tol_q20, cond):
    return dict(name=name, reads=reads, n_tx=n_tx, max_iter=max_iter, tol_q20=tol_q20, cond=cond)


def _read(rng, n, n_tx, wmax=4096):
    t = rng.choice(n_tx, size=n, replace=False)
    return [(int(x), int(rng.integers(1, wmax + 1))) for x in t]


def _random_reads(rng, n_reads, n_tx, sizes, wmax=4096):
    return [_read(rng, int(rng.choice(sizes)), n_tx, wmax) for _ in range(n_reads)]


def pack_events(reads):
    """what the packer meets on the multi-candidate reads, in order: (rows that end in padding, rows a read fills to the last slot,
    reads that would have straddled a row)"""
    pos = padded = exact = straddle = 0
    for r in reads:
        n = len(r)
        if n < 2:
            continue
        if pos % 64 + n > 64:
            straddle += 1
            padded += 1
            pos = (pos + 63) // 64 * 64
        pos += n
        if pos % 64 == 0:
            exact += 1
    if pos % 64:
        padded += 1
    return padded, exact, straddle


def em_cases():
    rng = np.random.default_rng(20260)
    cases = []
    cases.append(_case("no reads", [], 3, 5, 0, lambda c, tr: len(c["reads"]) == 0))
    cases.append(_case("a read without candidates beside others", [[(0, 7)], [], [(0, 1), (2, 4096)], [], [(1, 3), (2, 3)]], 4, 20, 0,
                       lambda c, tr: sum(1 for r in c["reads"] if not r) == 2))
    sizes = [1, 2, 3, 63, 64, 64, 1, 63, 2, 3]
    cases.append(_case("1, 2, 3, 63 and 64 candidates", [_read(rng, n, 70) for n in sizes], 70, 6, 0,
                       lambda c, tr: {len(r) for r in c["reads"]} == {1, 2, 3, 63, 64}))
    # packing: 40 + 30 would straddle (padding), 34 + 30 fill a row exactly, 32 + 32 again, 62 + 2 exactly, then a row that ends in padding
    psizes = [40, 30, 34, 1, 32, 32, 0, 62, 2, 5, 61, 3]
    cases.append(_case("rows with padding, rows filled exactly, reads that would have straddled", [_read(rng, n, 90) for n in psizes], 90, 6, 0,
                       lambda c, tr: all(v >= 2 for v in pack_events(c["reads"]))))
    cases.append(_case("weights 1 and 4096 in one read", [[(0, 1), (1, 4096)], [(1, 1), (2, 4096), (0, 1)], [(2, 1)]], 3, 30, 0,
                       lambda c, tr: any({1, 4096} <= {w for _, w in r} for r in c["reads"])))
    cases.append(_case("by hand: reads {A} and {A, B}", [[(0, 1)], [(0, 1), (1, 1)]], 2, 1, 0,
                       lambda c, tr: tr[0][0] == [ONE + ONE // 2, ONE // 2] and tr[1][0] == [ONE + 3 * ONE // 4, ONE // 4]))
    cases.append(_case("a count that reaches 0", [[(0, 1)]] * 300 + [[(0, 4096), (1, 1)]], 2, 4, 0,
                       lambda c, tr: tr[0][0][1] == 255 and all(t[0][1] == 0 for t in tr[1:]) and len(tr) >= 3))
    cases.append(_case("the shift: 5000 single reads", [[(0, 1)]] * 5000 + [[(0, 4096), (1, 4096)], [(2, 9), (0, 4096)], [(1, 1), (2, 1)]], 3, 4, 0,
                       lambda c, tr: max(t[1] for t in tr) >= 1))
    cases.append(_case("the shift: 140000 single reads", [[(0, 1)]] * 140000 + [[(0, 4096), (1, 4096)], [(2, 4096), (1, 77), (0, 4096)]], 3, 2, 0,
                       lambda c, tr: max(t[1] for t in tr) >= 5))
    hot = [[(0, int(rng.integers(1, 4097))), (int(rng.integers(1, 40)), int(rng.integers(1, 4097)))] for _ in range(20000)]
    cases.append(_case("a hot transcript: 20000 two-candidate reads that name transcript 0", hot, 40, 3, 0,
                       lambda c, tr: len(c["reads"]) == 20000 and all(r[0][0] == 0 and len(r) == 2 for r in c["reads"])))
    mid = _random_reads(rng, 300, 25, [0, 1, 1, 2, 2, 3, 5, 8])
    for mi in (0, 1, 2):
        cases.append(_case(f"max_iter {mi}", mid, 25, mi, 0, lambda c, tr, mi=mi: len(tr) == mi + 1))
    cases.append(_case("stops by tol before max_iter", mid, 25, 1000, 4096, lambda c, tr: 1 < len(tr) - 1 < 1000))
    cases.append(_case("does not stop by tol", mid, 25, 7, 0, lambda c, tr: len(tr) - 1 == 7))
    many = _random_reads(rng, 3000, 200, [1, 1, 1, 2, 3, 4, 6, 9, 17, 33], wmax=64)
    cases.append(_case("3000 reads over several workgroups", many, 200, 12, 0, lambda c, tr: sum(len(r) for r in c["reads"]) > 4 * 256))
    return cases


REFUSALS = (  # (name, reads or None for a hand-made CSR, n_tx) -- each must be RD_ERR_ARG with every output untouched
    ("a duplicate t in a read", [[(0, 1)], [(1, 2), (2, 2), (1, 3)]], 3),
    ("t out of range", [[(0, 1), (3, 1)]], 3),
    ("t negative", [[(-1, 1)]], 3),
    ("w = 0", [[(0, 1), (1, 0)]], 3),
    ("w = 4097", [[(0, 4097)]], 3),
    ("65 candidates", [[(t, 1) for t in range(65)]], 70),
)


# ---- candidate cases ------------------------------------------------------------------------------------------------------------
def copies_case():
    """one read against 70 copies of one transcript: 70 equal chains, kept in ascending t"""
    rng = np.random.default_rng(31)
    T = rng.integers(0, 4, size=900, dtype=np.uint8)
    return [T.copy() for _ in range(70)], [mr.mutate(rng, T[100:800], 0.08)]


def many_segments_case():
    """one read against 2100 copies of a short transcript (indexed with max_occ = 4000): a read with thousands of segments, over many
    64-segment rounds of the candidate kernel's two loops"""
    rng = np.random.default_rng(33)
    T = rng.integers(0, 4, size=220, dtype=np.uint8)
    return [T.copy() for _ in range(2100)], [mr.mutate(rng, T[20:210], 0.04)]


def edge_case():
    """transcripts: two unrelated, one gene of three isoforms (each skipping one inner exon).  reads: 0 the middle of an unrelated
    transcript (its only chain ends far from the 3' end); 1 the last 500 bases of transcript 1, exact (d3 = 0); 2 the same with 60 bases
    of tail appended (d3 = -60: the read runs past the transcript's end); 3 a shared stretch of the gene, exact; 4, 5 mutated reads of
    isoforms, one ending at the 3' end; 6 no seed"""
    rng = np.random.default_rng(32)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    u0, u1 = rnd(1800), rnd(1200)
    exons = [rnd(int(rng.integers(150, 400))) for _ in range(8)]
    iso = [np.concatenate([e for j, e in enumerate(exons) if j != s]) for s in (2, 4, 5)]
    transcripts = [u0, u1] + iso
    shared = np.concatenate(exons[6:])
    reads = [u0[500:1100].copy(), u1[-500:].copy(), np.concatenate([u1[-500:], np.zeros(60, dtype=np.uint8)]), shared[-450:].copy(),
             mr.mutate(rng, iso[0][200:1200], 0.12), mr.mutate(rng, iso[2][-700:], 0.12), rnd(300)]
    return transcripts, reads


CAND_PARAMS = (dict(max_cand=16, min_frac_q10=922, max_3p=-1), dict(max_cand=16, min_frac_q10=0, max_3p=-1),
               dict(max_cand=16, min_frac_q10=1024, max_3p=-1), dict(max_cand=16, min_frac_q10=922, max_3p=0),
               dict(max_cand=16, min_frac_q10=922, max_3p=50), dict(max_cand=2, min_frac_q10=0, max_3p=50))
