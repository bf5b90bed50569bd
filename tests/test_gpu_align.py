"""GPU checks of the read-accuracy evaluation (rd_align_batch / Backend.align / python -m radian_amd.align) against the CPU
restatement (tests/_align_ref.py): optimal scores, the tie-broken alignment, the soft clip and counts, batching under a budget,
and the command line end to end; the same outputs under every score set of tests/_align_ref.py (linear gaps, scores at the int32
bound), and the refusals of a pair past that bound and of gap_open > gap_extend with the outputs untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_ref as aref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_pairs(rng):
    def rnd(n):
        return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))

    def mutate(s, p=0.12):
        out = bytearray()
        for c in s:
            r = rng.random()
            if r < p / 3:
                continue
            out.append(c if r > p else int(rng.choice(list(b"ACGT"))))
            if rng.random() < p / 3:
                out.append(int(rng.choice(list(b"ACGT"))))
        return bytes(out)

    pairs = []
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129):
        for m in (1, 63, 64, 65, 128, 129):
            a = rnd(n)
            pairs.append((a, mutate(a) if n > 8 else rnd(m)))
            pairs.append((rnd(n), rnd(m)))
    x = rnd(300)
    pairs += [(x, x), (b"A" * 200, b"C" * 200), (rnd(3000), rnd(40)), (rnd(40), rnd(3000)), (rnd(1), rnd(2000)), (rnd(2000), rnd(1)),
              (b"ACGTN" * 40, b"ACGT" * 50), (b"", rnd(10)), (rnd(10), b""), (b"", b"")]
    big = rnd(20000)
    pairs.append((big, mutate(big)))
    return pairs


@pytest.fixture(scope="module")
def workload():
    from radian_amd import synthetic
    _, refs, reads = synthetic.alignment_pairs(2000, seed=11, median_len=300)
    # substitutions only, no junk: pairs whose optimal alignment is mostly unique
    _, r2, q2 = synthetic.alignment_pairs(200, seed=12, median_len=200, p_sub=0.03, p_ins=0.0, p_del=0.0, max_junk=0)
    refs = [r.encode() for r in refs + r2]
    reads = [q.replace("U", "T").encode() for q in reads + q2]
    for a, b in _edge_pairs(np.random.default_rng(5)):
        refs.append(a)
        reads.append(b)
    score, nopt, ops = aref.align_cpu(refs, reads)
    return refs, reads, score, nopt, ops


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def test_align_matches_cpu_restatement(be, workload):
    from radian_amd.backend import align_clip_count
    refs, reads, score, nopt, ops = workload
    res = be.align(refs, reads, with_ops=True)
    bad = np.nonzero(res.score.astype(np.int64) != score)[0]
    assert bad.size == 0, [(int(p), len(refs[p]), len(reads[p]), int(res.score[p]), int(score[p])) for p in bad[:10]]
    unique = 0
    for p in range(len(refs)):
        got = res.ops[p]
        assert aref.rescore(got, refs[p], reads[p]) == score[p], p       # optimal, and consumes both sequences exactly
        assert got == ops[p], (p, len(refs[p]), len(reads[p]))           # the same tie-break
        cnt, st = align_clip_count(ops[p], refs[p], reads[p])
        assert res.status[p] == st and tuple(int(c) for c in res.counts[p]) == cnt, p
        unique += int(nopt[p] == 1)
    print(f"\n{len(refs)} pairs, {unique} with a unique optimal alignment (their counts are the reference's)")
    assert unique >= 50


def test_align_without_ops_and_batch_order_invariance(be, workload):
    refs, reads, score, _, _ = workload
    res = be.align(refs, reads)
    assert res.ops is None and np.array_equal(res.score.astype(np.int64), score)
    perm = np.random.default_rng(9).permutation(len(refs))
    sh = be.align([refs[p] for p in perm], [reads[p] for p in perm], budget_bytes=256 << 20)   # several batches
    assert np.array_equal(sh.score, res.score[perm])
    assert np.array_equal(sh.counts, res.counts[perm])
    assert np.array_equal(sh.status, res.status[perm])


def test_tiny_budget_reports_the_big_pair_and_aligns_the_rest(be, workload):
    from radian_amd import RadianHipError
    from radian_amd.backend import ALIGN_TOO_LARGE, align_workspace_bytes
    refs, reads, score, _, _ = workload
    big = max(range(len(refs)), key=lambda p: len(refs[p]) * len(reads[p]))
    budget = align_workspace_bytes(3000, 3000)
    assert align_workspace_bytes(len(refs[big]), len(reads[big])) > budget
    with pytest.raises(RadianHipError) as ei:
        be.align(refs, reads, budget_bytes=budget)
    assert "[rd error -4]" in str(ei.value) and f"pair {big} " in str(ei.value)
    res = be.align(refs, reads, budget_bytes=budget, allow_too_large=True)
    assert res.status[big] == ALIGN_TOO_LARGE
    rest = np.arange(len(refs)) != big
    assert np.array_equal(res.score[rest].astype(np.int64), score[rest])
    assert (res.status[rest] != ALIGN_TOO_LARGE).all()


def test_command_line_end_to_end(tmp_path):
    from radian_amd import synthetic
    from radian_amd.backend import align_clip_count
    ids, refs, reads = synthetic.alignment_pairs(300, seed=23, median_len=400)
    fa, tsv = tmp_path / "calls.fasta", tmp_path / "refs.tsv"
    synthetic.write_alignment_inputs(str(fa), str(tsv), ids, refs, reads)
    p = subprocess.run([sys.executable, "-m", "radian_amd.align", str(fa), str(tsv), "--dump-alignments", str(tmp_path / "aln.txt")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    exp_out = tmp_path / "expected.tsv"
    exp_stdout = aref.reference_main(str(fa), str(tsv), align_clip_count, str(exp_out))
    assert (tmp_path / "calls.tsv").read_bytes() == exp_out.read_bytes()
    assert p.stdout == exp_stdout
    assert (tmp_path / "aln.txt").read_text().count("\n") == 4 * 300


# ---------------------------------------------------------------------------------------------- scores other than 2 / -4 / -4 / -2
_SET_ID = lambda sc: "_".join(str(v) for v in sc)


@pytest.fixture(scope="module")
def set_pairs():
    pairs = aref.score_set_pairs()
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _check_against_restatement(be, refs, reads, sc, budget_bytes):
    """every output of Backend.align under the scores sc == the restatement's, exactly; returns the restatement's ops"""
    from radian_amd.backend import align_clip_count
    score, _, ops = aref.align_cpu(refs, reads, sc)
    res = be.align(refs, reads, scores=sc, with_ops=True)
    bad = np.nonzero(res.score.astype(np.int64) != score)[0]
    assert bad.size == 0, (sc, [(int(p), len(refs[p]), len(reads[p]), int(res.score[p]), int(score[p])) for p in bad[:10]])
    for p in range(len(refs)):
        assert res.ops[p] == ops[p], (sc, p, len(refs[p]), len(reads[p]))                     # the same tie-break
        assert aref.rescore(res.ops[p], refs[p], reads[p], sc) == score[p], (sc, p)           # its columns add up to the score
        cnt, st = align_clip_count(ops[p], refs[p], reads[p])
        assert res.status[p] == st and tuple(int(c) for c in res.counts[p]) == cnt, (sc, p)
    plain = be.align(refs, reads, scores=sc)
    assert plain.ops is None and np.array_equal(plain.score, res.score) and np.array_equal(plain.counts, res.counts)
    perm = np.random.default_rng(9).permutation(len(refs))
    sh = be.align([refs[p] for p in perm], [reads[p] for p in perm], scores=sc, budget_bytes=budget_bytes)
    assert np.array_equal(sh.score, res.score[perm]) and np.array_equal(sh.counts, res.counts[perm]) and np.array_equal(sh.status, res.status[perm])
    return ops


@pytest.mark.parametrize("sc", aref.SMALL_SETS, ids=_SET_ID)
def test_align_under_every_score_set(be, set_pairs, sc):
    """Linear gaps (every open bit of align_fwd_kernel decided on a tie), a zero match score, a zero and a positive mismatch score, free
    extension, an expensive opening: scores, ops, counts and status equal the restatement's on lengths around the 64-row tile and the
    64-column chunk and on pairs with very many co-optimal alignments; the same without ops and in several batches.  The set's ops
    hold gap runs of both kinds and a substitution, so no branch of the two kernels passes unvisited."""
    from radian_amd.backend import align_workspace_bytes
    refs, reads = set_pairs
    budget = 6 * align_workspace_bytes(129, 129)
    assert sum(align_workspace_bytes(len(a), len(b)) for a, b in zip(refs, reads)) > 3 * budget        # several batches
    ops = _check_against_restatement(be, refs, reads, sc, budget)
    assert aref.longest_run(ops, ord("D")) >= 2 and aref.longest_run(ops, ord("I")) >= 2, sc
    # a D column and an I column replace an X column for two openings: where that scores more, no optimal alignment holds an X
    assert (aref.longest_run(ops, ord("X")) >= 1) == aref.can_substitute(sc), sc


@pytest.fixture(scope="module")
def bound_pair():
    """n + m = 4095: at |score| = 65535 the longest pair the argument check admits (65535 * 4096 < 2^28)"""
    rng = np.random.default_rng(43)
    a = bytes(rng.choice(list(b"ACGT"), 2048).astype(np.uint8))
    b = (aref._mutate(rng, a, b"ACGT") + bytes(rng.choice(list(b"ACGT"), 200).astype(np.uint8)))[:2047]
    assert len(a) + len(b) == 4095
    return a, b


@pytest.mark.parametrize("sc", aref.BOUND_SETS, ids=_SET_ID)
def test_align_at_the_int32_bound(be, set_pairs, bound_pair, sc):
    """the largest scores the entry point takes, on the longest pair it then admits and on some of the edge pairs: exact against the
    int64 restatement, so neither -2^30 nor a sum near 2^28 is reached or wrapped"""
    from radian_amd.backend import align_workspace_bytes
    refs, reads = set_pairs
    pick = [p for p in range(len(refs)) if (len(refs[p]), len(reads[p])) in ((1, 1), (3, 129), (129, 3), (64, 64), (65, 127), (128, 63), (129, 129))]
    pick += list(range(len(refs) - 11, len(refs)))                                                    # the tie-heavy pairs and the empty ones
    refs, reads = [refs[p] for p in pick] + [bound_pair[0]], [reads[p] for p in pick] + [bound_pair[1]]
    assert 65535 * (4095 + 1) < 1 << 28 <= 65535 * (4096 + 1)
    ops = _check_against_restatement(be, refs, reads, sc, align_workspace_bytes(2048, 2047))
    assert aref.longest_run(ops, ord("D")) >= 2 and aref.longest_run(ops, ord("I")) >= 2, sc


def _raw_align(be, refs, reads, sc, fill=-7):
    """rd_align_batch on pre-filled outputs: (rc, error text, whether every output still holds the fill)"""
    from radian_amd.backend import _concat, _p
    n = len(refs)
    rbuf, roff = _concat(refs)
    qbuf, qoff = _concat(reads)
    score, status, ops_len = (np.full(n, fill, dtype=np.int32) for _ in range(3))
    counts = np.full((n, 4), fill, dtype=np.int32)
    ops_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((roff[1:] - roff[:-1]) + (qoff[1:] - qoff[:-1]), out=ops_off[1:])
    ops = np.full(max(int(ops_off[-1]), 1), 0x5a, dtype=np.uint8)
    rc = be._L.rd_align_batch(be._h, _p(rbuf), _p(roff), _p(qbuf), _p(qoff), n, *(int(v) for v in sc), 0, _p(score), _p(counts), _p(status),
                              _p(ops), _p(ops_off), _p(ops_len))
    untouched = all((x == fill).all() for x in (score, status, ops_len, counts)) and (ops == 0x5a).all()
    return rc, be._L.rd_last_error().decode(), untouched


def test_pair_past_the_int32_bound_is_refused_before_any_output(be, bound_pair):
    a, b = bound_pair
    refs, reads = [b"ACGT", b"AC", a], [b"ACT", b"", b + b"A"]                                       # pair 2: n + m = 4096
    rc, msg, untouched = _raw_align(be, refs, reads, aref.BOUND_SETS[0])
    assert rc == -1 and untouched and "rd_align_batch: pair 2 (2048 x 2048) is too long for int32 scores" in msg, (rc, msg)
    rc, msg, untouched = _raw_align(be, refs, reads, aref.BOUND_SETS[1])
    assert rc == -1 and untouched and "pair 2 (2048 x 2048)" in msg, (rc, msg)
    rc, msg, untouched = _raw_align(be, refs[:2] + [a], reads[:2] + [b], aref.BOUND_SETS[0])        # n + m = 4095 goes through
    assert rc == 0 and not untouched, (rc, msg)


def test_gap_open_above_gap_extend_is_refused_before_any_output(be):
    """with open > extend the recurrence reopens adjacent gaps: its score is not the stated gap cost (tests/test_align_cpu.py)"""
    from radian_amd import RadianHipError
    refs, reads = [b"ACGTACGT", b"AC", b""], [b"ACTTACG", b"", b"G"]
    for sc in (aref.REFUSED_SET, (2, -4, -2, -4)):
        rc, msg, untouched = _raw_align(be, refs, reads, sc)
        assert rc == -1 and untouched and msg.startswith("rd_align_batch: gap_open") and "gap_open <= gap_extend" in msg, (sc, rc, msg)
        with pytest.raises(RadianHipError, match="gap_open <= gap_extend"):
            be.align(refs, reads, scores=sc)
    rc, msg, untouched = _raw_align(be, refs, reads, (2, -4, -3, -3))                               # equality, linear gaps, is legal
    assert rc == 0 and not untouched, (rc, msg)
    assert np.array_equal(be.align(refs, reads, scores=(2, -4, -3, -3)).score, aref.align_cpu(refs, reads, (2, -4, -3, -3))[0])
