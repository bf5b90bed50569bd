"""GPU checks of the read-accuracy evaluation (rd_align_batch / Backend.align / python -m radian_amd.align) against the CPU
restatement (tests/_align_ref.py): optimal scores, the tie-broken alignment, the soft clip and counts, batching under a budget,
and the command line end to end."""
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
