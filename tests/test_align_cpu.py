"""No-GPU checks of the read-accuracy evaluation (radian_amd.align, rd_align_*): the library's clip-and-count against the reference's
own analyse_alignment (tests/golden/align_clip_cases.json), the command line's parsing, output path and summary, the CPU
restatement (tests/_align_ref.py) against brute force, and the GPU entry point failing loudly without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_ref as aref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "align_clip_cases.json")


@pytest.fixture(scope="module")
def lib():
    from radian_amd import build, _lib
    build.build()
    return _lib.load()


def _columns_to_ops(gt, mid, pred):
    ops, ref, read = [], [], []
    for g, m, p in zip(gt, mid, pred):
        if g == "-":
            ops.append("I"), read.append(p)
        elif p == "-":
            ops.append("D"), ref.append(g)
        else:
            ops.append("M" if m == "|" else "X"), ref.append(g), read.append(p)
    return "".join(ops), "".join(ref), "".join(read)


def test_clip_count_equals_the_reference_golden(lib):
    from radian_amd.backend import ALIGN_CLIP_INDEX_ERROR, ALIGN_EMPTY_AFTER_CLIP, ALIGN_OK, align_clip_count
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 500
    seen = set()
    for c in cases:
        ops, ref, read = _columns_to_ops(c["gt"], c["mid"], c["pred"])
        cnt, st = align_clip_count(ops, ref, read)
        if c["out"] == "IndexError":
            assert st == ALIGN_CLIP_INDEX_ERROR, (c, cnt, st)
            seen.add("index")
        else:
            assert st in (ALIGN_OK, ALIGN_EMPTY_AFTER_CLIP), (c, st)
            assert list(cnt) == c["out"], (c, cnt)
            seen.add("empty" if st == ALIGN_EMPTY_AFTER_CLIP else "ok")
    assert seen == {"index", "empty", "ok"}


def test_clip_count_wraps_negative_indices_and_skips_n(lib):
    from radian_amd.backend import ALIGN_OK, align_clip_count
    from radian_amd.backend import ALIGN_EMPTY_AFTER_CLIP, ALIGN_CLIP_INDEX_ERROR
    # "MMI": clip_start runs to the last column (2) without a break; clip_end scans back, column 1 looks at 0 and -1 (= column 2,
    # a ref gap), column 0 at -1 and -2: no break, clip_end = 0 < clip_start: nothing left
    assert align_clip_count("MMI", "AC", "ACG") == ((0, 0, 0, 0), ALIGN_EMPTY_AFTER_CLIP)
    # "MM": clip_start reads gt[2]
    assert align_clip_count("MM", "AC", "AC")[1] == ALIGN_CLIP_INDEX_ERROR
    assert align_clip_count("", "", "") == ((0, 0, 0, 0), ALIGN_EMPTY_AFTER_CLIP)
    assert align_clip_count("IMMMXI", "ACGT", "GACGAC") == ((3, 1, 0, 0), ALIGN_OK)
    # a deletion of N and an insertion of N count as nothing
    assert align_clip_count("MMMDIMMM", "AAANCCC", "AAANCCC")[0] == (6, 0, 0, 0)
    assert align_clip_count("MMMDIMMM", "AAAGCCC", "AAATCCC")[0] == (6, 0, 1, 1)
    with pytest.raises(Exception):
        align_clip_count("MQ", "AC", "AC")


def test_workspace_bytes(lib):
    from radian_amd.backend import align_workspace_bytes
    small, big = align_workspace_bytes(100, 100), align_workspace_bytes(20000, 20000)
    assert 0 < small < big
    assert 0.5 * 20000 * 20000 <= big <= 0.6 * 20000 * 20000   # four direction bits per cell + boundary rows and sequences
    assert align_workspace_bytes(0, 5) > 0 and align_workspace_bytes(-1, 5) == -1


def test_cpu_restatement_against_brute_force():
    """score and number of optimal alignments of tiny pairs by enumerating every alignment; the tie-broken traceback is optimal"""
    rng = np.random.default_rng(3)

    def all_alignments(a, b):
        if not a and not b:
            yield ""
            return
        if a and b:
            for rest in all_alignments(a[1:], b[1:]):
                yield ("M" if a[0] == b[0] else "X") + rest
        if a:
            for rest in all_alignments(a[1:], b):
                yield "D" + rest
        if b:
            for rest in all_alignments(a, b[1:]):
                yield "I" + rest

    pairs = [(b"", b""), (b"A", b""), (b"", b"AC"), (b"A", b"A"), (b"AC", b"CA")]
    for _ in range(60):
        n, m = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        pairs.append((bytes(rng.choice(list(b"ACG"), n).astype(np.uint8)), bytes(rng.choice(list(b"ACG"), m).astype(np.uint8))))
    score, nopt, ops = aref.align_cpu([p[0] for p in pairs], [p[1] for p in pairs])
    for k, (a, b) in enumerate(pairs):
        sc = [aref.rescore(o.encode(), a, b) for o in all_alignments(a, b)]
        best = max(sc)
        assert score[k] == best, (a, b)
        assert nopt[k] == min(sc.count(best), 2), (a, b, sc.count(best))
        assert aref.rescore(ops[k], a, b) == best


def test_cpu_tie_break_order():
    # one ref base against a two-base read with a mismatch either way: diagonal first, so the insertion comes last
    _, _, ops = aref.align_cpu([b"A", b"AC"], [b"CA", b"A"])
    assert ops[0] == b"IM"        # only one optimum: the match
    assert ops[1] == b"MD"
    _, nopt, ops = aref.align_cpu([b"AA"], [b"A"])
    assert nopt[0] == 2 and ops[0] == b"DM"   # at (2, 1) the diagonal ties with the deletion and wins: the gap goes first


@pytest.fixture(scope="module")
def small_pairs():
    return aref.small_pairs()


@pytest.mark.parametrize("sc", aref.ACCEPTED_SETS, ids=lambda sc: "_".join(str(v) for v in sc))
def test_restatement_equals_the_three_state_model_under_every_accepted_score_set(small_pairs, sc):
    """gap_open <= gap_extend: Gotoh's recurrence (the restatement, the kernels) is the stated gap cost.  The model is written
    independently (a gap is entered only from another state); the traceback's columns add up to the score; the pairs tie heavily."""
    refs, reads = [p[0] for p in small_pairs], [p[1] for p in small_pairs]
    score, nopt, ops = aref.align_cpu(refs, reads, sc)
    for k, (a, b) in enumerate(small_pairs):
        assert int(score[k]) == aref.three_state(a, b, sc), (k, sc)
        assert aref.rescore(ops[k], a, b, sc) == score[k], (k, sc)
    assert 2 * int((nopt >= 2).sum()) >= len(small_pairs), (sc, nopt.tolist())


def test_open_above_extend_is_not_the_stated_gap_cost(small_pairs):
    """Why the entry points refuse gap_open > gap_extend (include/radian_hip.h): at (1, -2, -1, -3) the recurrence closes a gap and
    reopens it in the next column for 2 * open, where one gap of length 2 costs open + extend.  Its score is then above the optimum of
    the stated cost model, and the traced columns do not add up to it.  Relaxing the refusal brings this back."""
    sc = aref.REFUSED_SET
    assert sc[2] > sc[3]
    refs, reads = [p[0] for p in small_pairs], [p[1] for p in small_pairs]
    score, _, ops = aref.align_cpu(refs, reads, sc)
    model = [aref.three_state(a, b, sc) for a, b in small_pairs]
    differ = [k for k in range(len(small_pairs)) if int(score[k]) != model[k]]
    assert differ, "the recurrence and the cost model agree on every pair: the counter-example is gone"
    assert all(int(score[k]) > model[k] for k in differ)        # never below: every alignment of the model is a path of the recurrence
    assert any(aref.rescore(ops[k], refs[k], reads[k], sc) != score[k] for k in range(len(small_pairs)))
    # equality (linear gaps) has no such case
    for k, (a, b) in enumerate(small_pairs[:8]):
        assert int(aref.gotoh_batch([a], [b], (1, -2, -3, -3))[0][0]) == aref.three_state(a, b, (1, -2, -3, -3)), k


def test_score_set_pairs_cover_every_branch_under_every_set():
    """what tests/test_gpu_align.py asserts of the device's ops holds for the restatement's: under every set the tie-broken alignments
    of its pairs hold a run of two or more D, a run of two or more I, and an X wherever an optimal alignment can hold one"""
    pairs = aref.score_set_pairs()
    refs, reads = [p[0] for p in pairs], [p[1] for p in pairs]
    assert {len(r) for r in refs} >= {0, 1, 2, 3, 63, 64, 65, 127, 128, 129} and max(len(s) for s in refs + reads) <= 140
    for sc in aref.SMALL_SETS:
        _, nopt, ops = aref.align_cpu(refs, reads, sc)
        assert aref.longest_run(ops, ord("D")) >= 2 and aref.longest_run(ops, ord("I")) >= 2, sc
        assert (aref.longest_run(ops, ord("X")) >= 1) == aref.can_substitute(sc), sc
        assert 2 * int((nopt >= 2).sum()) >= len(pairs), sc
    assert [sc for sc in aref.SMALL_SETS if not aref.can_substitute(sc)] == [(2, -4, 0, 0)]


def test_fasta_and_tsv_parsing(tmp_path):
    from radian_amd import align
    fa = tmp_path / "x.fasta"
    fa.write_text("junk before\n>r1 some description\nACGU\nUUA \n\n>r2\n>r3\tx\r\nAC GT\r\n")
    assert align.read_fasta(str(fa)) == [("r1", "ACGUUUA"), ("r2", ""), ("r3", "ACGT")]
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("read\ttxt\tseq\nr1\tt\tACGT\nr2\tt\tGG\nr1\tt\tTTTT\n")
    assert align.read_ref_tsv(str(tsv)) == {"r1": "TTTT", "r2": "GG"}
    tsv.write_text("h\nr1\tACGT\n")
    with pytest.raises(ValueError):
        align.read_ref_tsv(str(tsv))


def test_output_path_rule():
    from radian_amd import align
    assert align.output_path("runs/a.fasta") == "runs/a.tsv"
    assert align.output_path("x.fasta.d/a.fasta") == "x.tsv.d/a.tsv"   # str.replace on the whole path, as the reference
    with pytest.raises(SystemExit):
        align.output_path("reads.fa")


def test_summary_format():
    from radian_amd import align
    stats = [align.rates(90, 4, 3, 3), align.rates(45, 5, 0, 0)]
    # read 1: 100 columns -> 90 / 3 / 3 / 4 / 10 %; read 2: 50 columns -> 90 / 0 / 0 / 10 / 10 %
    assert align.summary(stats) == ("Accuracy\tMEDIAN: 90.00\tMEAN: 90.00\n"
                                    "Insertions\tMEDIAN: 1.50\tMEAN: 1.50\n"
                                    "Deletions\tMEDIAN: 1.50\tMEAN: 1.50\n"
                                    "Substitutions\tMEDIAN: 7.00\tMEAN: 7.00\n\n"
                                    "Total error\tMEDIAN: 10.00\tMEAN: 10.00\n\n")


def test_missing_id_raises_keyerror_before_writing(tmp_path):
    fa = tmp_path / "r.fasta"
    fa.write_text(">a\nACGU\n>missing\nACGT\n")
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("h\th\th\na\tt\tACGT\n")
    p = subprocess.run([sys.executable, "-m", "radian_amd.align", str(fa), str(tsv)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0
    assert p.stderr.strip().splitlines()[-1] == "KeyError: 'missing'"
    assert not (tmp_path / "r.tsv").exists()


def test_output_path_equal_to_input_is_refused(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_text(">a\nACGT\n")
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("h\na\tt\tACGT\n")
    p = subprocess.run([sys.executable, "-m", "radian_amd.align", str(fa), str(tsv)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "overwrite" in p.stderr
    assert fa.read_text() == ">a\nACGT\n"


def test_align_fails_loudly_without_gpu(lib, tmp_path):
    n = ctypes.c_int(-1)
    lib.rd_device_count(ctypes.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is present")
    fa = tmp_path / "r.fasta"
    fa.write_text(">a\nACGU\n")
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("h\na\tt\tACGT\n")
    p = subprocess.run([sys.executable, "-m", "radian_amd.align", str(fa), str(tsv)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "no CPU fallback" in p.stderr
    assert not (tmp_path / "r.tsv").exists()


def test_synthetic_workload_shape():
    from radian_amd import synthetic
    ids, refs, reads = synthetic.alignment_pairs(400, seed=7)
    assert len(set(ids)) == 400
    lens = np.array([len(r) for r in refs])
    assert 1200 < np.median(lens) < 1900
    assert any("U" in q for q in reads) and any("N" in r for r in refs)
    assert all(set(q) <= set("ACGTU") for q in reads)
    assert synthetic.alignment_pairs(3, seed=7) == synthetic.alignment_pairs(3, seed=7)
