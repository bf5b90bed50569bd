"""No-GPU checks of the signal-to-reference alignment: the plain-Python restatement of the event contract
(tests/_events_ref.py) on hand-checkable cases, rd_event_stats_host against it, the partition property on real forced alignments
(tests/_ctcalign_ref.py), the host formulas and the TSV layout of radian_amd/resquiggle.py, and the host code of events.hip under
AddressSanitizer + UBSan (tests/asan_events.cpp).  Every comparison is for equality."""
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _ctcalign_ref as caref
import _events_ref as ref
from _events_cases import LENGTHS, NO_PATH, OK, aln_of as _aln, mutated_alignment_cases, raw_call as _raw_call, refusal_cases, same_events, seeded_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return seeded_cases()


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_one_label_fills_the_read():
    ev = ref.events([3, -4, 5, 7], [0], [3])
    assert ev == {"start": [0], "end": [4], "n": [4], "sum": [11], "sumsq": [9 + 16 + 25 + 49], "min": [-4], "max": [7]}
    assert ref.partitions(ev, [0], [3])


def test_restatement_leading_and_trailing_blanks_belong_to_no_event():
    raw = [100, 1, 2, 3, 4, 5, 6, 100, 100]
    first, last = [1, 3, 4], [1, 3, 6]          # label 0 owns the blank row 2; rows 0, 7 and 8 are outside
    ev = ref.events(raw, first, last)
    assert ev["start"] == [1, 3, 4] and ev["end"] == [3, 4, 7] and ev["n"] == [2, 1, 3]
    assert ev["sum"] == [3, 3, 15] and ev["sumsq"] == [5, 9, 16 + 25 + 36] and ev["min"] == [1, 3, 4] and ev["max"] == [2, 3, 6]
    assert sum(ev["n"]) == last[-1] + 1 - first[0] == 6 and ref.partitions(ev, first, last)


def test_restatement_events_of_one_sample_and_no_path():
    ev = ref.events([-7, 8, -9], [0, 1, 2], [0, 1, 2])
    assert ev["n"] == [1, 1, 1] and ev["sum"] == [-7, 8, -9] and ev["min"] == ev["max"] == [-7, 8, -9] and ev["sumsq"] == [49, 64, 81]
    nop = ref.events([1, 2, 3], [-1, -1], [-1, -1], status=NO_PATH)
    assert nop == {"start": [-1, -1], "end": [-1, -1], "n": [0, 0], "sum": [0, 0], "sumsq": [0, 0], "min": [0, 0], "max": [0, 0]}
    assert ref.events([1, 2], [], []) == {k: [] for k in nop}


# ---------------------------------------------------------------------------------------------- the host entry point
def test_event_stats_host_equals_the_restatement(cases):
    from radian_amd.backend import event_stats_host
    raws, firsts, lasts, status, exp = cases
    got = event_stats_host(raws, _aln(firsts, lasts, status))
    for r in range(len(raws)):
        same_events(got, r, exp[r])
        if status[r] == OK:
            assert ref.partitions(exp[r], firsts[r], lasts[r])
    # the int16 extremes in events of 70 000 samples: the sum of squares passes 2^32 and the sum leaves int32 on either side (70 000 samples
    # cannot take a sum past 2^32: 70 000 * 32 768 < 2^32)
    big = exp[3]
    assert big["n"][1:4] == [70000] * 3 and big["sum"][1] == -70000 * 32768 < -2 ** 31 and big["sum"][2] == 70000 * 32767 > 2 ** 31
    assert min(big["sumsq"][1:4]) > 2 ** 32 and big["min"][3] == -32768 and big["max"][3] == 32767
    assert all(set(LENGTHS) <= set(e["n"]) for e in exp[:3])       # (a read's last event ends with its label's own rows)
    # one read per call and the reads in reversed order: the same values
    rev = event_stats_host(raws[::-1], _aln(firsts[::-1], lasts[::-1], status[::-1]))
    for r in range(len(raws)):
        same_events(rev, len(raws) - 1 - r, exp[r])
        same_events(event_stats_host([raws[r]], _aln([firsts[r]], [lasts[r]], [status[r]])), 0, exp[r])


def test_event_stats_host_refuses_bad_arguments():
    from radian_amd import _lib
    L = _lib.load()
    good, bad = refusal_cases()
    assert _raw_call(L.rd_event_stats_host, **good) == 0
    for name, kw in bad:
        assert _raw_call(L.rd_event_stats_host, **kw) == -1, name   # RD_ERR_ARG
        assert L.rd_last_error()
    # the steps of a read without a path are not looked at
    assert _raw_call(L.rd_event_stats_host, **{**good, "first": [-1, -1, -1], "last": [-1, -1, -1], "status": [NO_PATH]}) == 0


# ---------------------------------------------------------------------------------------------- real alignments partition the signal
def test_events_of_real_alignments_partition_the_signal():
    from radian_amd.backend import event_stats_host
    cases = mutated_alignment_cases()
    res = [caref.align_fast(P, lab) for P, lab, _ in cases]
    assert [r.status for r in res] == [caref.OK] * len(cases)          # no no-path read at all
    got = event_stats_host([raw for _, _, raw in cases], _aln([r.first_step for r in res], [r.last_step for r in res], [r.status for r in res]))
    n_events = 0
    for i, ((P, lab, raw), r) in enumerate(zip(cases, res)):
        exp = ref.events(raw, r.first_step, r.last_step)
        assert ref.partitions(exp, r.first_step, r.last_step), i
        same_events(got, i, exp)
        n_events += len(lab)
    assert n_events > 4000


# ---------------------------------------------------------------------------------------------- host formulas and files of the command
def test_mean_stdv_level_formulas():
    from radian_amd import resquiggle as rq
    mean, stdv = rq.event_moments(4, 3 - 4 + 5 + 8, 9 + 16 + 25 + 64)
    assert mean == 3.0 and stdv == math.sqrt(114 / 4 - 9.0)
    assert rq.event_moments(3, 21, 147) == (7.0, 0.0)                       # a constant event
    assert rq.event_moments(3, 3 * 32767, 3 * 32767 * 32767)[1] == 0.0     # the variance's argument is clamped at 0
    raw = np.array([10, 12, 11, 30, 9, 10, 13], dtype=np.int16)
    median, mad = rq.read_scale(raw)
    assert (median, mad) == (11.0, 1.0)
    assert rq.event_level(14.0, median, mad) == 3.0 / 1.4826
    # the reference's normalisation of the same read, unclipped
    z = (raw.astype(np.float64) - np.median(raw)) / (1.4826 * np.median(np.abs(raw - np.median(raw))))
    assert rq.event_level(float(raw[3]), median, mad) == z[3]


def test_event_rows_follow_the_span_and_the_column_order():
    from radian_amd import resquiggle as rq
    raw = np.array([100, 1, 2, 3, 4, 5, 6, 100, 100], dtype=np.int16)
    first, last = [1, 3, 4], [1, 3, 6]
    ev = ref.events(raw, first, last)
    span = "AcU"                                   # 5'->3'; decode order is its reverse: label 0 is U
    rows, levels, dwells = rq.event_rows("r1", "tx", span, raw, tuple(np.array(ev[k]) for k in ("start", "end", "sum", "sumsq", "min", "max")), [7, 8, 9])
    assert rq.EVENT_COLUMNS == ("read_id", "ref_name", "ref_pos", "base", "start", "end", "n", "mean", "stdv", "min", "max", "level", "q")
    assert [r[:7] for r in rows] == [("r1", "tx", "0", "A", "4", "7", "3"), ("r1", "tx", "1", "C", "3", "4", "1"), ("r1", "tx", "2", "U", "1", "3", "2")]
    assert [r[12] for r in rows] == ["9", "8", "7"] and dwells == [3, 1, 2]
    assert [int(r[4]) for r in rows] == sorted((int(r[4]) for r in rows), reverse=True)      # the sample indices decrease
    median, mad = rq.read_scale(raw)
    assert rows[0][7:12] == ("5.0000", f"{math.sqrt(77 / 3 - 25):.4f}", "4", "6", f"{(5.0 - median) / (1.4826 * mad):.6f}")
    assert levels[0] == (5.0 - median) / (1.4826 * mad)


def test_kmer_table_on_a_toy_span(tmp_path):
    from radian_amd import resquiggle as rq
    kt = rq.KmerTable(3)
    kt.add("ACGUA", [0.5, 1.0, 2.0, 4.0, 8.0], [1, 2, 3, 4, 5])     # centres C, G, U: ACG, CGT, GTA (U = T)
    kt.add("acg", [0.0, 3.0, 0.0], [9, 6, 9])                       # ACG again
    assert kt.rows() == [("ACG", "2", "2.000000", "1.000000", "4.0000"), ("CGT", "1", "2.000000", "0.000000", "3.0000"),
                         ("GTA", "1", "4.000000", "0.000000", "4.0000")]
    kt.write(str(tmp_path / "k.tsv"))
    lines = open(str(tmp_path / "k.tsv")).read().splitlines()
    assert lines[0].split("\t") == ["kmer", "n_events", "level_mean", "level_sd", "dwell_mean"] and len(lines) == 4
    kt1 = rq.KmerTable(1)
    kt1.add("AC", [1.0, 2.0], [1, 1])
    assert [r[0] for r in kt1.rows()] == ["A", "C"]                 # k = 1: no base is skipped
    with pytest.raises(ValueError):
        rq.KmerTable(4)
    assert rq._median_of_counts({3: 2, 5: 1, 9: 1}) == 4.0 and rq._median_of_counts({}) is None


def test_reference_statuses_and_the_tsv_readers(tmp_path):
    from radian_amd import resquiggle as rq
    p = tmp_path / "read_ref.tsv"
    p.write_text("read_id\ttranscript\tspan\nr1\ttxA\tACGU\nr2\ttxB\tACNGT\nr4\ttxC\t\n")
    from radian_amd.label_build import read_ref_tsv
    refs, names = read_ref_tsv(str(p)), rq.read_ref_names(str(p))
    assert names == {"r1": "txA", "r2": "txB", "r4": "txC"} and set(refs) == set(names)
    st, codes = rq.reference_status("r1", refs)
    assert st is None and codes.tolist() == [3, 2, 1, 0]            # reversed, U = T
    assert rq.reference_status("r2", refs) == ("has-N", None)
    assert rq.reference_status("r3", refs) == ("no-reference", None)
    st, codes = rq.reference_status("r4", refs)
    assert st is None and len(codes) == 0
    assert rq.STATUSES == ("ok", "no-reference", "has-N", "no-path", "too-large", "signal")
    assert rq.SUMMARY_COLUMNS == ("read_id", "status", "n_samples", "ref_len", "score", "score_per_base", "median_dwell", "first_sample", "last_sample")


def test_run_counts_reads_that_never_reach_the_gpu(tmp_path):
    """`no-reference`, `has-N` and empty reads are decided on the host: with only such reads the device is never asked"""
    from radian_amd import resquiggle as rq
    args = types.SimpleNamespace(kmer=5, kmer_table=str(tmp_path / "k.tsv"), summary=str(tmp_path / "s.tsv"), batch_reads=2, budget_bytes=0,
                                 outlier_clip=4, chunk_len=1024, step_size=128)
    reads = [("f", "r2", np.arange(50, dtype=np.int16)), ("f", "r3", np.arange(60, dtype=np.int16)), ("f", "r1", np.zeros(0, dtype=np.int16))]
    refs = {"r1": "ACGU", "r2": "ACNGT"}
    st = rq.run(args, None, reads, refs, {"r1": "txA", "r2": "txB"}, lambda stem: pytest.fail("nothing is written"))
    assert (st["reads"], st["written"], st["has-N"], st["no-reference"], st["signal"], st["ok"]) == (3, 0, 1, 1, 1, 0)
    rows = [ln.split("\t") for ln in open(args.summary).read().splitlines()]
    assert rows[0] == list(rq.SUMMARY_COLUMNS)
    assert [r[:4] for r in rows[1:]] == [["r2", "has-N", "50", "5"], ["r3", "no-reference", "60", "0"], ["r1", "signal", "0", "4"]]
    assert open(args.kmer_table).read() == "\t".join(rq.KMER_COLUMNS) + "\n"
    text = rq.summary(st)
    assert "reads: 3 seen, 0 written" in text and "status: ok: 0; no-reference: 1; has-N: 1; no-path: 0; too-large: 0; signal: 1" in text


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_event_stats_host(tmp_path):
    """tests/asan_events.cpp: the host side of events.hip (argument check, boundary rule, the plain loop) built with AddressSanitizer + UBSan,
    on exact-size heap buffers: random valid inputs against a loop of its own, and every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_events"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_events.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 300 and int(last[2]) >= 12          # "<n> accepted <m> refused"
