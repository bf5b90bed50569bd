"""No-GPU checks of the poly(A) tail estimation: the plain-Python restatement of the contract (tests/_polya_ref.py)
by hand on a toy, every seeded case's defining condition (tests/_polya_cases.py), rd_polya_segment_host against the restatement on every
case and every refusal, the synthetic tails (radian_amd.synthetic.tail_read), the host formulas and the moves-based rate of
radian_amd/polya.py, and the host code of polya.hip under AddressSanitizer + UBSan as a stand-alone program (tests/asan_polya.cpp).
Every comparison of integers is for equality."""
import io
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _polya_cases as pc
import _polya_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def groups():
    return pc.all_groups()


def _params(p):
    from radian_amd.backend import PolyaParams
    return PolyaParams(**p)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_on_a_three_window_toy():
    """win 8; window 0 alternates 0 / 40, window 1 is constant 10, window 2 is 10 but for one 11; two samples are left over.
    sorted: 4 x 0, 16 x 10 (ranks 4..19), 11, 4 x 40, and the tail's 10, 10 -> 26 samples, ranks 12 and 13 are 10: m2 = 20.
    |2x - 20|: 17 x 0 (the 10s), 2 (the 11), 4 x 20 (the 0s), 4 x 60 (the 40s): ranks 12, 13 are 0 -> d4 = 0: MAD_ZERO."""
    x = [0, 40] * 4 + [10] * 8 + [10] * 7 + [11] + [10, 10]
    p = ref.params(win=8, flat_q=256, max_gap=0, min_samples=8)
    assert ref.scale(x) == (20, 0)
    assert ref.segment(x, p) == dict(status=ref.MAD_ZERO, tail_start=-1, tail_end=-1, n_flat=0, sum=0, sumsq=0, m2=20, d4=0, n_candidates=0)
    # spread the levels so that the MAD is not zero: window 0 alternates 0 / 40, window 1 is constant 10, window 2 is 12 .. 19
    x = [0, 40] * 4 + [10] * 8 + list(range(12, 20)) + [5]
    # sorted: 0 0 0 0 5 10 x8 12 13 14 15 16 17 18 19 40 40 40 40 (25 samples): rank 12 is 10 -> m2 = 20
    # |2x - 20|: 20 x4, 10, 0 x8, 4 6 8 10 12 14 16 18, 60 x4 -> sorted 0 x8 4 6 8 10 10 12 ...: rank 12 is 10 -> d4 = 20
    assert ref.scale(x) == (20, 20)
    # flat_q = 256 (sd <= MAD = 5): A = 8 * 256 * 20 = 40960, thr = 40960^2 >> 20 = 1600 = (8 * 5)^2
    assert ref.threshold(8, 256, 20) == 1600
    m2, d4, thr, wins = ref.windows(x, p)
    # window 0: S = 160, Q = 6400, V = 8 * 6400 - 160^2 = 25600 (sd 20); window 1: V = 0; window 2: S = 124, Q = 1964, V = 15712 - 15376 = 336
    assert wins == [(160, 6400, 0), (80, 800, 1), (124, 1964, 1)]
    out = ref.segment(x, p)
    assert out == dict(status=ref.OK, tail_start=8, tail_end=24, n_flat=2, sum=204, sumsq=2764, m2=20, d4=20, n_candidates=1)
    # the level band in units of MAD / 256: window 1 sits at the median (0), window 2 at mean 15.5: 512 (2 * 124 - 160) = 45056 = 281.6 * 160
    lvl = dict(p, use_level=1, lo_q=-10, hi_q=281)
    assert [w[2] for w in ref.windows(x, lvl)[3]] == [0, 1, 0]
    assert [w[2] for w in ref.windows(x, dict(lvl, hi_q=282))[3]] == [0, 1, 1]
    assert ref.segment(x, dict(lvl, min_samples=16))["status"] == ref.NONE
    assert ref.segments_of([1, 0, 0, 1, 1, 0, 1], 1) == [(0, 0, 1), (3, 6, 3)] and ref.segments_of([1, 0, 0, 1], 2) == [(0, 3, 2)]


def test_the_threshold_cannot_saturate_through_the_abi():
    """A = win flat_q d4 <= 256 * 32767 * 262142 < 2^41 (d4 is the sum of two values of |2x - m2| <= 131071), so A^2 < 2^82: the case
    "A^2 >= 2^84" does not exist for a read.  The rule's saturation is checked where it can be reached: tests/asan_polya.cpp calls it."""
    A = 256 * 32767 * 2 * 131071
    assert A < 1 << 41 and A * A >> 20 < 1 << 64
    assert ref.threshold(256, 32767, 2 * 131071) == A * A >> 20


def test_every_case_meets_its_defining_condition(groups):
    names = [g["name"] for g in groups]
    assert len(set(names)) == len(names) >= 13
    n_cond = 0
    for g in groups:
        for r, x in enumerate(g["reads"]):
            wins = ref.windows(x, g["p"])[3] if len(x) else []
            if g["flags"][r] is not None:
                assert [w[2] for w in wins] == g["flags"][r], (g["name"], r)
            if r in g["cond"]:
                assert g["cond"][r](ref.segment(x, g["p"]), wins), (g["name"], r)
                n_cond += 1
    assert n_cond >= 28
    shapes = groups[0]
    assert sorted(len(x) // 8 for x in shapes["reads"])[-1] == 5003 and {63, 64, 65, 255, 256, 257} <= {len(x) // 8 for x in shapes["reads"]}
    assert {0, 7, 8, 15} <= {len(x) for x in shapes["reads"]}


# ---------------------------------------------------------------------------------------------- the host entry point
def test_polya_segment_host_equals_the_restatement(groups):
    from radian_amd.backend import polya_segment_host
    for g in groups:
        got = polya_segment_host(g["reads"], _params(g["p"]))
        exp = [ref.segment(x, g["p"]) for x in g["reads"]]
        for r in range(len(exp)):
            pc.same(got, r, exp[r])
        n = len(exp)
        rev = polya_segment_host(g["reads"][::-1], _params(g["p"]))
        for r in range(n):
            pc.same(rev, n - 1 - r, exp[r])
            pc.same(polya_segment_host([g["reads"][r]], _params(g["p"])), 0, exp[r])


def test_polya_segment_host_refuses_bad_arguments():
    from radian_amd import _lib
    L = _lib.load()
    good, bad = pc.refusal_cases()
    assert pc.raw_call(L.rd_polya_segment_host, **good) == 0
    for name, kw in bad:
        outs = [np.full(2, 77, dtype=np.int64 if f in ("tail_start", "tail_end", "sum", "sumsq") else np.int32) for f in ref.FIELDS]
        assert pc.raw_call(L.rd_polya_segment_host, outs=outs, **kw) == -1, name   # RD_ERR_ARG
        assert all((o == 77).all() for o in outs), name
    assert pc.raw_call(L.rd_polya_segment_host, raw=None, off=None, p=good["p"], n_reads=0) == 0    # n_reads == 0 is RD_OK
    assert L.rd_polya_workspace_bytes(4096, 32) == 2 * 4096 + 14 * 128 + 2048 and L.rd_polya_workspace_bytes(10, 7) == -1


# ---------------------------------------------------------------------------------------------- synthetic tails
def test_tail_read_tails_are_found_within_a_window():
    """The bound is the window grid's: every window that is wholly outside the tail is non-flat and every window wholly inside it is flat
    (asserted), so the first flat window is the one that straddles the tail's start or the first one inside it -- it starts less than win
    samples from the truth on either side; the same at the end."""
    from radian_amd import synthetic
    from radian_amd.backend import PolyaParams, polya_segment_host
    p = PolyaParams()     # the command's defaults
    assert p.args() == (32, 46, 0, 0, 0, 2, 480, 0)
    pd = dict(zip(ref.PARAMS, p.args()))
    shapes = [dict(), dict(leader=0, adapter=37, tail=481 + 62, body=900), dict(leader=333, adapter=515, tail=3001, body=2500, tail_level=540.0)]
    for seed, kw in enumerate(shapes):
        x, (a, e) = synthetic.tail_read(np.random.default_rng(40 + seed), **kw)
        assert x.dtype == np.int16 and len(x) == sum(kw.get(k, d) for k, d in (("leader", 400), ("adapter", 600), ("tail", 1500), ("body", 4000)))
        wins = ref.windows(x, pd)[3]
        inside = [j for j in range(len(wins)) if j * 32 >= a and (j + 1) * 32 <= e]
        outside = [j for j in range(len(wins)) if (j + 1) * 32 <= a or j * 32 >= e]
        assert len(inside) >= 15 and all(wins[j][2] for j in inside) and not any(wins[j][2] for j in outside)
        out = ref.segment(x, pd)
        assert out["status"] == ref.OK and out["n_candidates"] == 1
        assert abs(out["tail_start"] - a) < 32 and abs(out["tail_end"] - e) < 32
        pc.same(polya_segment_host([x], p), 0, out)


# ---------------------------------------------------------------------------------------------- the command's host side
def test_host_formulas_and_moves_rate_on_a_toy(tmp_path):
    from radian_amd import polya
    from radian_amd.backend import polya_q
    assert polya_q(0.12) == 46 and polya_q(1.0) == 380 and polya_q(-2.0) == -759
    # a segment of 4 samples 10, 12, 10, 12: mean 11, sd 1; median 8 (m2 = 16), MAD 2 (d4 = 8): level = 3 / 2.9652, spread = 1 / 2.9652
    level, spread = polya.segment_level(4, 44, 488, 16, 8)
    assert level == (11.0 - 8.0) / (1.4826 * 2.0) and spread == 1.0 / (1.4826 * 2.0)
    # the rate: bases whose first sample is >= tail_end, written 5' -> 3' (the positions decrease)
    first = [190, 170, 150, 130, 110, 90, 70, 50, 30, 10]
    last = [199, 180, 160, 140, 120, 100, 80, 60, 40, 20]
    assert polya.moves_rate(first, last, 50) == (200 - 50) / 8            # 8 bases start at or after sample 50
    assert math.isnan(polya.moves_rate(first, last, 51))                   # 7 bases: below the minimum of 8
    assert polya.moves_rate(first, last, 0) == 200 / 10
    assert math.isnan(polya.moves_rate([-1] * 12, [-1] * 12, 0))           # a read without a path
    mv = tmp_path / "moves.tsv"
    mv.write_text("read_id\tn_samples\tfirst_step\tlast_step\n" + "ra\t200\t" + ",".join(map(str, first)) + "\t" + ",".join(map(str, last)) + "\nrb\t5\t\t\n")
    moves = polya.read_moves(str(mv))
    assert sorted(moves) == ["ra", "rb"] and moves["ra"][0].tolist() == first and moves["rb"][1].tolist() == []

    # run() on a stub backend: the rows, the nan rules and the counters
    class Stub:
        def polya_segment(self, raws, p, budget_bytes=0, allow_too_large=False):
            from radian_amd.backend import polya_segment_host
            return polya_segment_host(raws, p)

    args = polya.build_parser().parse_args(["x", "-o", "y", "--window", "8", "--min-samples", "16", "--max-gap", "0", "--batch-reads", "2"])
    polya.check_args(args)
    rng = np.random.default_rng(3)
    tail = pc.read_from_flags([0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], 8, rng)            # tail = samples [16, 48)
    reads = [("f", "ra", tail), ("f", "rz", np.zeros(0, np.int16)), ("f", "rc", tail), ("f", "rb", np.full(20, 3, np.int16))]
    big = (np.array(first) + 48, np.array(last) + 48)
    buf = io.StringIO()
    st = polya.run(args, Stub(), reads, buf, {"ra": big, "rb": moves["rb"]})
    rows = [ln.split("\t") for ln in buf.getvalue().splitlines()]
    assert rows[0] == list(polya.COLUMNS)
    exp = ref.segment(tail, dict(zip(ref.PARAMS, polya.params_of(args).args())))
    level, spread = polya.segment_level(32, exp["sum"], exp["sumsq"], exp["m2"], exp["d4"])
    assert rows[1] == ["ra", "ok", "96", "16", "48", "32", f"{level:.6f}", f"{spread:.6f}", "20.0000", "1.60", "1"]
    assert rows[2] == ["rz", "empty", "0", "-1", "-1", "0", "nan", "nan", "nan", "nan", "0"]
    assert rows[3][:6] == ["rc", "ok", "96", "16", "48", "32"] and rows[3][8:] == ["nan", "nan", "1"]         # missing from the moves file
    assert rows[4][:3] == ["rb", "mad-zero", "20"]
    assert (st["reads"], st["ok"], st["empty"], st["mad-zero"], st["no-moves"], st["tail_samples"], st["tail_nt"]) == (4, 2, 1, 1, 1, [32, 32], [1.6])
    text = polya.summary(st)
    assert "reads: 4 seen" in text and "ok: 2; none: 0; mad-zero: 1; short: 0; empty: 1; too-large: 0" in text
    assert "median tail_samples: 32.0" in text and "median tail_nt: 1.60" in text and "missing from the moves file: 1" in text
    # a fixed rate, and neither option
    args.samples_per_base = 8.0
    buf = io.StringIO()
    polya.run(args, Stub(), reads[:1], buf, None)
    assert buf.getvalue().splitlines()[1].split("\t")[8:10] == ["8.0000", "4.00"]
    args.samples_per_base = None
    buf = io.StringIO()
    polya.run(args, Stub(), reads[:1], buf, None)
    assert buf.getvalue().splitlines()[1].split("\t")[8:10] == ["nan", "nan"]
    for bad in (["--window", "7"], ["--flat-sd", "0"], ["--max-gap", "1025"], ["--min-samples", "4"], ["--level-lo", "2", "--level-hi", "1"]):
        with pytest.raises(SystemExit):
            polya.check_args(polya.build_parser().parse_args(["x", "-o", "y"] + bad))
    lv = polya.params_of(polya.build_parser().parse_args(["x", "-o", "y", "--level-lo", "-1", "--level-hi", "1.5"]))
    assert (lv.use_level, lv.lo_q, lv.hi_q) == (1, -380, 569)


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_polya_segment_host(tmp_path):
    """tests/asan_polya.cpp: the host side of polya.hip (argument check, the rules, the plain loop) built with AddressSanitizer + UBSan as a
    stand-alone executable, on exact-size heap buffers of the cases' shapes; the threshold rule up to its saturation; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_polya"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_polya.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 200 and int(last[2]) >= 17          # "<n> accepted <m> refused"
