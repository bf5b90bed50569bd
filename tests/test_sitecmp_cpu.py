"""No-GPU checks of the two-sample site comparison: the plain-Python restatement of the contract
(tests/_sitecmp_ref.py) by hand on a toy, every seeded case's defining condition (tests/_sitecmp_cases.py), rd_site_compare_host against
the restatement on every case and every refusal, the header's overflow bounds, the quantisation, site coordinates and refusals of
radian_amd/compare.py, its host statistics against scipy where scipy is installed, the separation of shifted sites on
radian_amd.synthetic.site_events, and the host code of sitecmp.hip under AddressSanitizer + UBSan as a stand-alone program
(tests/asan_sitecmp.cpp).  Every comparison of integers is for equality."""
import ctypes
import io
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _sitecmp_cases as sc
import _sitecmp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(got, want, where):
    for f in ref.FIELDS:
        a = getattr(got, f)
        assert a.dtype == want[f].dtype and a.shape == want[f].shape, (where, f, a.dtype, a.shape)
        assert np.array_equal(a, want[f]), (where, f)


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_by_hand_on_a_toy():
    """a = 1 3 3, b = 2 3 5 5 (n0 = 3, n1 = 4).
    moments   sum 7 / 15, sumsq 1 + 9 + 9 = 19 / 4 + 9 + 25 + 25 = 63; med2: a ranks 1, 1 -> 3 + 3 = 6; b ranks 1, 2 -> 3 + 5 = 8
    u2        x = 1: nothing of b below or equal -> 0; x = 3 (twice): 2 * #{b < 3} + #{b = 3} = 2 * 1 + 1 = 3 -> u2 = 6  (U = 3)
    ks        x = 1: |1 * 4 - 0 * 3| = 4; x = 2: |1 * 4 - 1 * 3| = 1; x = 3: |3 * 4 - 2 * 3| = 6; x = 5: |3 * 4 - 4 * 3| = 0 -> 6 at x = 3
    tie       multiplicities 1 (x = 1), 1 (2), 3 (3), 2 (5): 0 + 0 + (27 - 3) + (8 - 2) = 30"""
    e = ref.site_entry(4, [3, 1, 3], [5, 2, 5, 3])
    assert e == dict(out_site=4, status=ref.OK, n=(3, 4), sum=(7, 15), sumsq=(19, 63), vmin=(1, 2), vmax=(3, 5), med2=(6, 8), u2=6, ks_num=6, ks_x=3,
                     tie=30)
    # one-sided: the absent sample's fields and the rank fields are 0
    assert ref.site_entry(0, [], [4, 2]) == dict(out_site=0, status=ref.ONE_SIDED, n=(0, 2), sum=(0, 6), sumsq=(0, 20), vmin=(0, 2), vmax=(0, 4),
                                                 med2=(0, 6), u2=0, ks_num=0, ks_x=0, tie=0)
    # the events in any order, two sites
    got = ref.compare([9, 4, 4, 9, 4], [1, 0, 1, 0, 0], [7, -7, 0, 7, 2])
    assert [g["out_site"] for g in got] == [4, 9] and got[0]["n"] == (2, 1) and got[1]["tie"] == 6 and got[0]["u2"] == 2
    keys, segs = ref.segments([9, 4, 4, 9, 4], [1, 0, 1, 0, 0], [7, -7, 0, 7, 2])
    assert segs == [(4, 0, 2, 3), (9, 3, 4, 5)] and keys[0] == 4 * 131072 + 32761 and keys[4] == 9 * 131072 + 65536 + 32775
    # the numpy form of the deep case is the same definition
    rng = np.random.default_rng(5)
    s, c, v = rng.integers(0, 4, 500), rng.integers(0, 2, 500), rng.integers(-6, 6, 500)
    assert ref.compare_deep(s, c, v) == ref.compare(s, c, v)


def test_every_case_meets_its_defining_condition():
    groups = sc.all_groups() + [sc.deep_group()]
    names = [g["name"] for g in groups]
    assert len(set(names)) == len(names) == 10
    n_cond = 0
    for g in groups:
        by = {e["out_site"]: e for e in sc.reference(g["name"])}
        assert sorted(by) == sorted(set(g["site"].tolist()))
        for s, pred in g["cond_of"].items():
            assert pred(by[s]), (g["name"], s, by[s])
            n_cond += 1
    assert n_cond == 37
    depths = {sum(e["n"]) for e in sc.reference("depths") if e["out_site"] < 100}
    assert depths == set(sc.DEPTHS) == {1, 2, 63, 64, 65, sc.C - 1, sc.C, sc.C + 1, 3 * sc.C + 5} and len(depths) == 9
    g = next(g for g in groups if g["name"] == "interleaved")
    assert (g["site"][1:] != g["site"][:-1]).all()                     # no site is contiguous in the input
    g = next(g for g in groups if g["name"] == "wide_sites")
    assert g["n_sites"] == 2 ** 32 - 1 and {0, 2 ** 32 - 2} <= set(g["site"].tolist())


# ---------------------------------------------------------------------------------------------- the host entry point
def test_site_compare_host_equals_the_restatement():
    from radian_amd.backend import SITE_FIELDS, site_compare_host
    assert SITE_FIELDS == ref.FIELDS
    for g in sc.all_groups() + [sc.deep_group()]:
        want = ref.as_arrays(sc.reference(g["name"]))
        _equal(site_compare_host(g["site"], g["cond"], g["value"], g["n_sites"]), want, g["name"])
        if g["name"] != "deep":
            _equal(site_compare_host(g["site"][::-1], g["cond"][::-1], g["value"][::-1], g["n_sites"]), want, g["name"] + " reversed")
            _equal(site_compare_host(g["site"], g["cond"], g["value"], g["n_sites"], capacity=len(want["status"]) + 3), want, g["name"] + " roomy")
    empty = site_compare_host(np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int16), 5)
    assert len(empty.status) == 0


def test_every_refusal_of_the_host_entry_point():
    from radian_amd import _lib
    from radian_amd.backend import RadianHipError, SiteResult, _p, site_compare_host, site_workspace_bytes
    site, cond, value = np.array([0, 1, 1], np.uint32), np.array([0, 1, 0], np.uint8), np.array([5, 6, 7], np.int16)
    L = _lib.load()

    def call(s, c, v, n_events, n_sites, cap, null_out=None):
        res, n_out = SiteResult(2), ctypes.c_int64(-9)
        bufs = res._bufs()
        if null_out is not None:
            bufs[null_out] = None
        rc = L.rd_site_compare_host(s, c, v, n_events, n_sites, cap, *bufs, ctypes.byref(n_out))
        untouched = n_out.value == -9 and all((getattr(res, f) == 0).all() for f in ref.FIELDS)
        return rc, untouched, L.rd_last_error().decode()

    assert call(_p(site), _p(cond), _p(value), 3, 2, 2)[0] == 0
    for args, word in (((None, _p(cond), _p(value), 3, 2, 2), "null"), ((_p(site), None, _p(value), 3, 2, 2), "null"),
                       ((_p(site), _p(cond), None, 3, 2, 2), "null"), ((_p(site), _p(cond), _p(value), 2 ** 31, 2, 2), "2^31 - 1"),
                       ((_p(site), _p(cond), _p(value), 3, 1, 2), "site 1"), ((_p(site), _p(cond), _p(value), 3, 2, 1), "2 distinct sites")):
        rc, untouched, msg = call(*args)
        assert rc == -1 and untouched and word in msg, (args[3:], msg)
    for k in range(12):
        assert call(_p(site), _p(cond), _p(value), 3, 2, 2, null_out=k)[0] == -1
    bad = cond.copy()
    bad[2] = 2
    rc, untouched, msg = call(_p(site), _p(bad), _p(value), 3, 2, 2)
    assert rc == -1 and untouched and "event 2 has cond 2" in msg
    with pytest.raises(RadianHipError):
        site_compare_host(site, bad, value, 2)
    with pytest.raises(ValueError):
        site_compare_host(site, cond[:2], value, 2)
    assert site_workspace_bytes(10) == 1600 and site_workspace_bytes(0) == 0 and site_workspace_bytes(-1) == -1 and site_workspace_bytes(2 ** 31) == -1


def test_the_headers_bounds_are_arithmetic():
    """include/radian_hip.h: with |v| <= 2^15 and N = n0 + n1 <= 2^20 no field overflows int64 and the packed maximum stays below 2^55"""
    N, V = 1 << 20, 1 << 15
    assert (2 ** 31 - 1) * V * V < 1 << 61                                   # sumsq, for any n_events the call takes
    assert (2 ** 31 - 1) * V < 1 << 63                                       # sum
    assert N ** 3 - N <= 1 << 60                                             # tie: every value equal
    assert 2 * (N // 2) * (N // 2) <= 1 << 39                                # u2 <= 2 n0 n1
    assert (N // 2) * (N // 2) <= 1 << 38                                    # ks_num <= n0 n1
    assert ((N // 2) ** 2 << 16 | 65535) < 1 << 55                           # the word the kernels take the maximum of
    assert 2 * V - 1 <= 65535 and (2 ** 32 - 2) << 17 | 0x1ffff < 1 << 49    # the key: 16 value bits, 1 cond bit, 32 site bits
    hdr = open(os.path.join(ROOT, "include", "radian_hip.h")).read()
    for word in ("sumsq < 2^61", "tie <= 2^60", "u2 <= 2^39", "ks_num <= 2^38", "below 2^55"):
        assert word in hdr, word
    # the all-equal case reaches the tie bound's form
    e = {e["out_site"]: e for e in sc.reference("all_equal")}[0]
    assert e["tie"] == 130 ** 3 - 130


# ---------------------------------------------------------------------------------------------- the command's host side
def test_quantisation():
    from radian_amd.compare import quantise_dwell, quantise_level
    lv = quantise_level([0.0, 1.0, -1.0, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, 31.9999, 32.0, 40.0, -32.0, -33.0, 0.00048])
    assert lv.dtype == np.int16 and lv.tolist() == [0, 1024, -1024, 0, 2, 2, 32767, 32767, 32767, -32768, -32768, 0]   # rint: half to even
    dw = quantise_dwell([1, 12, 32767, 32768, 100000])
    assert dw.dtype == np.int16 and dw.tolist() == [1, 12, 32767, 32767, 32767]


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


PAF_A = ("r1\t50\t0\t50\t+\ttB\t100\t10\t60\t40\t50\t255\n"
         "r2\t30\t0\t30\t+\ttA\t40\t5\t35\t25\t30\t255\ts1:i:3\n")
PAF_B = "r9\t30\t0\t30\t+\ttA\t40\t0\t30\t25\t30\t255\n"
HEADER = "read_id\tref_name\tref_pos\tbase\tstart\tend\tn\tmean\tstdv\tmin\tmax\tlevel\tq\n"


def _row(rid, ref, pos, base, n, level, q):
    return f"{rid}\t{ref}\t{pos}\t{base}\t0\t{n}\t{n}\t0.0\t0.0\t0\t0\t{level}\t{q}\n"


def test_site_coordinates_from_a_hand_written_paf(tmp_path):
    """transcripts sorted by name: tA (40 bases) takes sites 0..39, tB (100) 40..139.  r1 spans tB from 10: its ref_pos 3 is tB position 13,
    site 53; r2 spans tA from 5: ref_pos 0 is site 5; r9 (sample B) spans tA from 0: ref_pos 5 is site 5 as well"""
    from radian_amd import compare
    pa, pb = compare.read_paf(_write(tmp_path / "a.paf", PAF_A)), compare.read_paf(_write(tmp_path / "b.paf", PAF_B))
    assert pa == {"r1": ("tB", 100, 10), "r2": ("tA", 40, 5)} and pb == {"r9": ("tA", 40, 0)}
    names, offsets, n_sites = compare.transcript_offsets([pa, pb])
    assert names == ["tA", "tB"] and offsets == {"tA": (0, 40), "tB": (40, 100)} and n_sites == 140
    ev = _write(tmp_path / "x.events.tsv", HEADER + _row("r1", "tB", 3, "G", 9, 0.5, 20) + _row("r2", "tA", 0, "C", 40000, -1.25, 3)
                + _row("rX", "tB", 0, "A", 5, 0.1, 20) + _row("rX", "tB", 1, "A", 5, 0.1, 20) + _row("r1", "tB", 4, "T", 7, "nan", 20))
    bases = {}
    st = {"files": 0, "events": 0, "kept": 0, "reads-no-mapping": 0, "no-mapping": 0, "low-q": 0, "bad-level": 0}
    site, level, dwell = compare.load_events([ev], pa, offsets, 5, bases, st)
    assert site.dtype == np.uint32 and site.tolist() == [53] and level.tolist() == [512] and dwell.tolist() == [9]
    assert st == {"files": 1, "events": 5, "kept": 1, "reads-no-mapping": 1, "no-mapping": 2, "low-q": 1, "bad-level": 1}
    assert bases == {53: "G", 5: "C", 54: "T"}
    st2 = dict(st, files=0, events=0, kept=0)
    evb = _write(tmp_path / "y.events.tsv", HEADER + _row("r9", "tA", 5, "C", 3, 0.25, 9))
    assert compare.load_events([evb], pb, offsets, 0, bases, st2)[0].tolist() == [5]


def test_every_refusal_of_the_commands_parser(tmp_path, monkeypatch):
    from radian_amd import compare
    pa = compare.read_paf(_write(tmp_path / "a.paf", PAF_A))
    offsets = compare.transcript_offsets([pa])[1]

    def load(rows, paf=pa, bases=None):
        st = {"files": 0, "events": 0, "kept": 0, "reads-no-mapping": 0, "no-mapping": 0, "low-q": 0, "bad-level": 0}
        return compare.load_events([_write(tmp_path / "e.events.tsv", HEADER + rows)], paf, offsets, 0, {} if bases is None else bases, st)

    with pytest.raises(SystemExit, match="transcript tA has two different lengths"):
        compare.transcript_offsets([pa, compare.read_paf(_write(tmp_path / "c.paf", PAF_B.replace("\t40\t", "\t41\t")))])
    with pytest.raises(SystemExit, match="read r1 is on tA here and on tB in the PAF"):
        load(_row("r1", "tA", 3, "G", 9, 0.5, 20))
    with pytest.raises(SystemExit, match="tB position 13 is A here and G elsewhere"):
        load(_row("r1", "tB", 3, "G", 9, 0.5, 20) + _row("r1", "tB", 3, "A", 9, 0.5, 20))
    with pytest.raises(SystemExit, match="position 100 is outside tB"):
        load(_row("r1", "tB", 90, "G", 9, 0.5, 20))
    with pytest.raises(SystemExit, match="header lacks"):
        compare.load_events([_write(tmp_path / "h.events.tsv", "read_id\tref_name\n")], pa, offsets, 0, {}, {"files": 0})
    with pytest.raises(SystemExit, match="fewer than 9 PAF columns"):
        compare.read_paf(_write(tmp_path / "d.paf", "r1\t50\t0\n"))
    with pytest.raises(SystemExit, match="outside the transcript's length"):
        compare.read_paf(_write(tmp_path / "d.paf", PAF_B.replace("\t40\t0\t", "\t40\t40\t")))
    # more events than one call takes: the limit is a module constant, lowered here
    os.makedirs(tmp_path / "A"), os.makedirs(tmp_path / "B")
    _write(tmp_path / "A" / "x.events.tsv", HEADER + _row("r1", "tB", 3, "G", 9, 0.5, 20) + _row("r1", "tB", 4, "G", 9, 0.5, 20))
    _write(tmp_path / "B" / "y.events.tsv", HEADER + _row("r9", "tA", 5, "C", 3, 0.25, 9))
    args = compare.build_parser().parse_args(["--a", str(tmp_path / "A"), "--a-paf", str(tmp_path / "a.paf"), "--b", str(tmp_path / "B"), "--b-paf",
                                              _write(tmp_path / "b.paf", PAF_B), "-o", str(tmp_path / "o.tsv")])
    compare.check_args(args)
    assert len(compare.load(args)[4]) == 3
    monkeypatch.setattr(compare, "MAX_EVENTS", 2)
    with pytest.raises(SystemExit, match="3 events in all, more than 2\\^31 - 1"):
        compare.load(args)
    for bad in (["--min-depth", "0"], ["--min-q", "-1"], ["--alpha", "0"], ["--alpha", "1.5"], ["--budget-bytes", "-1"], ["--a", str(tmp_path / "nope")],
                ["--b-paf", str(tmp_path / "nope.paf")]):
        base = ["--a", str(tmp_path / "A"), "--a-paf", str(tmp_path / "a.paf"), "--b", str(tmp_path / "B"), "--b-paf", str(tmp_path / "b.paf"), "-o", "o"]
        with pytest.raises(SystemExit):
            compare.check_args(compare.build_parser().parse_args(base + bad))


def test_the_site_limit_is_2_to_the_32_minus_1(tmp_path):
    from radian_amd import compare
    assert compare.MAX_SITES == 2 ** 32 - 1 and compare.MAX_EVENTS == 2 ** 31 - 1
    ok = "r0\t5\t0\t5\t+\tt0\t{}\t0\t5\t5\t5\t255\nr1\t5\t0\t5\t+\tt1\t{}\t0\t5\t5\t5\t255\n"
    assert compare.transcript_offsets([compare.read_paf(_write(tmp_path / "g.paf", ok.format(2 ** 31, 2 ** 31 - 1)))])[2] == 2 ** 32 - 1
    with pytest.raises(SystemExit, match="4294967296 sites in all, more than 2\\^32 - 1"):
        compare.transcript_offsets([compare.read_paf(_write(tmp_path / "g.paf", ok.format(2 ** 31, 2 ** 31)))])


def test_host_statistics_by_hand():
    """the toy of the first test: n0 = 3, n1 = 4, u2 = 6, ks_num = 6, tie = 30.
    ks_d = 6 / 12 = 0.5, lambda = 0.5 sqrt(12 / 7); U = 3, mu = 6, N = 7, var = 12 / 12 (8 - 30 / 42) = 7.2857..., z = (3 - 6 + 0.5) / sqrt(var)"""
    from radian_amd import compare
    d, p = compare.ks_test(6, 3, 4)
    assert d == 0.5 and p == compare.kolmogorov_tail(0.5 * math.sqrt(12 / 7))
    z, p = compare.mwu_test(6, 30, 3, 4)
    assert z == pytest.approx(-2.5 / math.sqrt(8 - 30 / 42), rel=1e-15) and p == pytest.approx(math.erfc(abs(z) / math.sqrt(2)), rel=1e-15)
    assert compare.mwu_test(12, 30, 3, 4) == (0.0, 1.0) and compare.mwu_test(40 * 90, 130 ** 3 - 130, 40, 90) == (0.0, 1.0)
    assert compare.sample_moments(3, 7, 19, 6, 1.0) == (7 / 3, math.sqrt((3 * 19 - 49) / 6), 3.0)
    assert compare.sample_moments(1, 1024, 1024 * 1024, 2048, 1024.0)[::2] == (1.0, 1.0) and math.isnan(compare.sample_moments(1, 5, 25, 10, 1.0)[1])
    assert all(math.isnan(v) for v in compare.sample_moments(0, 0, 0, 0, 1.0))
    assert compare.kolmogorov_tail(0.0) == 1.0 and compare.kolmogorov_tail(1e-3) == 1.0 and compare.kolmogorov_tail(40.0) == 0.0
    # Benjamini-Hochberg: p = .01 .04 .03 .04 (m = 4): ranks 1 3 2 4 (the tie by position) -> .04 .04 .04 .04; and a monotone example
    assert compare.benjamini_hochberg([0.01, 0.04, 0.03, 0.04]) == [0.04, 0.04, 0.04, 0.04]
    assert compare.benjamini_hochberg([0.001, 0.5, 0.01]) == pytest.approx([0.003, 0.5, 0.015]) and compare.benjamini_hochberg([]) == []
    assert [compare.row_status(*a) for a in ((0, 10, 10, 10), (0, 9, 10, 10), (1, 0, 50, 10), (2, 600000, 600000, 10), (3, 50, 50, 10), (2, 5, 2 ** 21, 10))] \
        == ["ok", "low-depth", "one-sided", "deep", "too-large", "low-depth"]


def test_host_statistics_against_scipy():
    """U and D of the integers are scipy's statistics; mwu_p and the Kolmogorov tail agree with scipy to 1e-12 relative for p > 1e-300
    (measured: 7e-15 and 9e-15; the margin covers another libm)"""
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    from radian_amd import compare
    worst_p = worst_q = 0.0
    n = 0
    for g in sc.all_groups():
        groups = ref.by_site(g["site"], g["cond"], g["value"])
        for e in sc.reference(g["name"]):
            if e["status"] != ref.OK:
                continue
            a, b = groups[e["out_site"]]
            n0, n1 = e["n"]
            mw = stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided", method="asymptotic")
            assert mw.statistic == e["u2"] / 2
            ks = stats.ks_2samp(a, b, method="asymp")
            assert round(ks.statistic * n0 * n1) == e["ks_num"] and abs(ks.statistic - e["ks_num"] / (n0 * n1)) <= 4 * np.finfo(float).eps
            z, p = compare.mwu_test(e["u2"], e["tie"], n0, n1)
            if e["tie"] < (n0 + n1) ** 3 - (n0 + n1) and mw.pvalue > 1e-300:
                worst_p = max(worst_p, abs(p - mw.pvalue) / mw.pvalue)
                n += 1
    for lam in [0.05 * k for k in range(1, 400)]:
        want = float(special.kolmogorov(lam))
        if want > 1e-300:
            worst_q = max(worst_q, abs(compare.kolmogorov_tail(lam) - want) / want)
    print(f"mwu_p worst relative difference {worst_p:.2e} over {n} sites; Kolmogorov tail {worst_q:.2e}")
    assert n >= 25 and worst_p <= 1e-12 and worst_q <= 1e-12


def test_separation_on_synthetic_site_events():
    """synthetic.site_events, seed 11: 300 sites at depth >= 100, every tenth site's level moved by 0.5 z in sample 1.  Through the
    restatement's integers and the command's formulas (q over mwu_p): observed here 30 of 30 shifted sites with level q <= 0.05 and 3 of
    270 unshifted ones (the bound allows 13)."""
    from radian_amd import compare, synthetic
    shifted = set(range(0, 300, 10))
    ev = synthetic.site_events(np.random.default_rng(11), n_sites=300, median_depth=110.0, sigma=0.3, min_depth=100, shifted=shifted)
    assert ev["depth"].min() >= 100 and ev["depth"].max() > 150
    entries = ref.compare(ev["site"], ev["cond"], compare.quantise_level(ev["level"]))
    assert len(entries) == 300 and all(e["status"] == ref.OK for e in entries)
    q = compare.benjamini_hochberg([compare.mwu_test(e["u2"], e["tie"], *e["n"])[1] for e in entries])
    hit = {e["out_site"] for e, v in zip(entries, q) if v <= 0.05}
    print(f"shifted sites found {len(hit & shifted)} of {len(shifted)}; unshifted sites called {len(hit - shifted)} of {300 - len(shifted)}")
    assert shifted <= hit
    assert len(hit - shifted) <= 0.05 * (300 - len(shifted))
    # the dwell channel sees the stretch at most of those sites, and sample 1's mean dwell is longer there
    dw = ref.compare(ev["site"], ev["cond"], compare.quantise_dwell(ev["dwell"]))
    assert sum(e["sum"][1] * e["n"][0] > e["sum"][0] * e["n"][1] for e in dw if e["out_site"] in shifted) >= 28


def test_write_table_on_the_toy():
    """two transcripts, three sites: an ok site, a low-depth site and a one-sided site; only the ok row carries test columns"""
    from radian_amd import compare
    rng = np.random.default_rng(3)
    site = np.array([2] * 30 + [41] * 6 + [45] * 4)
    cond = np.array([0] * 15 + [1] * 15 + [0, 0, 0, 1, 1, 1] + [1] * 4)
    value = rng.integers(-50, 50, 40)
    res = types.SimpleNamespace(**ref.as_arrays(ref.compare(site, cond, value)))
    buf = io.StringIO()
    st = compare.write_table(buf, ["tA", "tB"], {"tA": (0, 40), "tB": (40, 100)}, {2: "A", 41: "C", 45: "G"}, {"dwell": res}, 10, 0.05)
    rows = [ln.split("\t") for ln in buf.getvalue().splitlines()]
    assert rows[0] == ["ref_name", "pos", "base", "status", "n_a", "n_b"] + ["dwell_" + c for c in compare.STAT_COLUMNS]
    assert [r[:6] for r in rows[1:]] == [["tA", "2", "A", "ok", "15", "15"], ["tB", "1", "C", "low-depth", "3", "3"], ["tB", "5", "G", "one-sided", "0", "4"]]
    assert "nan" not in rows[1] and rows[2][12:] == ["nan"] * 5 and rows[2][6] != "nan" and rows[3][6] == "nan" and rows[3][7] != "nan"
    assert rows[1][16] == rows[1][15]                                   # one tested site: q == mwu_p
    assert (st["ok"], st["low-depth"], st["one-sided"], st["deep"], st["too-large"]) == (1, 1, 1, 0, 0)
    text = compare.summary({k: {"files": 1, "events": 9, "kept": 8, "reads-no-mapping": 1, "no-mapping": 1, "low-q": 0, "bad-level": 0} for k in "ab"}, st,
                           ["dwell"], 0.05)
    assert "sample A: 1 files, 9 events read, 8 kept" in text and "sites: ok: 1; low-depth: 1; one-sided: 1; deep: 0; too-large: 0" in text
    assert "dropped: no-mapping: 1; low-q: 0; bad-level: 0 (1 reads absent from the PAF)" in text and "dwell: " in text


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_site_compare_host(tmp_path):
    """tests/asan_sitecmp.cpp: the host side of sitecmp.hip (argument check, the rules, the counting pass, plan and buckets, the host twin)
    built with AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap buffers of the cases' shapes; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_sitecmp"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_sitecmp.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 400 and int(last[2]) >= 1600          # "<n> accepted <m> refused"
