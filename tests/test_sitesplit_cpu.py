"""No-GPU checks of the exact two-cluster split: the plain-Python restatement of the contract
(tests/_sitesplit_ref.py) by hand on 3 + 4 values, its NumPy twin against it, every seeded case's defining condition
(tests/_sitesplit_cases.py), rd_site_split_host against the restatement on every case, field and refusal, the header's bounds as
arithmetic, the workspace formula, the formulas of `compare --split` on a hand-built table, the stoichiometry and the per-read calls on
seeded sites, the bytes `compare` writes without --split, `simulate --mods-out` against the draws, the whole chain on the host twins
(the floors the GPU test holds the same chain to), and the host code under AddressSanitizer + UBSan as a stand-alone program
(tests/asan_sitesplit.cpp).  Every comparison of integers is for equality."""
import ctypes
import io
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _sitecmp_ref as cmp_ref
import _sitesplit_cases as sc
import _sitesplit_e2e as e2e
import _sitesplit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(got, want, where):
    for f in ref.FIELDS:
        a = getattr(got, f)
        assert a.dtype == want[f].dtype and a.shape == want[f].shape, (where, f, a.dtype, a.shape)
        assert np.array_equal(a, want[f]), (where, f)


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_by_hand_on_3_and_4_values():
    """a = 1 3 3, b = 2 3 5 5: pooled 1 2 3 3 3 5 5, N = 7, total 22.  Cuts 1, 2, 3 (5 is the pooled maximum):
    c = 1: n_lo 1, S_lo 1:  D = 1 * 6 - 21 * 1 = -15;  J = 225 / 6  = 37.5
    c = 2: n_lo 2, S_lo 3:  D = 3 * 5 - 19 * 2 = -23;  J = 529 / 10 = 52.9
    c = 3: n_lo 5, S_lo 12: D = 12 * 2 - 10 * 5 = -26; J = 676 / 10 = 67.6   <- the cut
    low cluster: a has 1 3 3 (n 3, sum 7, sumsq 19), b has 2 3 (n 2, sum 5, sumsq 13).
    With min_frac_q16 = 19661 (0.3) a cluster needs 65536 n >= 19661 * 7 = 137627, n >= 3: c = 1 and 2 fail on the low side, c = 3 (n_hi 2) on
    the high side -> NONE.  With 18000: 65536 n >= 126000, n >= 2: cuts 2 and 3 are admissible, 3 is still the best."""
    assert ref.cuts([1, 3, 3], [2, 3, 5, 5], 0) == [(1, -15, 1, 6), (2, -23, 2, 5), (3, -26, 5, 2)]
    e = ref.site_entry(4, [3, 1, 3], [5, 2, 5, 3])
    assert e == dict(out_site=4, status=ref.OK, n=(3, 4), sum=(7, 15), sumsq=(19, 63), cut=3, n_cuts=3, n_lo=(3, 2), sum_lo=(7, 5), sumsq_lo=(19, 13))
    assert ref.site_entry(4, [3, 1, 3], [5, 2, 5, 3], 19661)["status"] == ref.NONE
    e = ref.site_entry(4, [3, 1, 3], [5, 2, 5, 3], 18000)
    assert (e["status"], e["cut"], e["n_cuts"]) == (ref.OK, 3, 2)
    # one-sided and all-equal: totals only
    assert ref.site_entry(0, [], [4, 2]) == dict(out_site=0, status=ref.ONE_SIDED, n=(0, 2), sum=(0, 6), sumsq=(0, 20), cut=0, n_cuts=0, n_lo=(0, 0),
                                                 sum_lo=(0, 0), sumsq_lo=(0, 0))
    assert ref.site_entry(0, [4], [4, 4])["status"] == ref.NONE
    # the events in any order, two sites
    got = ref.split([9, 4, 4, 9, 4], [1, 0, 1, 0, 0], [7, -7, 0, 7, 2])
    assert [g["out_site"] for g in got] == [4, 9] and (got[0]["cut"], got[0]["n_lo"]) == (-7, (1, 0)) and got[1]["status"] == ref.NONE


def test_twin_equals_plain():
    rng = np.random.default_rng(5)
    for mf in (0, 9000, 32768):
        s, c, v = rng.integers(0, 6, 900), rng.integers(0, 2, 900), rng.integers(-40, 40, 900)
        assert ref.split_deep(s, c, v, mf) == ref.split(s, c, v, mf)
    for g in sc.all_groups():
        assert ref.split_deep(g["site"], g["cond"], g["value"], g["min_frac_q16"]) == sc.reference(g["name"]), g["name"]


def test_every_case_meets_its_defining_condition():
    groups = sc.all_groups() + [sc.deep_group()]
    names = [g["name"] for g in groups]
    assert len(set(names)) == len(names) == 11
    n_cond, seen = 0, set()
    for g in groups:
        by = {e["out_site"]: e for e in sc.reference(g["name"])}
        vals = ref.by_site(g["site"], g["cond"], g["value"])
        assert sorted(by) == sorted(set(g["site"].tolist()))
        for s, pred in g["cond_of"].items():
            assert pred(by[s], *vals[s]), (g["name"], s, by[s])
            n_cond += 1
        seen |= {e["status"] for e in by.values()}
    assert n_cond == 50 and seen == {ref.OK, ref.ONE_SIDED, ref.DEEP, ref.NONE}
    depths = {sum(e["n"]) for e in sc.reference("depths") if e["out_site"] < 100}
    assert depths == set(sc.DEPTHS) == {1, 2, 3, 63, 64, 65, sc.C - 1, sc.C, sc.C + 1, 3 * sc.C + 5} and len(depths) == 10
    g = next(g for g in groups if g["name"] == "interleaved")
    assert (g["site"][1:] != g["site"][:-1]).all()                     # no site is contiguous in the input
    g = next(g for g in groups if g["name"] == "wide_sites")
    assert g["n_sites"] == 2 ** 32 - 1 and {0, 2 ** 32 - 2} <= set(g["site"].tolist())
    assert {g["min_frac_q16"] for g in groups} == {0, sc.FRAC_Q16, 32768}
    # the recorded near-tie is what its search describes: three clusters inside their boxes, the two boundary cuts a part in 2^55 apart
    (n1, t, n3), (S1, T, H) = sc.NEAR_TIE
    lo, mid, hi = sc.near_tie_values()
    for vals, n, S, box in zip((lo, mid, hi), (n1, t, n3), (S1, T, H), sc.NEAR_TIE_BOXES):
        assert len(vals) == n and sum(vals) == S and box[0] <= min(vals) and max(vals) <= box[1] and max(vals) - min(vals) <= 1
    first, second = sc.ranked(lo + mid, hi)[:2]
    assert {first[0], second[0]} == {max(lo), max(mid)}
    gap = first[1] ** 2 * (second[2] * second[3]) - second[1] ** 2 * (first[2] * first[3])
    assert 0 < gap and gap << 55 < first[1] ** 2 * (second[2] * second[3]) and abs(first[1]) > 1 << 27


# ---------------------------------------------------------------------------------------------- the host entry point
def test_site_split_host_equals_the_restatement():
    from radian_amd.backend import SPLIT_FIELDS, site_split_host
    assert SPLIT_FIELDS == ref.FIELDS
    for g in sc.all_groups() + [sc.deep_group()]:
        want = ref.as_arrays(sc.reference(g["name"]))
        _equal(site_split_host(g["site"], g["cond"], g["value"], g["n_sites"], g["min_frac_q16"]), want, g["name"])
        if g["name"] != "deep":
            _equal(site_split_host(g["site"][::-1], g["cond"][::-1], g["value"][::-1], g["n_sites"], g["min_frac_q16"]), want, g["name"] + " reversed")
            _equal(site_split_host(g["site"], g["cond"], g["value"], g["n_sites"], g["min_frac_q16"], capacity=len(want["status"]) + 3), want,
                   g["name"] + " roomy")
    empty = site_split_host(np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int16), 5)
    assert len(empty.status) == 0
    # the totals are rd_site_compare_host's
    from radian_amd.backend import site_compare_host
    g = sc.all_groups()[0]
    a, b = site_split_host(g["site"], g["cond"], g["value"], g["n_sites"]), site_compare_host(g["site"], g["cond"], g["value"], g["n_sites"])
    for f in ("out_site", "n", "sum", "sumsq"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_every_refusal_of_the_host_entry_point():
    from radian_amd import _lib
    from radian_amd.backend import RadianHipError, SplitResult, _p, site_split_host
    site, cond, value = np.array([0, 1, 1], np.uint32), np.array([0, 1, 0], np.uint8), np.array([5, 6, 7], np.int16)
    L = _lib.load()

    def call(s, c, v, n_events, n_sites, cap, mf=0, null_out=None):
        res, n_out = SplitResult(2), ctypes.c_int64(-9)
        bufs = res._bufs()
        if null_out is not None:
            bufs[null_out] = None
        rc = L.rd_site_split_host(s, c, v, n_events, n_sites, cap, mf, *bufs, ctypes.byref(n_out))
        untouched = n_out.value == -9 and all((getattr(res, f) == 0).all() for f in ref.FIELDS)
        return rc, untouched, L.rd_last_error().decode()

    assert call(_p(site), _p(cond), _p(value), 3, 2, 2)[0] == 0 and call(_p(site), _p(cond), _p(value), 3, 2, 2, 32768)[0] == 0
    for args, word in (((None, _p(cond), _p(value), 3, 2, 2), "null"), ((_p(site), None, _p(value), 3, 2, 2), "null"),
                       ((_p(site), _p(cond), None, 3, 2, 2), "null"), ((_p(site), _p(cond), _p(value), 2 ** 31, 2, 2), "2^31 - 1"),
                       ((_p(site), _p(cond), _p(value), 3, 1, 2), "site 1"), ((_p(site), _p(cond), _p(value), 3, 2, 1), "2 distinct sites"),
                       ((_p(site), _p(cond), _p(value), 3, 2, 2, -1), "min_frac_q16"), ((_p(site), _p(cond), _p(value), 3, 2, 2, 32769), "min_frac_q16"),
                       ((_p(site), _p(cond), _p(value), 3, 2, -1), "capacity")):
        rc, untouched, msg = call(*args)
        assert rc == -1 and untouched and word in msg, (args[3:], msg)
    for k in range(10):
        assert call(_p(site), _p(cond), _p(value), 3, 2, 2, null_out=k)[0] == -1
    bad = cond.copy()
    bad[2] = 2
    rc, untouched, msg = call(_p(site), _p(bad), _p(value), 3, 2, 2)
    assert rc == -1 and untouched and "event 2 has cond 2" in msg
    with pytest.raises(RadianHipError):
        site_split_host(site, bad, value, 2)
    with pytest.raises(RadianHipError):
        site_split_host(site, cond, value, 2, min_frac_q16=40000)
    with pytest.raises(ValueError):
        site_split_host(site, cond[:2], value, 2)
    # n_events == 0 is RD_OK with n_out = 0, whatever the pointers
    n_out = ctypes.c_int64(-9)
    res = SplitResult(0)
    assert L.rd_site_split_host(None, None, None, 0, 5, 0, 0, *res._bufs(), ctypes.byref(n_out)) == 0 and n_out.value == 0


def test_the_headers_bounds_are_arithmetic():
    """include/radian_hip.h: with |v| <= 2^15 and N <= 2^16, |D| <= 2^16 n_lo n_hi <= 2^46, D^2 <= 2^92, n_lo n_hi <= 2^30 and a cross
    product is below 2^122: it fits one unsigned 128-bit word; the comparisons of the admissibility rule stay far inside int64"""
    N, V = 1 << 16, 1 << 15
    h = N // 2
    # |D| = |S_lo n_hi - S_hi n_lo| <= V n_lo n_hi + V n_hi n_lo
    assert 2 * V * h * h == 1 << 46 and (1 << 46) ** 2 == 1 << 92 and h * h == 1 << 30 and (1 << 92) * (1 << 30) == 1 << 122 < 1 << 128
    for n_lo in (1, 2, 100, h - 1, h, h + 1, N - 1):                      # n_lo n_hi is largest at the middle; so is the bound on |D|
        assert n_lo * (N - n_lo) <= h * h and 2 * V * n_lo * (N - n_lo) <= 1 << 46
    assert V * N * N < 1 << 63 and 65536 * N < 1 << 63 and 32768 * N < 1 << 63          # S_lo N, and both sides of the admissibility rule
    assert (2 ** 31 - 1) * V * V < 1 << 61 and (2 ** 31 - 1) * V < 1 << 63               # the prefix arrays over a whole launch
    # the extreme case of the cases reaches the bound's form
    by = {e["out_site"]: e for e in sc.reference("deep")}
    g = sc.deep_group()
    a, b = ref.by_site(g["site"], g["cond"], g["value"])[5]
    c = ref.cuts(a, b, 0)
    assert max(x[1] ** 2 * (y[2] * y[3]) for x in c for y in c).bit_length() == 122 and by[5]["status"] == ref.OK
    hdr = open(os.path.join(ROOT, "include", "radian_hip.h")).read()
    for word in ("<= 2^46", "D^2 <= 2^92", "n_lo n_hi <= 2^30", "below 2^122", "N > 2^16"):
        assert word in hdr, word
    from radian_amd.backend import SITE_NONE, SPLIT_STATUS_NAMES
    assert SITE_NONE == ref.NONE == 4 and SPLIT_STATUS_NAMES[ref.NONE] == "none" and "#define RD_SITE_NONE 4" in hdr


def test_the_workspace_formula():
    """rd_site_split_workspace_bytes(n) = rd_site_workspace_bytes(n) + 16 n + 112 ceil(n / 256), as the header states it"""
    from radian_amd.backend import site_split_workspace_bytes, site_workspace_bytes
    for n in (0, 1, 2, 255, 256, 257, 512, 513, 65536, 10 ** 6, 2 ** 31 - 1):
        assert site_split_workspace_bytes(n) == site_workspace_bytes(n) + 16 * n + 112 * ((n + 255) // 256) == 176 * n + 112 * ((n + 255) // 256), n
    assert site_split_workspace_bytes(-1) == -1 and site_split_workspace_bytes(2 ** 31) == -1
    hdr = open(os.path.join(ROOT, "include", "radian_hip.h")).read()
    assert "rd_site_workspace_bytes(n_events) + 16 n_events + 112 ceil(n_events / 256)" in hdr


# ---------------------------------------------------------------------------------------------- the command's host side
def test_split_statistics_by_hand():
    """the toy of the first test: a = 1 3 3, b = 2 3 5 5, cut 3: low cluster 1 2 3 3 3 (a: 3, b: 2), high cluster 5 5 (a: 0, b: 2).
    frac_hi 0 / 3 and 2 / 4; mean_lo 12 / 5, mean_hi 5; within sums of squares: low 5 * 32 - 144 = 16 -> 16 / 5 = 3.2, high 0;
    pooled sd = sqrt(3.2 / 5) = 0.8; sep = 2.6 / 0.8 = 3.25; lor = ln((0.5 * 2.5) / (3.5 * 2.5)) = ln(1 / 7);
    G = 2 [3 ln(3 * 7 / 15) + 2 ln(2 * 7 / 20) + 2 ln(2 * 7 / 8)] (the empty cell adds nothing)"""
    from radian_amd import compare
    e = ref.site_entry(0, [1, 3, 3], [2, 3, 5, 5])
    got = compare.split_stats(e["n"], e["n_lo"], e["sum"], e["sum_lo"], e["sumsq"], e["sumsq_lo"], e["cut"], 1.0)
    g = 2 * (3 * math.log(21 / 15) + 2 * math.log(14 / 20) + 2 * math.log(14 / 8))
    assert got[:5] == [3.0, 0.0, 0.5, 2.4, 5.0]
    assert got[5] == pytest.approx(3.25, rel=1e-15) and got[6] == pytest.approx(math.log(1 / 7), rel=1e-15)
    assert got[7] == pytest.approx(math.erfc(math.sqrt(g / 2)), rel=1e-14)
    # units: the level channel's 1/1024 z leaves fractions, sep, lor and p as they are and scales cut and the means
    lv = compare.split_stats(e["n"], e["n_lo"], e["sum"], e["sum_lo"], e["sumsq"], e["sumsq_lo"], e["cut"], 1024.0)
    assert lv[0] == 3 / 1024 and lv[3] == 2.4 / 1024 and lv[1:3] == got[1:3] and lv[5] == pytest.approx(got[5], rel=1e-15) and lv[6:] == got[6:]
    # two values and nothing else: no spread inside the clusters
    e = ref.site_entry(0, [5] * 6, [5, 9, 9, 9])
    inf = compare.split_stats(e["n"], e["n_lo"], e["sum"], e["sum_lo"], e["sumsq"], e["sumsq_lo"], e["cut"], 1.0)
    assert inf[5] == float("inf") and inf[1:3] == [0.0, 0.75] and inf[6] < 0
    # a table whose samples sit in both clusters alike: G = 0, p = 1
    e = ref.site_entry(0, [1, 1, 8, 8], [1, 8])
    same = compare.split_stats(e["n"], e["n_lo"], e["sum"], e["sum_lo"], e["sumsq"], e["sumsq_lo"], e["cut"], 1.0)
    assert same[7] == 1.0 and same[6] == pytest.approx(0.0, abs=1e-15)


def test_write_table_with_split_columns_on_a_hand_built_table():
    """three sites: a split ok site, an ok site whose values are all equal (split status NONE: nan split columns) and a low-depth site"""
    from radian_amd import compare
    site = np.array([2] * 30 + [41] * 24 + [45] * 6)
    cond = np.array([0] * 15 + [1] * 15 + [0] * 12 + [1] * 12 + [0, 0, 0, 1, 1, 1])
    value = np.array([10] * 8 + [50] * 7 + [10] * 14 + [50] + [7] * 24 + [1, 2, 3, 4, 5, 6])
    res = types.SimpleNamespace(**cmp_ref.as_arrays(cmp_ref.compare(site, cond, value)))
    spl = types.SimpleNamespace(**ref.as_arrays(ref.split(site, cond, value, 6554)))
    buf = io.StringIO()
    st = compare.write_table(buf, ["tA", "tB"], {"tA": (0, 40), "tB": (40, 100)}, {2: "A", 41: "C", 45: "G"}, {"dwell": res}, 10, 0.05, {"dwell": spl})
    rows = [ln.split("\t") for ln in buf.getvalue().splitlines()]
    assert rows[0] == ["ref_name", "pos", "base", "status", "n_a", "n_b"] + ["dwell_" + c for c in compare.STAT_COLUMNS + compare.SPLIT_COLUMNS]
    assert [r[:4] for r in rows[1:]] == [["tA", "2", "A", "ok"], ["tB", "1", "C", "ok"], ["tB", "5", "G", "low-depth"]]
    assert rows[1][17:20] == ["10.000000", f"{7 / 15:.6f}", f"{1 / 15:.6f}"] and rows[1][20:22] == ["10.000000", "50.000000"] and rows[1][22] == "inf"
    assert rows[1][25] == rows[1][24] and float(rows[1][24]) < 0.05          # one split site: split_q == split_p
    assert rows[2][17:] == ["nan"] * 9 and rows[2][16] != "nan" and rows[3][17:] == ["nan"] * 9
    assert st["split"] == {"dwell": {2: 10}}
    # without the splits the same call writes the parent's table: the first 17 columns
    plain = io.StringIO()
    st0 = compare.write_table(plain, ["tA", "tB"], {"tA": (0, 40), "tB": (40, 100)}, {2: "A", 41: "C", 45: "G"}, {"dwell": res}, 10, 0.05)
    assert [ln.split("\t") for ln in plain.getvalue().splitlines()] == [r[:17] for r in rows] and "split" not in st0
    text = compare.summary({k: {"files": 1, "events": 9, "kept": 8, "reads-no-mapping": 1, "no-mapping": 1, "low-q": 0, "bad-level": 0} for k in "ab"}, st,
                           ["dwell"], 0.05)
    assert "dwell split: 1 sites with split_q <= 0.05 (thresholds not calibrated)" in text
    # the per-read rows: events of site 2 only, in input order, cluster = value > cut
    reads = {"ids": [f"r{i}" for i in range(60)], "index": np.arange(60, dtype=np.uint32)}
    out = io.StringIO()
    n = compare.write_reads(out, ["tA", "tB"], {"tA": (0, 40), "tB": (40, 100)}, reads, site, cond, {"dwell": value}, ["dwell"], st["split"])
    got = [ln.split("\t") for ln in out.getvalue().splitlines()]
    assert n == 30 and got[0] == ["read_id", "sample", "ref_name", "pos", "channel", "value", "cluster"]
    assert got[1:] == [[f"r{i}", "ab"[cond[i]], "tA", "2", "dwell", str(value[i]), str(int(value[i] > 10))] for i in range(30)]


def _synthetic_split_sites(seed, n_sites=300, depth=40, noise=0.1, shift=1.0, frac=0.5):
    """sites in the style of radian_amd.synthetic.site_events: a level of its own per site (uniform over -1.5 .. 1.5 z), `depth` events
    per sample with Gaussian noise; at every tenth site `frac` of sample A's events are moved by `shift`.  -> (site, cond, level, moved)"""
    rng = np.random.default_rng(seed)
    site = np.repeat(np.arange(n_sites), 2 * depth)
    cond = np.tile(np.repeat([0, 1], depth), n_sites).astype(np.uint8)
    level = np.repeat(rng.uniform(-1.5, 1.5, n_sites), 2 * depth) + noise * rng.standard_normal(site.size)
    moved = np.zeros(site.size, dtype=bool)
    k = int(round(frac * depth))
    for s in range(0, n_sites, 10):
        moved[s * 2 * depth: s * 2 * depth + k] = True
    return site, cond, level + shift * moved, moved


def test_stoichiometry_and_read_calls_on_seeded_sites():
    """300 sites at depth 40 per sample, event noise 0.1 z, every tenth site with half of sample A moved by 1.0 z (seed 26), through the
    restatement's integers and the command's formulas at --split-min-frac 0.1.  Measured here: 30 of 30 modified sites with split_q <=
    0.05 and 0 of 270 unmodified ones; at the modified sites frac_hi_a is 0.5 to within 0.0 at the worst site and 1200 of 1200 events of
    sample A fall on the side of the cut they were drawn on.  Each floor is one site (one event) under the measured count: it guards a
    reseed."""
    from radian_amd import compare
    site, cond, level, moved = _synthetic_split_sites(26)
    value = compare.quantise_level(level)
    entries = ref.split(site, cond, value, int(np.rint(0.1 * 65536)))
    assert len(entries) == 300 and all(e["status"] == ref.OK for e in entries)
    stats = [compare.split_stats(e["n"], e["n_lo"], e["sum"], e["sum_lo"], e["sumsq"], e["sumsq_lo"], e["cut"], 1024.0) for e in entries]
    q = compare.benjamini_hochberg([s[7] for s in stats])
    modified = set(range(0, 300, 10))
    hit = {e["out_site"] for e, v in zip(entries, q) if v <= 0.05}
    worst = max(abs(stats[s][1] - 0.5) for s in modified)
    right = sum(int((value[i] > entries[site[i]]["cut"]) == moved[i]) for i in range(site.size) if site[i] in modified and cond[i] == 0)
    print(f"modified sites called {len(hit & modified)} of 30; unmodified sites called {len(hit - modified)} of 270; worst |frac_hi_a - 0.5| {worst:.4f}; "
          f"sample A's events on their side of the cut {right} of 1200")
    assert len(hit & modified) >= 29                   # measured 30
    assert len(hit - modified) <= 1                    # measured 0
    assert worst <= 1 / 40                             # measured 0.0: one event of 40
    assert right >= 1199                               # measured 1200
    assert all(stats[s][2] == 0.0 for s in modified)   # sample B has nothing above the cut there


def _compare_args(tmp_path, extra=()):
    from radian_amd import compare
    return compare.build_parser().parse_args(["--a", str(tmp_path / "A"), "--a-paf", str(tmp_path / "a.paf"), "--b", str(tmp_path / "B"), "--b-paf",
                                              str(tmp_path / "b.paf"), "-o", str(tmp_path / "o.tsv"), "--min-depth", "3"] + list(extra))


def _two_samples(tmp_path):
    """two event directories and PAFs over one transcript of 12 sites: sample A's events at sites 2 .. 7 come in two clusters"""
    rng = np.random.default_rng(9)
    header = "read_id\tref_name\tref_pos\tbase\tstart\tend\tn\tmean\tstdv\tmin\tmax\tlevel\tq\n"
    for c, d in enumerate("AB"):
        os.makedirs(tmp_path / d)
        rows, paf = [], []
        for r in range(14):
            rid = f"{d}{r}"
            paf.append(f"{rid}\t12\t0\t12\t+\ttX\t12\t0\t12\t12\t12\t255\n")
            for pos in range(12):
                lv = 0.2 * pos + 0.05 * rng.standard_normal() + (0.9 if c == 0 and 2 <= pos <= 7 and r % 2 else 0.0)
                rows.append(f"{rid}\ttX\t{pos}\t{'ACGT'[pos % 4]}\t0\t1\t{int(rng.integers(3, 40))}\t0.0\t0.0\t0\t0\t{lv:.6f}\t20\n")
        (tmp_path / d / "e.events.tsv").write_text(header + "".join(rows))
        (tmp_path / f"{d.lower()}.paf").write_text("".join(paf))


def test_without_split_the_command_writes_the_parents_bytes(tmp_path, monkeypatch, capsys):
    """`compare` without --split against the table its formulas write from tests/_sitecmp_ref.py's integers (the parent's whole output);
    with --split the first columns of every channel are those same bytes.  On the host twins."""
    from radian_amd import compare
    e2e.on_the_host(monkeypatch)
    _two_samples(tmp_path)
    args = _compare_args(tmp_path)
    compare.check_args(args)
    compare.main(["--a", args.a, "--a-paf", args.a_paf, "--b", args.b, "--b-paf", args.b_paf, "-o", args.out, "--min-depth", "3"])
    text = capsys.readouterr().out
    names, offsets, n_sites, bases, site, cond, values, sample_st = compare.load(args)
    assert "reads" not in sample_st                                           # no read index is kept without --reads-out
    results = {ch: types.SimpleNamespace(**cmp_ref.as_arrays(cmp_ref.compare(site, cond, values[ch]))) for ch in compare.CHANNELS}
    want = io.StringIO()
    st = compare.write_table(want, names, offsets, bases, results, 3, 0.05)
    plain = open(args.out, "rb").read()
    assert plain == want.getvalue().encode()
    assert text == compare.summary(sample_st, st, list(compare.CHANNELS), 0.05) and "split" not in text
    # with --split: the same rows with nine more columns per channel, and per-read rows at the called sites
    compare.main(["--a", args.a, "--a-paf", args.a_paf, "--b", args.b, "--b-paf", args.b_paf, "-o", str(tmp_path / "s.tsv"), "--min-depth", "3", "--split",
                  "--reads-out", str(tmp_path / "r.tsv")])
    text2 = capsys.readouterr().out
    rows0 = [ln.split("\t") for ln in plain.decode().splitlines()]
    rows1 = [ln.split("\t") for ln in open(tmp_path / "s.tsv").read().splitlines()]
    assert [r[:17] + r[26:37] for r in rows1] == rows0 and len(rows1[0]) == 6 + 2 * 20
    assert text2.startswith(text) and "level split: " in text2 and "thresholds not calibrated" in text2
    called = {int(r[1]) for r in rows1[1:] if r[25] != "nan" and float(r[25]) <= 0.05}
    assert {2, 3, 4, 5, 6, 7} <= called
    reads = [ln.split("\t") for ln in open(tmp_path / "r.tsv").read().splitlines()][1:]
    level_rows = [r for r in reads if r[4] == "level"]
    assert {int(r[3]) for r in level_rows} == called and len(level_rows) == 28 * len(called)
    for r in level_rows:
        if int(r[3]) in (2, 3, 4, 5, 6, 7):
            assert int(r[6]) == (1 if r[0].startswith("A") and int(r[0][1:]) % 2 else 0), r
    # refusals of the new flags
    for bad in (["--split", "--split-min-frac", "0.6"], ["--split", "--split-min-frac", "-0.1"], ["--reads-out", "x.tsv"]):
        with pytest.raises(SystemExit):
            compare.check_args(_compare_args(tmp_path, bad))


# ---------------------------------------------------------------------------------------------- simulate --mods-out
def test_mods_out_agrees_with_the_draws(tmp_path, monkeypatch, capsys):
    """the same seed with --modify at fraction 0 and at fraction 1: `modified` is all 0 / all 1, one row for every read and site the read
    covers; at fraction 0.5 the column is the draw (a read is modified exactly where its plan says); and --mods-out changes no other file"""
    from radian_amd import simulate
    e2e.on_the_host(monkeypatch)
    fa, _ = e2e.write_inputs(str(tmp_path))
    sites = [("t0", 40), ("t0", 250), ("t1", 300)]                              # t0:40 is covered only by fragments of 260 bases and more

    def run(frac, name, mods_out=True):
        mod = tmp_path / f"m{name}.tsv"
        mod.write_text("".join(f"{t}\t{p}\t1.0\t1.0\t{frac}\n" for t, p in sites))
        out = tmp_path / name
        argv = [fa, "-o", str(out), "--reads", "12", "--seed", "5", "--length-median", "250", "--length-sigma", "0.2", "--min-length", "200", "--tail",
                "20", "--model-seed", "7", "--modify", str(mod)] + (["--mods-out", str(tmp_path / f"{name}.mods.tsv")] if mods_out else [])
        simulate.main(argv)
        capsys.readouterr()
        rows = [ln.split("\t") for ln in open(tmp_path / f"{name}.mods.tsv").read().splitlines()] if mods_out else None
        return rows, {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}

    rows0, files0 = run(0.0, "f0")
    rows1, files1 = run(1.0, "f1")
    assert rows0[0] == rows1[0] == ["read_id", "ref_name", "pos", "modified"]
    assert [r[:3] for r in rows0] == [r[:3] for r in rows1] and {r[3] for r in rows0[1:]} == {"0"} and {r[3] for r in rows1[1:]} == {"1"}
    truth = {r[0]: (r[1], int(r[2]), int(r[3])) for r in [ln.split("\t") for ln in files0["truth.tsv"].decode().splitlines()][1:]}
    want = [[rid, name, str(p)] for rid, (name, a, e) in truth.items() for t, p in sites if t == name and a <= p < e]
    assert [r[:3] for r in rows0[1:]] == want and 12 < len(want) < 24         # t0:40 is covered by some of t0's reads only
    assert files0["truth.tsv"] == files1["truth.tsv"] and files0["sim_0000.fast5"] != files1["sim_0000.fast5"]
    # fraction 0.5: the column is the plan's draw
    args = simulate.build_parser().parse_args([fa, "-o", "x", "--reads", "12", "--seed", "5", "--length-median", "250", "--length-sigma", "0.2",
                                               "--min-length", "200", "--tail", "20", "--model-seed", "7"])
    from radian_amd.map import Transcripts
    tr = Transcripts.read(fa, None, None)
    (tmp_path / "mh.tsv").write_text("".join(f"{t}\t{p}\t1.0\t1.0\t0.5\n" for t, p in sites))
    plans = simulate.draw_reads(args, tr, np.random.Generator(np.random.PCG64(5)), simulate.read_sites(str(tmp_path / "mh.tsv"), tr))
    rows_h, files_h = run(0.5, "fh")
    assert [r for r in rows_h[1:]] == [[p.read_id, tr.names[p.t], str(pos), str(hit)] for p in plans for pos, hit in p.covered]
    assert all({pos for pos, hit in p.covered if hit} == {m[0] for m in p.mods} for p in plans) and {r[3] for r in rows_h[1:]} == {"0", "1"}
    # without --mods-out every other file is the same, byte for byte
    _, files_n = run(0.5, "fn", mods_out=False)
    assert files_n == files_h
    with pytest.raises(SystemExit, match="--mods-out goes with --modify"):
        simulate.check_args(simulate.build_parser().parse_args([fa, "-o", "x", "--reads", "1", "--mods-out", "m.tsv"]))


# ---------------------------------------------------------------------------------------------- the chain on the host twins
def test_the_chain_on_the_host_twins_sets_the_floors(tmp_path, monkeypatch):
    """tests/_sitesplit_e2e.py on rd_sim_signal_host, rd_eventalign_host, rd_site_compare_host and rd_site_split_host: the files equal the
    tables written from the restatements' integers; the three modified sites have level split_q <= 0.05 (measured 2.0e-6, 6.7e-4 and
    2.4e-8); frac_hi_a times the reads equals the reads --mods-out calls modified (17 of 28, 12 of 28, 24 of 36: measured difference 0
    reads) and no read of either sample is in the wrong cluster (measured 0 of 59, 59 and 69).  The floors of the GPU test are these less
    one read per site."""
    e2e.on_the_host(monkeypatch)
    for (name, pos) in e2e.MOD_SITES:
        assert e2e.level_margin(name, pos) >= 2.5 and pos >= e2e.LENGTHS[int(name[1:])] - 200 + 2
    outs, dirs = e2e.run_chain(str(tmp_path))
    sites, reads, text = outs[0]
    table, rows, st = e2e.expected_tables(dirs, str(tmp_path))
    assert sites.decode() == table and reads.decode() == rows
    rec = e2e.recovery(table, rows, open(tmp_path / "mods_a.tsv").read())
    print("split_q, reads of A, modified, frac_hi_a * reads, wrong calls, calls:", rec)
    assert tuple(r[1] for r in rec) == e2e.MEASURED["n_a"] and tuple(r[2] for r in rec) == e2e.MEASURED["modified"]
    assert tuple(round(r[3]) for r in rec) == e2e.MEASURED["above"] and tuple(r[4] for r in rec) == e2e.MEASURED["wrong"]
    for q, n_a, modified, above, wrong, calls in rec:
        assert q <= e2e.ALPHA and abs(above - modified) <= e2e.FRAC_TOLERANCE_READS and wrong <= e2e.WRONG_READS and calls >= n_a
    assert f"level split: {len(st['split']['level'])} sites with split_q <= 0.05 (thresholds not calibrated)" in text


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_site_split_host(tmp_path):
    """tests/asan_sitesplit.cpp: the host side of the split (argument check, the rules of site_rules.h, the launch plan and buckets under
    rd_site_split_workspace_bytes, the host twin) built with AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap
    buffers of the cases' shapes; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_sitesplit"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_sitesplit.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 400 and int(last[2]) >= 1800          # "<n> accepted <m> refused"
