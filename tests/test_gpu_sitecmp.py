"""GPU checks of the two-sample site comparison (rd_site_compare / rd_site_diag_segments, radian_amd/csrc/sitecmp.hip) against the
plain-Python restatement of its contract (tests/_sitecmp_ref.py) and against rd_site_compare_host, and of `python -m radian_amd.compare`.
Everything is compared for EXACT equality.

Sizes follow the kernels (tests/_sitecmp_cases.py; every case's defining condition is asserted in tests/test_sitecmp_cpu.py): a wave of
the site kernel takes a chunk of C = 256 elements of one site, 64 lanes wide -- sites of 1, 2, 63, 64, 65, C - 1, C, C + 1 and 3C + 5
events, one event against C + 1, site ids up to 2^32 - 2, and one site of 2^20 events (4096 chunks, the deepest that gets rank
statistics) beside one of 2^20 + 1 (DEEP)."""
import io
import types

import numpy as np
import pytest

import _sitecmp_cases as sc
import _sitecmp_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    return sc.all_groups()


def _equal(got, want, where):
    for f in ref.FIELDS:
        a = getattr(got, f)
        assert a.dtype == want[f].dtype and a.shape == want[f].shape, (where, f, a.dtype, a.shape)
        assert np.array_equal(a, want[f]), (where, f)


def test_diag_segments_equal_the_restatement(be, groups):
    for g in groups:
        keys, segs = be.site_diag_segments(g["site"], g["cond"], g["value"], g["n_sites"])
        e_keys, e_segs = ref.segments(g["site"], g["cond"], g["value"])
        assert keys.dtype == np.uint64 and segs.dtype == np.int64
        assert keys.tolist() == e_keys, g["name"]
        assert [tuple(s) for s in segs.tolist()] == e_segs, g["name"]


def test_site_compare_equals_the_restatement_and_the_host(be, groups):
    from radian_amd.backend import site_compare_host
    seen = set()
    for g in groups:
        want = ref.as_arrays(sc.reference(g["name"]))
        got = be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"])
        _equal(got, want, g["name"])
        host = site_compare_host(g["site"], g["cond"], g["value"], g["n_sites"])
        for f in ref.FIELDS:
            assert getattr(got, f).dtype == getattr(host, f).dtype and np.array_equal(getattr(got, f), getattr(host, f)), (g["name"], f)
        seen |= set(got.status.tolist())
    assert seen == {ref.OK, ref.ONE_SIDED}
    empty = be.site_compare(np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int16), 5)
    assert len(empty.status) == 0


def test_site_compare_does_not_depend_on_the_order_of_the_events(be, groups):
    rng = np.random.default_rng(31)
    for g in groups:
        want = ref.as_arrays(sc.reference(g["name"]))
        _equal(be.site_compare(g["site"][::-1], g["cond"][::-1], g["value"][::-1], g["n_sites"]), want, g["name"] + " reversed")
        p = rng.permutation(len(g["site"]))
        _equal(be.site_compare(g["site"][p], g["cond"][p], g["value"][p], g["n_sites"]), want, g["name"] + " permuted")


def _launches(needs, budget):
    """the planner restated: consecutive sites under the budget; a site over it alone ends the open launch"""
    n, acc = 0, None
    for b in needs:
        if b > budget:
            acc = None
        elif acc is None or acc + b > budget:
            n, acc = n + 1, b
        else:
            acc += b
    return n


def test_site_compare_does_not_depend_on_the_budget(be, groups):
    from radian_amd.backend import site_workspace_bytes
    g = groups[0]
    entries = sc.reference(g["name"])
    want = ref.as_arrays(entries)
    needs = [site_workspace_bytes(sum(e["n"])) for e in entries]
    assert needs == [160 * sum(e["n"]) for e in entries]
    budget = max(needs) + 160
    assert _launches(needs, budget) >= 3                                 # at least three launches
    _equal(be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"], budget_bytes=budget), want, "three launches")
    tight = sorted(needs)[len(needs) // 2]                               # the median site's need: many launches, half the sites left out
    got = be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"], budget_bytes=tight, allow_too_large=True)
    assert _launches(needs, tight) >= 3
    for j, e in enumerate(entries):
        assert (got.status[j] == ref.TOO_LARGE) == (needs[j] > tight), j
        if needs[j] <= tight:
            for f in ref.FIELDS:
                assert np.array_equal(getattr(got, f)[j], want[f][j]), (j, f)


def test_a_budget_under_one_sites_need(be, groups):
    from radian_amd import RadianHipError
    g = groups[0]
    entries = sc.reference(g["name"])
    want = ref.as_arrays(entries)
    needs = [160 * sum(e["n"]) for e in entries]
    big = int(np.argmax(needs))
    budget = needs[big] - 1
    assert sorted(needs)[-2] <= budget
    with pytest.raises(RadianHipError) as ei:
        be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"], budget_bytes=budget)
    msg = str(ei.value)
    assert "[rd error -4]" in msg and f"site {entries[big]['out_site']} " in msg and "1 site(s) not compared" in msg
    got = be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"], budget_bytes=budget, allow_too_large=True)
    for j in range(len(entries)):
        for f in ref.FIELDS:
            if j == big and f not in ("out_site", "n"):
                assert np.array_equal(getattr(got, f)[j], np.array(ref.TOO_LARGE if f == "status" else 0) * np.ones_like(want[f][j])), f
            else:
                assert np.array_equal(getattr(got, f)[j], want[f][j]), (j, f)


def test_site_compare_refuses_bad_arguments_before_anything_is_launched(be):
    import ctypes
    from radian_amd.backend import SiteResult, _p
    site, cond, value = np.array([0, 1, 1], np.uint32), np.array([0, 1, 0], np.uint8), np.array([5, 6, 7], np.int16)

    def call(h, s, c, v, n_events, n_sites, budget, cap):
        res, n_out = SiteResult(2), ctypes.c_int64(-9)
        rc = be._L.rd_site_compare(h, s, c, v, n_events, n_sites, budget, cap, *res._bufs(), ctypes.byref(n_out))
        return rc, n_out.value == -9 and all((getattr(res, f) == 0).all() for f in ref.FIELDS)

    assert call(be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 2) == (0, False)
    bad = cond.copy()
    bad[0] = 3
    for args in ((None, _p(site), _p(cond), _p(value), 3, 2, 0, 2), (be._h, None, _p(cond), _p(value), 3, 2, 0, 2),
                 (be._h, _p(site), None, _p(value), 3, 2, 0, 2), (be._h, _p(site), _p(cond), None, 3, 2, 0, 2),
                 (be._h, _p(site), _p(cond), _p(value), 2 ** 31, 2, 0, 2), (be._h, _p(site), _p(cond), _p(value), 3, 1, 0, 2),
                 (be._h, _p(site), _p(bad), _p(value), 3, 2, 0, 2), (be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 1),
                 (be._h, _p(site), _p(cond), _p(value), 3, 2, -1, 2)):
        assert call(*args) == (-1, True), args[4:]
    rc, untouched = call(be._h, None, None, None, 0, 2, 0, 0)           # n_events == 0 is RD_OK with n_out = 0
    assert rc == 0 and not untouched


def test_a_site_of_2_to_the_20_events_and_one_more(be):
    from radian_amd.backend import site_compare_host
    g = sc.deep_group()
    want = ref.as_arrays(sc.reference("deep"))
    assert want["status"].tolist() == [ref.DEEP, ref.OK] and want["n"].sum(axis=1).tolist() == [2 ** 20 + 1, 2 ** 20]
    _equal(be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"]), want, "deep")
    _equal(site_compare_host(g["site"], g["cond"], g["value"], g["n_sites"]), want, "deep, host")


# ---------------------------------------------------------------------------------------------- the command
HEADER = "read_id\tref_name\tref_pos\tbase\tstart\tend\tn\tmean\tstdv\tmin\tmax\tlevel\tq\n"
TRANSCRIPTS = (("tB|second", 0, 25), ("tA|first", 25, 40))     # (name, first synthetic site, sites): sorted by name, tA comes first


def _build_sample(tmp_path, ev, c, rng, missing):
    """sample c of synthetic.site_events as an events directory and a PAF: read `s{c}_{name}_{k}` holds the k-th event of every site of
    one transcript that has one; its span starts at the first such site.  -> (directory, PAF path, the events the command must keep as
    (transcript, position, level as printed, dwell), counters)"""
    d = tmp_path / f"events_{c}"
    d.mkdir()
    kept, paf, files = [], [], {0: [], 1: []}
    st = {"events": 0, "no-mapping": 0, "low-q": 0, "reads-no-mapping": 0}
    for name, first, n in TRANSCRIPTS:
        per_site = {s: np.flatnonzero((ev["site"] == first + s) & (ev["cond"] == c)) for s in range(n)}
        for k in range(max(len(v) for v in per_site.values())):
            rid = f"s{c}_{name.split('|')[0]}_{k}"
            sites = [s for s in range(n) if len(per_site[s]) > k]
            start = sites[0]
            absent = rid == missing
            if not absent:
                paf.append(f"{rid}\t{n}\t0\t{n}\t+\t{name}\t{n + 7}\t{start + 3}\t{n + 3}\t{n}\t{n}\t255\ts1:i:9\n")
            st["reads-no-mapping"] += absent
            for s in sites:
                i = per_site[s][k]
                q = int(rng.integers(0, 30))
                level = f"{ev['level'][i]:.6f}"
                files[k % 2].append(f"{rid}\t{name}\t{s - start}\t{'ACGT'[(first + s) % 4]}\t0\t1\t{int(ev['dwell'][i])}\t0.0\t0.0\t0\t0\t{level}\t{q}\n")
                st["events"] += 1
                if absent:
                    st["no-mapping"] += 1
                elif q < 5:
                    st["low-q"] += 1
                else:
                    kept.append((name, s + 3, float(level), int(ev["dwell"][i])))
    for k, rows in files.items():
        with open(d / f"part{k}.events.tsv", "w") as f:
            f.write(HEADER + "".join(rows))
    with open(tmp_path / f"sample_{c}.paf", "w") as f:
        f.write("".join(paf))
    return str(d), str(tmp_path / f"sample_{c}.paf"), kept, st


def test_command_on_two_hand_built_samples(be, tmp_path, capsys):
    """byte-identical to the table the command's own host formulas write from the restatement's integers, and across --budget-bytes; one
    read is missing from its PAF, events below --min-q are dropped; the summary's counts"""
    from radian_amd import compare, synthetic
    rng = np.random.default_rng(41)
    ev = synthetic.site_events(rng, n_sites=65, median_depth=22.0, sigma=0.7, shifted=(3, 11, 30), level_shift=1.0)
    built = [_build_sample(tmp_path, ev, c, rng, "s0_tA_1") for c in (0, 1)]
    outs, texts = {}, {}
    tight = 160 * 400                                                    # holds any site here, and the events need more than three of it
    assert ev["depth"].sum(axis=1).max() < 400 and ev["depth"].sum() > 6 * 400
    for budget in (0, tight):
        argv = ["--a", built[0][0], "--a-paf", built[0][1], "--b", built[1][0], "--b-paf", built[1][1], "-o", str(tmp_path / f"sites{budget}.tsv"),
                "--min-q", "5", "--min-depth", "8", "--budget-bytes", str(budget)]
        compare.main(argv)
        texts[budget] = capsys.readouterr().out
        outs[budget] = open(tmp_path / f"sites{budget}.tsv", "rb").read()
    assert outs[0] == outs[tight] and texts[0] == texts[tight]
    # the same table from the restatement: transcripts sorted by name, tA|first (47 bases) then tB|second (32 bases)
    names, offsets = ["tA|first", "tB|second"], {"tA|first": (0, 47), "tB|second": (47, 32)}
    site, cond, level, dwell, bases = [], [], [], [], {}
    for c in (0, 1):
        for name, pos, lv, dw in built[c][2]:
            site.append(offsets[name][0] + pos)
            cond.append(c)
            level.append(lv)
            dwell.append(dw)
    for name, first, n in TRANSCRIPTS:
        for s in range(n):
            bases[offsets[name][0] + s + 3] = "ACGT"[(first + s) % 4]
    results = {"level": types.SimpleNamespace(**ref.as_arrays(ref.compare(site, cond, compare.quantise_level(level)))),
               "dwell": types.SimpleNamespace(**ref.as_arrays(ref.compare(site, cond, compare.quantise_dwell(dwell))))}
    buf = io.StringIO()
    st = compare.write_table(buf, names, offsets, bases, results, 8, 0.05)
    assert outs[0].decode() == buf.getvalue()
    rows = [ln.split("\t") for ln in outs[0].decode().splitlines()]
    assert len(rows[0]) == 6 + 22 and len(rows) == 1 + len(set(site)) and rows[1][0] == "tA|first" and rows[-1][0] == "tB|second"
    assert st["ok"] >= 20 and st["ok"] + st["low-depth"] + st["one-sided"] == len(set(site)) and st["significant"]["level"] >= 2
    text = texts[0]
    for c, name in ((0, "A"), (1, "B")):
        b = built[c][3]
        assert f"sample {name}: 2 files, {b['events']} events read, {len(built[c][2])} kept" in text
        assert f"dropped: no-mapping: {b['no-mapping']}; low-q: {b['low-q']}; bad-level: 0 ({b['reads-no-mapping']} reads absent from the PAF)" in text
    assert built[0][3]["reads-no-mapping"] == 1 and built[0][3]["no-mapping"] > 0 and built[0][3]["low-q"] > 0 and built[1][3]["no-mapping"] == 0
    assert "sites: " + "; ".join(f"{s}: {st[s]}" for s in compare.ROW_STATUS) in text
    assert f"level: {st['significant']['level']} sites with q <= 0.05" in text and f"dwell: {st['significant']['dwell']} sites with q <= 0.05" in text
    # one channel alone writes that channel's columns, identical to the same columns of the full table
    compare.main(["--a", built[0][0], "--a-paf", built[0][1], "--b", built[1][0], "--b-paf", built[1][1], "-o", str(tmp_path / "dwell.tsv"), "--min-q", "5",
                  "--min-depth", "8", "--channel", "dwell"])
    capsys.readouterr()
    alone = [ln.split("\t") for ln in open(tmp_path / "dwell.tsv").read().splitlines()]
    assert alone == [r[:6] + r[17:] for r in rows]
