"""GPU checks of the exact two-cluster split (rd_site_split, radian_amd/csrc/sitecmp.hip) against the plain-Python
restatement of its contract (tests/_sitesplit_ref.py) and against rd_site_split_host, and of `python -m radian_amd.compare --split`.
Everything is compared for EXACT equality.

Sizes follow the kernels (tests/_sitesplit_cases.py; every case's defining condition is asserted in tests/test_sitesplit_cpu.py): a wave
takes a chunk of C = 256 sorted elements of one site, 64 lanes wide, and a second kernel picks the best of a site's chunks -- sites of 1,
2, 3, 63, 64, 65, C - 1, C, C + 1 and 3C + 5 events, cuts evaluated at the last element of a chunk, the first of the next and in the
third chunk, an exact tie met across chunks, a near-tie that fp64 cannot order, site ids up to 2^32 - 2, and sites of 2^16 events (256
chunks, the deepest that are split: one at the int16 extremes, whose cross products take 122 bits) beside one of 2^16 + 1 (DEEP)."""
import os

import numpy as np
import pytest

import _sitesplit_cases as sc
import _sitesplit_e2e as e2e
import _sitesplit_ref as ref

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
        assert np.array_equal(a, want[f]), (where, f, a, want[f])


def _call(be, g, **kw):
    return be.site_split(g["site"], g["cond"], g["value"], g["n_sites"], g["min_frac_q16"], **kw)


def test_site_split_equals_the_restatement_and_the_host(be, groups):
    """every group in one call (min_frac_q16 is the call's), field by field and dtype by dtype"""
    from radian_amd.backend import site_split_host
    seen = set()
    for g in groups:
        want = ref.as_arrays(sc.reference(g["name"]))
        got = _call(be, g)
        _equal(got, want, g["name"])
        host = site_split_host(g["site"], g["cond"], g["value"], g["n_sites"], g["min_frac_q16"])
        for f in ref.FIELDS:
            assert getattr(got, f).dtype == getattr(host, f).dtype and np.array_equal(getattr(got, f), getattr(host, f)), (g["name"], f)
        seen |= set(got.status.tolist())
    assert seen == {ref.OK, ref.ONE_SIDED, ref.NONE}
    empty = be.site_split(np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int16), 5)
    assert len(empty.status) == 0


def test_every_group_with_min_frac_0_in_one_call(be, groups):
    """the groups whose min_frac_q16 is 0, side by side in one call under site ids of their own: a site never affects another"""
    site, cond, value, want, base = [], [], [], [], 0
    for g in groups:
        if g["min_frac_q16"] != 0 or g["name"] == "wide_sites":
            continue
        site.append(g["site"].astype(np.uint64) + base)
        cond.append(g["cond"])
        value.append(g["value"])
        want += [dict(e, out_site=e["out_site"] + base) for e in sc.reference(g["name"])]
        base += 1000
    site = np.concatenate(site).astype(np.uint32)
    got = be.site_split(site, np.concatenate(cond), np.concatenate(value), base)
    _equal(got, ref.as_arrays(want), "all in one")
    assert len(want) >= 40


def test_site_split_does_not_depend_on_the_order_of_the_events(be, groups):
    rng = np.random.default_rng(31)
    for g in groups:
        want = ref.as_arrays(sc.reference(g["name"]))
        _equal(be.site_split(g["site"][::-1], g["cond"][::-1], g["value"][::-1], g["n_sites"], g["min_frac_q16"]), want, g["name"] + " reversed")
        p = rng.permutation(len(g["site"]))
        _equal(be.site_split(g["site"][p], g["cond"][p], g["value"][p], g["n_sites"], g["min_frac_q16"]), want, g["name"] + " permuted")


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


def _need(n):
    return 176 * n + 112 * ((n + 255) // 256)


def test_site_split_does_not_depend_on_the_budget(be, groups):
    from radian_amd.backend import site_split_workspace_bytes
    g = groups[0]
    entries = sc.reference(g["name"])
    want = ref.as_arrays(entries)
    needs = [site_split_workspace_bytes(sum(e["n"])) for e in entries]
    assert needs == [_need(sum(e["n"])) for e in entries]
    budget = max(needs) + 176
    assert _launches(needs, budget) >= 3                                 # at least three launches
    _equal(_call(be, g, budget_bytes=budget), want, "three launches")
    tight = sorted(needs)[len(needs) // 2]                               # the median site's need: many launches, half the sites left out
    got = _call(be, g, budget_bytes=tight, allow_too_large=True)
    assert _launches(needs, tight) >= 3
    for j, e in enumerate(entries):
        assert (got.status[j] == ref.TOO_LARGE) == (needs[j] > tight), j
        if needs[j] <= tight:
            for f in ref.FIELDS:
                assert np.array_equal(getattr(got, f)[j], want[f][j]), (j, f)
    # the tie across chunks and the near-tie under a budget that gives every site a launch of its own
    for name in ("tie", "near_tie", "locations"):
        g = next(x for x in groups if x["name"] == name)
        e = sc.reference(name)
        _equal(_call(be, g, budget_bytes=max(_need(sum(x["n"])) for x in e)), ref.as_arrays(e), name + ", one site per launch")


def test_a_budget_one_byte_under_the_largest_sites_need(be, groups):
    from radian_amd import RadianHipError
    g = groups[0]
    entries = sc.reference(g["name"])
    want = ref.as_arrays(entries)
    needs = [_need(sum(e["n"])) for e in entries]
    big = int(np.argmax(needs))
    budget = needs[big] - 1
    assert sorted(needs)[-2] <= budget
    with pytest.raises(RadianHipError) as ei:
        _call(be, g, budget_bytes=budget)
    msg = str(ei.value)
    assert "[rd error -4]" in msg and f"site {entries[big]['out_site']} " in msg and "1 site(s) not split" in msg
    got = _call(be, g, budget_bytes=budget, allow_too_large=True)
    for j in range(len(entries)):
        for f in ref.FIELDS:
            if j == big and f not in ("out_site", "n"):
                assert np.array_equal(getattr(got, f)[j], np.array(ref.TOO_LARGE if f == "status" else 0) * np.ones_like(want[f][j])), f
            else:
                assert np.array_equal(getattr(got, f)[j], want[f][j]), (j, f)


def test_site_split_refuses_bad_arguments_before_anything_is_launched(be):
    import ctypes
    from radian_amd.backend import SplitResult, _p
    site, cond, value = np.array([0, 1, 1], np.uint32), np.array([0, 1, 0], np.uint8), np.array([5, 6, 7], np.int16)

    def call(h, s, c, v, n_events, n_sites, budget, cap, mf=0):
        res, n_out = SplitResult(2), ctypes.c_int64(-9)
        rc = be._L.rd_site_split(h, s, c, v, n_events, n_sites, budget, cap, mf, *res._bufs(), ctypes.byref(n_out))
        return rc, n_out.value == -9 and all((getattr(res, f) == 0).all() for f in ref.FIELDS)

    assert call(be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 2) == (0, False)
    bad = cond.copy()
    bad[0] = 3
    for args in ((None, _p(site), _p(cond), _p(value), 3, 2, 0, 2), (be._h, None, _p(cond), _p(value), 3, 2, 0, 2),
                 (be._h, _p(site), None, _p(value), 3, 2, 0, 2), (be._h, _p(site), _p(cond), None, 3, 2, 0, 2),
                 (be._h, _p(site), _p(cond), _p(value), 2 ** 31, 2, 0, 2), (be._h, _p(site), _p(cond), _p(value), 3, 1, 0, 2),
                 (be._h, _p(site), _p(bad), _p(value), 3, 2, 0, 2), (be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 1),
                 (be._h, _p(site), _p(cond), _p(value), 3, 2, -1, 2), (be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 2, -1),
                 (be._h, _p(site), _p(cond), _p(value), 3, 2, 0, 2, 32769)):
        assert call(*args) == (-1, True), args[4:]
    rc, untouched = call(be._h, None, None, None, 0, 2, 0, 0)           # n_events == 0 is RD_OK with n_out = 0
    assert rc == 0 and not untouched


def test_sites_of_2_to_the_16_events_and_one_more(be):
    from radian_amd.backend import site_split_host
    g = sc.deep_group()
    want = ref.as_arrays(sc.reference("deep"))
    assert want["status"].tolist() == [ref.DEEP, ref.OK, ref.OK] and want["n"].sum(axis=1).tolist() == [2 ** 16 + 1, 2 ** 16, 2 ** 16]
    _equal(_call(be, g), want, "deep")
    _equal(site_split_host(g["site"], g["cond"], g["value"], g["n_sites"]), want, "deep, host")


def test_site_compare_is_unchanged_beside_the_split(be, groups):
    """rd_site_compare on the same events, before and after the split's calls on the same context, equals its own restatement
    (tests/_sitecmp_ref.py); its totals are the split's"""
    import _sitecmp_ref as cmp_ref
    for g in groups[:4] + groups[6:9]:
        want = cmp_ref.as_arrays(cmp_ref.compare(g["site"], g["cond"], g["value"]))
        before = be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"])
        split = _call(be, g)
        after = be.site_compare(g["site"], g["cond"], g["value"], g["n_sites"])
        for f in cmp_ref.FIELDS:
            assert np.array_equal(getattr(before, f), want[f]) and np.array_equal(getattr(after, f), want[f]), (g["name"], f)
        for f in ("out_site", "n", "sum", "sumsq"):
            assert np.array_equal(getattr(split, f), getattr(after, f)), (g["name"], f)


# ---------------------------------------------------------------------------------------------- the command
def test_command_end_to_end_on_two_simulated_samples(be, tmp_path):
    """tests/_sitesplit_e2e.py on the GPU: simulate (sample A with --modify at three sites and --mods-out, sample B without), eventalign
    --bounds truth.tsv, compare --split --reads-out under two budgets and twice under one.  The files are byte-identical across them and equal the
    tables the same formulas write from the restatements' integers; the three sites have level split_q <= 0.05; frac_hi_a and the
    per-read clusters meet the floors measured on the host twins (tests/test_sitesplit_cpu.py), each less one read per site."""
    from radian_amd.backend import site_split_workspace_bytes
    tight = site_split_workspace_bytes(600)                               # holds any site here (at most 2 * 64 events), and the events need many of it
    outs, dirs = e2e.run_chain(str(tmp_path), budgets=(0, tight, 0))
    assert outs[0] == outs[1] == outs[2]                                   # across the budgets, and across two runs at the same one
    sites, reads, text = outs[0]
    table, rows, st = e2e.expected_tables(dirs, str(tmp_path))
    assert sites.decode() == table and reads.decode() == rows
    n_events = sum(int(r.split("\t")[4]) + int(r.split("\t")[5]) for r in table.splitlines()[1:])
    assert n_events * 176 > 3 * tight
    rec = e2e.recovery(table, rows, open(tmp_path / "mods_a.tsv").read())
    print("split_q, reads of A, modified, frac_hi_a * reads, wrong calls, calls:", rec)
    for q, n_a, modified, above, wrong, calls in rec:
        assert q <= e2e.ALPHA
        assert abs(above - modified) <= e2e.FRAC_TOLERANCE_READS
        assert wrong <= e2e.WRONG_READS and calls >= n_a
    assert f"level split: {len(st['split']['level'])} sites with split_q <= 0.05 (thresholds not calibrated)" in text
    assert sorted(os.listdir(tmp_path / "events_a")) == ["sim_0000.events.tsv"]
