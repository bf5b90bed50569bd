"""GPU checks of the pileup: rd_pileup_add and rd_pileup_add_ops == the restatement (tests/_pileup_ref.py, its ops
from tests/_align_ref.py's traceback) in every site channel, every profile counter and every per-pair field on the seeded cases of
tests/_pileup_cases.py; the tables under a budget that cuts the pairs into several launches and over several calls; a pair over the
budget; the bound on the pairs between open and close; rd_pileup_read at several depths and capacities; a sparse table of 10^6 sites;
open after close; the scores and ops against Backend.align; and python -m radian_amd.pileup end to end, byte for byte.  Every
comparison of integers is for equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _pileup_cases as pc
import _pileup_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in (pc.length_grid(), pc.ops_cases(), pc.hot(), pc.disjoint(), pc.sparse()):
        c = dict(c, given=c["ops"] is not None, scores=None)
        if not c["given"]:
            c["ops"], c["scores"] = ref.aligned(c["spans"], c["reads"])
        c["sites"], c["prof"], c["out"] = ref.pileup(c["ops"], c["spans"], c["reads"], c["site0"], c["n_sites"], c["scores"])
        out[c["name"]] = c
    return out


def _table(be, n_sites):
    """the whole site table and the profile through rd_pileup_read"""
    t = be.pileup_read(min_depth=1)
    sites = np.zeros((n_sites, 8), dtype=np.uint32)
    sites[t.site] = t.counts
    return sites, t.profile


def _assert_tables(be, c, what, times=1):
    sites, prof = _table(be, c["n_sites"])
    exp = c["sites"][:c["n_sites"]]
    covered = exp[:, :6].sum(axis=1) > 0          # (a site with only ins / starts counts always has an M / X or D count too)
    assert np.array_equal(sites, times * exp * covered[:, None]) and np.array_equal(covered[:, None] * exp, exp), what
    assert np.array_equal(prof, times * c["prof"]), what


@pytest.mark.parametrize("name", ["length_grid", "hot", "disjoint"])
def test_add_equals_the_restatement(be, cases, name):
    """aligned on the device: every per-pair field (the score among them), the ops, every site channel and profile counter"""
    c = cases[name]
    be.pileup_open(c["n_sites"])
    res = be.pileup_add(c["spans"], c["reads"], c["site0"], with_ops=True)
    assert res.ops == c["ops"]
    assert np.array_equal(res.out, c["out"])
    _assert_tables(be, c, name)
    be.pileup_close()


@pytest.mark.parametrize("name", ["length_grid", "ops_cases", "hot", "disjoint"])
def test_add_ops_equals_the_restatement(be, cases, name):
    """the same kernel on columns the caller gives: column strings no aligner produces among them"""
    c = cases[name]
    be.pileup_open(c["n_sites"])
    res = be.pileup_add_ops(c["ops"], c["spans"], c["reads"], c["site0"])
    exp = c["out"].copy()
    exp[:, 1] = 0                                  # no alignment ran: no score
    bad = [c.get("names", list(range(len(exp))))[k] for k in np.nonzero((res.out != exp).any(axis=1))[0]]
    assert not bad, bad
    _assert_tables(be, c, name)
    be.pileup_close()


def test_each_column_string_alone(be, cases):
    """one pair per open table: a failure names the column string"""
    c = cases["ops_cases"]
    for k, name in enumerate(c["names"]):
        one = [k]
        pick = lambda key: [c[key][i] for i in one]
        n_sites = c["n_sites"]
        sites, prof, out = ref.pileup(pick("ops"), pick("spans"), pick("reads"), pick("site0"), n_sites)
        be.pileup_open(n_sites)
        res = be.pileup_add_ops(pick("ops"), pick("spans"), pick("reads"), pick("site0"))
        assert np.array_equal(res.out, out), name
        _assert_tables(be, dict(n_sites=n_sites, sites=sites, prof=prof), name)
    be.pileup_close()


def test_tables_do_not_depend_on_launches_or_calls(be, cases):
    """a budget that cuts the pairs into >= 3 launches, and three add calls against one: identical tables and fields"""
    from radian_amd.backend import pileup_workspace_bytes
    c = cases["length_grid"]
    n = len(c["spans"])
    need = [pileup_workspace_bytes(len(s), len(r)) for s, r in zip(c["spans"], c["reads"])]
    staged = sum(need) - n * (1024 + 256)          # (the figure of a pair alone includes a launch's fixed part)
    budget = staged // 4
    assert budget >= max(need) and staged >= 3 * budget                               # no launch holds more than a third: at least 3 launches
    be.pileup_open(c["n_sites"])
    res = be.pileup_add(c["spans"], c["reads"], c["site0"], budget_bytes=budget, with_ops=True)
    assert np.array_equal(res.out, c["out"]) and res.ops == c["ops"]
    _assert_tables(be, c, "budget")
    cuts = [0, n // 3, 2 * n // 3 + 1, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = be.pileup_add(c["spans"][a:b], c["reads"][a:b], c["site0"][a:b])
        assert np.array_equal(part.out, c["out"][a:b])
    _assert_tables(be, c, "three calls on top of one", times=2)
    be.pileup_close()


def test_pair_over_the_budget(be, cases):
    from radian_amd import RadianHipError
    from radian_amd.backend import PILEUP_TOO_LARGE, pileup_workspace_bytes
    c = cases["length_grid"]
    keep = [p for p in range(len(c["spans"])) if len(c["spans"][p]) <= 129 and len(c["reads"][p]) <= 129][:40]
    big = next(p for p in range(len(c["spans"])) if len(c["spans"][p]) == 200 and len(c["reads"][p]) == 200)
    order = keep[:20] + [big] + keep[20:]
    pick = lambda key: [c[key][p] for p in order]
    budget = max(pileup_workspace_bytes(len(c["spans"][p]), len(c["reads"][p])) for p in keep)
    assert pileup_workspace_bytes(200, 200) > budget
    sites, prof, out = ref.pileup([c["ops"][p] for p in keep], [c["spans"][p] for p in keep], [c["reads"][p] for p in keep],
                                  [c["site0"][p] for p in keep], c["n_sites"], [c["scores"][p] for p in keep])
    be.pileup_open(c["n_sites"])
    with pytest.raises(RadianHipError) as ei:
        be.pileup_add(pick("spans"), pick("reads"), pick("site0"), budget_bytes=budget)
    assert "[rd error -4]" in str(ei.value) and "RD_PILEUP_TOO_LARGE" in str(ei.value) and "pair 20 (200 x 200)" in str(ei.value)
    _assert_tables(be, dict(n_sites=c["n_sites"], sites=sites, prof=prof), "the others were accumulated")
    be.pileup_open(c["n_sites"])
    res = be.pileup_add(pick("spans"), pick("reads"), pick("site0"), budget_bytes=budget, allow_too_large=True)
    assert res.status[20] == PILEUP_TOO_LARGE and not res.out[20, 1:].any()
    assert np.array_equal(np.delete(res.out, 20, axis=0), out)
    _assert_tables(be, dict(n_sites=c["n_sites"], sites=sites, prof=prof), "allow_too_large")
    be.pileup_close()


def test_pair_bound_and_refusals(be):
    """2^31 - 1 pairs between open and close: the bound is an argument check, made before any array is read"""
    from radian_amd import RadianHipError
    one = np.zeros(4, dtype=np.int64)
    buf = np.zeros(64, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    be.pileup_open(10)
    L, h = be._L, be._h
    be.pileup_add_ops([b"M"], [b"A"], [b"A"], [0])
    for call in (lambda: L.rd_pileup_add_ops(h, p(buf), p(one), p(buf), p(one), p(buf), p(one), 2 ** 31 - 1, p(one), p(buf)),
                 lambda: L.rd_pileup_add(h, p(buf), p(one), p(buf), p(one), 2 ** 31 - 1, p(one), 2, -4, -4, -2, 0, p(buf), None, None, None)):
        assert call() == -1 and "2^31 - 1" in L.rd_last_error().decode()
    t = be.pileup_read()
    assert t.site.tolist() == [0] and t.counts[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1]              # nothing was added by the refused calls
    for bad in (lambda: be.pileup_add_ops([b"MS"], [b"AC"], [b"AC"], [0]), lambda: be.pileup_add_ops([b"MM"], [b"AC"], [b"A"], [0]),
                lambda: be.pileup_add_ops([b"MM"], [b"AC"], [b"AC"], [9]), lambda: be.pileup_add([b"AC"], [b"AC"], [9]),
                lambda: be.pileup_add([b"AC"], [b"AC"], [-1]), lambda: be.pileup_read(min_depth=0)):
        with pytest.raises(RadianHipError):
            bad()
    assert be.pileup_read().counts[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    be.pileup_close()
    for closed in (lambda: be.pileup_add([b"AC"], [b"AC"], [0]), lambda: be.pileup_add_ops([b"MM"], [b"AC"], [b"AC"], [0]), lambda: be.pileup_read()):
        with pytest.raises(RadianHipError) as ei:
            closed()
        assert "rd_pileup_open" in str(ei.value)


def test_read_depths_and_capacities(be, cases):
    from radian_amd import RadianHipError
    c = cases["length_grid"]
    be.pileup_open(c["n_sites"])
    be.pileup_add_ops(c["ops"], c["spans"], c["reads"], c["site0"])
    be.pileup_add_ops(c["ops"][:60], c["spans"][:60], c["reads"][:60], c["site0"][:60])
    be.pileup_add_ops(c["ops"][:30], c["spans"][:30], c["reads"][:30], c["site0"][:30])
    s1, p1, _ = ref.pileup(c["ops"][:60], c["spans"][:60], c["reads"][:60], c["site0"][:60], c["n_sites"])
    s2, p2, _ = ref.pileup(c["ops"][:30], c["spans"][:30], c["reads"][:30], c["site0"][:30], c["n_sites"])
    sites, prof = c["sites"] + s1 + s2, c["prof"] + p1 + p2
    for depth in (1, 3):
        idx, rows = ref.table(sites[:c["n_sites"]], depth)
        assert 0 < len(idx) and (depth == 1 or len(idx) < len(ref.table(sites[:c["n_sites"]], 1)[0]))
        for cap in (len(idx), len(idx) + 100, None):
            t = be.pileup_read(min_depth=depth, capacity=cap)
            assert np.array_equal(t.site, idx) and np.array_equal(t.counts, rows) and np.array_equal(t.profile, prof), (depth, cap)
        with pytest.raises(RadianHipError) as ei:
            be.pileup_read(min_depth=depth, capacity=len(idx) - 1)
        assert f"{len(idx)} sites" in str(ei.value)
        n_out = ctypes.c_int64(-1)
        assert be._L.rd_pileup_read(be._h, depth, 0, None, None, None, ctypes.byref(n_out)) == -1 and n_out.value == len(idx)   # the needed count comes back
    be.pileup_close()


def test_sparse_table_and_open_after_close(be, cases):
    """10^6 sites, 50 covered: the read-out returns 50 rows; a second open and an open after close start from zero"""
    c = cases["sparse"]
    be.pileup_open(c["n_sites"])
    be.pileup_add_ops(c["ops"], c["spans"], c["reads"], c["site0"])
    t = be.pileup_read()
    idx, rows = ref.table(c["sites"], 1)
    assert len(t.site) == 50 and np.array_equal(t.site, idx) and np.array_equal(t.counts, rows) and np.array_equal(t.profile, c["prof"])
    be.pileup_open(c["n_sites"])
    t = be.pileup_read()
    assert len(t.site) == 0 and not t.profile.any()
    be.pileup_add_ops(c["ops"], c["spans"], c["reads"], c["site0"])
    be.pileup_close()
    be.pileup_open(100)
    t = be.pileup_read()
    assert len(t.site) == 0 and not t.profile.any()
    be.pileup_add_ops([b"MM"], [b"AC"], [b"AG"], [98])
    t = be.pileup_read()
    assert t.site.tolist() == [98, 99] and t.counts.tolist() == [[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0, 0, 0]]
    be.pileup_close()


def test_scores_and_ops_are_aligns(be, cases):
    """rd_pileup_add aligns exactly as rd_align_batch does: the same scores and ops on the same pairs, and align is as it was"""
    c = cases["length_grid"]
    a = be.align(c["spans"], c["reads"], with_ops=True)
    be.pileup_open(c["n_sites"])
    r = be.pileup_add(c["spans"], c["reads"], c["site0"], with_ops=True)
    be.pileup_close()
    assert np.array_equal(r.score, a.score) and r.ops == a.ops
    assert a.ops == c["ops"] and [int(s) for s in a.score] == c["scores"]


@pytest.mark.parametrize("sc", [(2, -3, -2, -2), (5, -4, -10, -1)], ids=["linear_2_-3_-2_-2", "affine_5_-4_-10_-1"])
def test_add_under_other_scores_equals_add_ops_of_the_restatements_ops(be, cases, sc):
    """rd_pileup_add hands its scores to the alignment: under linear gaps and under an expensive opening it leaves the site counts, the
    profile and the per-pair fields that rd_pileup_add_ops leaves when fed the restatement's ops for those scores, and returns those ops"""
    import _align_ref as ar
    for name in ("length_grid", "hot"):
        c = cases[name]
        score, _, ops = ar.align_cpu(c["spans"], c["reads"], sc)
        ops = [bytes(o) for o in ops]
        assert ops != c["ops"], name                                     # not the default scores' alignments
        be.pileup_open(c["n_sites"])
        exp = be.pileup_add_ops(ops, c["spans"], c["reads"], c["site0"])
        exp_sites, exp_prof = _table(be, c["n_sites"])
        be.pileup_open(c["n_sites"])
        res = be.pileup_add(c["spans"], c["reads"], c["site0"], scores=sc, with_ops=True)
        sites, prof = _table(be, c["n_sites"])
        be.pileup_close()
        assert res.ops == ops, name
        want = exp.out.copy()
        want[:, 1] = score                                               # rd_pileup_add_ops ran no alignment: its score column is 0
        assert np.array_equal(res.out, want), name
        assert np.array_equal(sites, exp_sites) and np.array_equal(prof, exp_prof), name
        assert exp_sites.any() and exp_prof.any()
        # and the restatement of the pileup itself on those ops
        r_sites, r_prof, r_out = ref.pileup(ops, c["spans"], c["reads"], c["site0"], c["n_sites"], [int(s) for s in score])
        assert np.array_equal(res.out, r_out) and np.array_equal(prof, r_prof), name


def test_add_refuses_gap_open_above_gap_extend_under_its_own_name(be):
    from radian_amd import RadianHipError
    one = np.zeros(4, dtype=np.int64)
    one[1] = 2
    seq = np.frombuffer(b"ACAC", dtype=np.uint8).copy()
    out = np.full(16, -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    be.pileup_open(10)
    be.pileup_add_ops([b"M"], [b"A"], [b"A"], [0])
    for sc in ((1, -2, -1, -3), (2, -4, -2, -4)):
        rc = be._L.rd_pileup_add(be._h, p(seq), p(one), p(seq), p(one), 1, p(one[2:]), *sc, 0, p(out), None, None, None)
        msg = be._L.rd_last_error().decode()
        assert rc == -1 and msg.startswith("rd_pileup_add: gap_open") and "gap_open <= gap_extend" in msg and "rd_align_batch" not in msg, (rc, msg)
        assert (out == -7).all()                                                                   # the refusal precedes every write to `out`
        with pytest.raises(RadianHipError, match="rd_pileup_add: gap_open"):
            be.pileup_add([b"AC"], [b"AC"], [0], scores=sc)
    assert be.pileup_read().counts.tolist() == [[1, 0, 0, 0, 0, 0, 0, 1]]                           # nothing was added by the refused calls
    be.pileup_add([b"AC"], [b"AC"], [0], scores=(2, -4, -3, -3))                                   # equality is legal
    assert be.pileup_read().site.tolist() == [0, 1]
    be.pileup_close()


# ---------------------------------------------------------------------------------------------- the command line
def test_command_line_files_byte_for_byte(tmp_path):
    names, seqs, reads, paf, alt = pc.cli_case()
    exp = ref.cli_files(names, seqs, reads, paf)
    (tmp_path / "tx.fa").write_text("".join(f">{n} description\n{s[:100]}\n{s[100:]}\n" for n, s in zip(names, seqs)))
    (tmp_path / "reads.fasta").write_text("".join(f">{n}\n{s}\n" for n, s in reads))
    (tmp_path / "map.paf").write_text("".join(l + "\n" for l in paf))

    def run(tag, *extra):
        d = tmp_path / tag
        d.mkdir()
        cmd = [sys.executable, "-m", "radian_amd.pileup", str(tmp_path / "reads.fasta"), str(tmp_path / "tx.fa"), "--paf", str(tmp_path / "map.paf"),
               "-o", str(d / "pileup.tsv"), "--variants", str(d / "variants.tsv"), "--profile", str(d / "profile.tsv"), "--sam", str(d / "out.sam"), *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return {k: (d / f).read_text() for k, f in (("tsv", "pileup.tsv"), ("variants", "variants.tsv"), ("profile", "profile.tsv"), ("sam", "out.sam"))}, r.stdout

    files, stdout = run("a")
    for k in ("tsv", "variants", "profile", "sam"):
        assert files[k] == exp[k], k
    assert f"reads seen {len(reads)}, piled up {len(reads) - 2}" in stdout and "not-in-paf 2" in stdout and "minus-strand 1" in stdout and "duplicate 1" in stdout
    subs = [l.split("\t") for l in files["variants"].splitlines()[1:] if l.split("\t")[3] == "sub"]
    assert [(r[0], int(r[1]), r[4]) for r in subs] == [(names[pc.PLANTED[0]], pc.PLANTED[1], alt)]
    from radian_amd.backend import pileup_workspace_bytes
    small = 4 * pileup_workspace_bytes(330, 340)
    again, _ = run("b", "--batch-reads", "7", "--budget-bytes", str(small))
    assert again == files
    full, _ = run("c", "--all-sites")
    assert full["tsv"] == ref.cli_files(names, seqs, reads, paf, all_sites=True)["tsv"] and full["profile"] == files["profile"]
