"""GPU checks of the poly(A) flat-segment search (rd_polya_segment / rd_polya_diag_windows, radian_amd/csrc/polya.hip) against the
plain-Python restatement of its contract (tests/_polya_ref.py) and against rd_polya_segment_host, and of `python -m radian_amd.polya`.
Everything is compared for EXACT equality.

Sizes follow the kernels (tests/_polya_cases.py; every case's defining condition is asserted in tests/test_polya_cpu.py): a workgroup of
the window kernel takes 64 windows and the segment kernel sweeps 256 windows per chunk -- reads of 63, 64, 65, 255, 256, 257 and 5003
windows, segments over a chunk boundary, window lengths 8, 16 and 256 (lane groups of 8, 16 and 64) here and 32 (the command's default)
in the synthetic tails, one read of 1 000 000 samples (31 250 windows: 489 workgroups, 123 chunks)."""
import os
import shutil

import numpy as np
import pytest

import _polya_cases as pc
import _polya_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    gs = pc.all_groups()
    for g in gs:
        g["exp"] = [ref.segment(x, g["p"]) for x in g["reads"]]
    return gs


def _params(p):
    from radian_amd.backend import PolyaParams
    return PolyaParams(**p)


def test_diag_windows_equal_the_restatement(be, groups):
    for g in groups:
        m2, d4, thr, wins = be.polya_diag_windows(g["reads"], _params(g["p"]))
        for r, x in enumerate(g["reads"]):
            if len(x) == 0:
                assert (int(m2[r]), int(d4[r]), int(thr[r])) == (0, 0, 0) and len(wins[r][0]) == 0, (g["name"], r)
                continue
            e_m2, e_d4, e_thr, e_wins = ref.windows(x, g["p"])
            assert (int(m2[r]), int(d4[r]), int(thr[r])) == (e_m2, e_d4, e_thr), (g["name"], r)
            S, Q, F = wins[r]
            assert S.dtype == np.int32 and Q.dtype == np.int64 and F.dtype == np.uint8
            assert S.tolist() == [w[0] for w in e_wins] and Q.tolist() == [w[1] for w in e_wins] and F.tolist() == [w[2] for w in e_wins], (g["name"], r)


def test_segment_equals_the_restatement(be, groups):
    for g in groups:
        got = be.polya_segment(g["reads"], _params(g["p"]))
        for r in range(len(g["reads"])):
            pc.same(got, r, g["exp"][r])
    shapes = groups[0]
    st = [e["status"] for e in shapes["exp"]]
    assert {ref.OK, ref.EMPTY, ref.SHORT, ref.MAD_ZERO} <= set(st)


def test_segment_does_not_depend_on_the_grouping_and_equals_the_host(be, groups):
    from radian_amd.backend import POLYA_FIELDS, polya_segment_host, polya_workspace_bytes
    g = groups[0]
    reads, p, n = g["reads"], _params(g["p"]), len(g["reads"])
    whole = be.polya_segment(reads, p)
    host = polya_segment_host(reads, p)
    rev = be.polya_segment(reads[::-1], p)
    # a budget that holds the largest read and little more: several launches
    need = [polya_workspace_bytes(len(x), p.win) for x in reads]
    big = int(np.argmax(need))
    budget = need[big] + 4096
    assert 0 < big < n - 1 and sum(need[:big + 1]) > budget and need[big] + need[big + 1] > budget     # at least three launches
    cut = be.polya_segment(reads, p, budget_bytes=budget)
    for name in POLYA_FIELDS:
        a = getattr(whole, name)
        assert a.dtype == getattr(host, name).dtype and np.array_equal(a, getattr(host, name)), name
        assert np.array_equal(a, getattr(rev, name)[::-1]), name
        assert np.array_equal(a, getattr(cut, name)), name
    for r in range(n):
        one = be.polya_segment([reads[r]], p)
        for name in POLYA_FIELDS:
            assert getattr(one, name)[0] == getattr(whole, name)[r], (name, r)


def test_a_budget_that_excludes_exactly_one_read(be, groups):
    from radian_amd import RadianHipError
    from radian_amd.backend import POLYA_FIELDS, POLYA_TOO_LARGE, polya_workspace_bytes
    g = groups[0]
    reads, p = g["reads"], _params(g["p"])
    need = [polya_workspace_bytes(len(x), p.win) for x in reads]
    big = int(np.argmax(need))
    budget = need[big] - 1
    assert sorted(need)[-2] <= budget
    with pytest.raises(RadianHipError) as ei:
        be.polya_segment(reads, p, budget_bytes=budget)
    assert f"read {big} " in str(ei.value) and "1 read(s) not segmented" in str(ei.value)
    got = be.polya_segment(reads, p, budget_bytes=budget, allow_too_large=True)
    for r in range(len(reads)):
        if r == big:
            assert got.status[r] == POLYA_TOO_LARGE and (got.tail_start[r], got.tail_end[r]) == (-1, -1)
            assert all(getattr(got, f)[r] == 0 for f in POLYA_FIELDS if f not in ("status", "tail_start", "tail_end"))
        else:
            pc.same(got, r, g["exp"][r])


def test_segment_refuses_bad_arguments_before_anything_is_launched(be):
    good, bad = pc.refusal_cases()
    fn = lambda *a: be._L.rd_polya_segment(be._h, *a)
    assert pc.raw_call(fn, budget=0, **good) == 0
    for name, kw in bad:
        outs = [np.full(2, 77, dtype=np.int64 if f in ("tail_start", "tail_end", "sum", "sumsq") else np.int32) for f in ref.FIELDS]
        assert pc.raw_call(fn, outs=outs, budget=0, **kw) == -1, name   # RD_ERR_ARG
        assert all((o == 77).all() for o in outs), name
    assert pc.raw_call(fn, budget=-1, **good) == -1
    assert pc.raw_call(lambda *a: be._L.rd_polya_segment(None, *a), budget=0, **good) == -1   # a null context
    assert pc.raw_call(fn, raw=None, off=None, p=good["p"], n_reads=0, budget=0) == 0        # n_reads == 0 is RD_OK


def test_a_read_of_a_million_samples(be):
    from radian_amd import synthetic
    from radian_amd.backend import PolyaParams, polya_segment_host
    x, (a, e) = synthetic.tail_read(np.random.default_rng(5), leader=3000, adapter=5000, tail=20000, body=972000)
    assert len(x) == 1000000
    p = PolyaParams()
    exp = ref.segment(x, dict(zip(ref.PARAMS, p.args())))
    got = be.polya_segment([x], p)
    pc.same(got, 0, exp)
    pc.same(polya_segment_host([x], p), 0, exp)
    assert exp["status"] == ref.OK and abs(exp["tail_start"] - a) < 32 and abs(exp["tail_end"] - e) < 32


def _run_cli(argv, capsys):
    from radian_amd import polya
    polya.main(argv)
    return capsys.readouterr().out


def test_command_on_the_golden_reads_and_on_synthetic_tails(be, tmp_path, capsys):
    """byte-identical TSVs for --batch-reads 1 and 5 (and a small budget); the synthetic tails are found within a window of the truth"""
    from radian_amd import fast5, synthetic
    gold = tmp_path / "gold"
    gold.mkdir()
    shutil.copy(os.path.join(GOLDEN, "reads.fast5"), str(gold / "reads.fast5"))
    outs = {}
    for b in (1, 5):
        text = _run_cli([str(gold), "-o", str(tmp_path / f"gold{b}.tsv"), "--batch-reads", str(b)], capsys)
        outs[b] = open(str(tmp_path / f"gold{b}.tsv"), "rb").read()
        assert "reads: 5 seen" in text
    assert outs[1] == outs[5]
    rows = [ln.split("\t") for ln in outs[1].decode().splitlines()]
    assert len(rows) == 6 and rows[0][:3] == ["read_id", "status", "n_samples"] and all(len(r) == 11 for r in rows)
    assert [r[0] for r in rows[1:]] == [r.read_id for r in fast5.iter_reads(os.path.join(GOLDEN, "reads.fast5"))]
    # synthetic tails
    syn = tmp_path / "syn"
    syn.mkdir()
    rng = np.random.default_rng(77)
    reads, truth = {}, {}
    for i in range(7):
        x, t = synthetic.tail_read(rng, leader=int(rng.integers(0, 500)), adapter=int(rng.integers(300, 700)), tail=int(rng.integers(600, 2500)),
                                   body=int(rng.integers(6000, 9000)))
        reads[f"{i:08d}-syn"], truth[f"{i:08d}-syn"] = x, t
        flags = [w[2] for w in ref.windows(x, ref.params(win=32, flat_q=46))[3]]      # the premise of the bound (tests/test_polya_cpu.py)
        assert all(f == (j * 32 >= t[0] and (j + 1) * 32 <= t[1]) for j, f in enumerate(flags) if (j + 1) * 32 <= t[0] or j * 32 >= t[0] and (j + 1) * 32 <= t[1] or j * 32 >= t[1])
    fast5.write_multi_fast5(str(syn / "tails.fast5"), reads)
    outs = {}
    for b, extra in ((1, []), (5, []), (3, ["--budget-bytes", "40000"])):
        _run_cli([str(syn), "-o", str(tmp_path / f"syn{b}.tsv"), "--batch-reads", str(b), "--samples-per-base", "12.5"] + extra, capsys)
        outs[b] = open(str(tmp_path / f"syn{b}.tsv"), "rb").read()
    assert outs[1] == outs[5] == outs[3]
    rows = [ln.split("\t") for ln in outs[1].decode().splitlines()][1:]
    assert len(rows) == 7
    for r in rows:
        a, e = truth[r[0]]
        assert r[1] == "ok" and abs(int(r[3]) - a) < 32 and abs(int(r[4]) - e) < 32, r
        assert r[5] == str(int(r[4]) - int(r[3])) and r[8] == "12.5000" and r[9] == f"{(int(r[4]) - int(r[3])) / 12.5:.2f}"
