"""GPU checks of banded eventalign: rd_eventalign_banded against the restatement of its contract
(tests/_eventalign_banded_ref.py) on the seeded cases (tests/_eventalign_banded_cases.py; their defining conditions are asserted in
tests/test_eventalign_banded_cpu.py), the identity with rd_eventalign on the device, the budget, and `python -m radian_amd.eventalign
--events --refine` on a small `simulate` run.  Every output field is compared for EXACT equality.

Sizes follow the DP kernel: one wave per read, state s in lane s & 63, a window of 64 states, a back-pointer word per row stored 64 rows at
a time -- L + 2 on both sides of 64 and 128, and at the full DP's wave and band sizes, with T = L, L + 1, 2 L and 8 L + 5 rows (T on both
sides of a multiple of 64); guides on the path, 30 to 33 states off it to either side, constant, all before and all after the window, with
runs, with jumps of 63, 64 and 65 states in one row; T = 1, T < L, T = 2^19 at the value bound; every status beside unaffected neighbours."""
import os

import numpy as np
import pytest

import _eventalign_banded_cases as bc
import _eventalign_banded_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    gs = bc.groups()
    for _, cases in gs:
        for c in cases:
            bc.reference(c)
    return gs


@pytest.fixture(scope="module")
def whole(be, groups):
    return [be.eventalign_banded(model=bc.backend_model(m), **bc.call_args(cases)) for m, cases in groups]


def _need(cases):
    from radian_amd.backend import eventalign_banded_workspace_bytes
    return [eventalign_banded_workspace_bytes(c["t_hi"] - c["t_lo"], len(c["codes"])) for c in cases]


def _same(a, i, b, j, what="", edge=True):
    for f in ("status", "score", "m2", "d4") + (("n_edge",) if edge else ()):
        assert int(getattr(a, f)[i]) == int(getattr(b, f)[j]), (what, f)
    assert a.fit_sums[i].tolist() == b.fit_sums[j].tolist(), what
    assert a.first_step[i].tolist() == b.first_step[j].tolist() and a.last_step[i].tolist() == b.last_step[j].tolist(), what
    for f in ("start", "end", "sum", "sumsq", "min", "max"):
        assert getattr(a.events, f)[i].tolist() == getattr(b.events, f)[j].tolist(), (what, f)


def test_the_batches_equal_the_restatement(groups, whole):
    """every case of a model in one call: every status sits between reads that are aligned, and none of them is affected"""
    seen = set()
    for (m, cases), res in zip(groups, whole):
        for r, c in enumerate(cases):
            ref.assert_read_equal(res, r, bc.reference(c), c["name"])
        seen |= {int(s) for s in res.status}
    assert seen == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH, ref.OFF_BAND}


def test_one_read_per_call_and_reversed(be, groups, whole):
    for (m, cases), res in zip(groups, whole):
        bm = bc.backend_model(m)
        for r, c in enumerate(cases):
            if c["t_hi"] - c["t_lo"] <= 10000:
                _same(be.eventalign_banded(model=bm, **bc.call_args([c])), 0, res, r, c["name"])
        rev = be.eventalign_banded(model=bm, **bc.call_args(cases[::-1]))
        for r, c in enumerate(cases):
            _same(rev, len(cases) - 1 - r, res, r, c["name"])


def test_identity_with_eventalign_on_the_device(be, groups, whole):
    """every case whose full path meets the interior condition (the upper rim itself is inside): every output rd_eventalign has is equal"""
    (m, cases), res = groups[0], whole[0]
    assert m is bc.MODEL
    inside = [r for r, c in enumerate(cases) if bc.is_interior(c, bc.full_reference(c))]
    assert len(inside) >= 80
    few = [cases[r] for r in inside]
    full = be.eventalign(model=bc.backend_model(), **bc.full_args(few))
    for j, r in enumerate(inside):
        _same(res, r, full, j, cases[r]["name"], edge=False)


def test_budget_from_the_workspace_formula(be, groups, whole):
    """a budget of exactly the largest read's workspace: every read is aligned, over several launches; one byte less: that read alone is
    TOO_LARGE, the call names it with RD_ERR_NOMEM and the others are as before"""
    from radian_amd.backend import EVAL_TOO_LARGE, RadianHipError
    (m, cases), res0 = groups[0], whole[0]
    bm = bc.backend_model(m)
    need = [n if int(s) in (ref.OK, ref.OFF_BAND) else 0 for n, s in zip(_need(cases), res0.status)]      # (the others never reach a launch)
    big = int(np.argmax(need))
    assert sum(need) > 3 * need[big] and sorted(need)[-2] < need[big]
    res = be.eventalign_banded(model=bm, budget_bytes=need[big], **bc.call_args(cases))
    for r, c in enumerate(cases):
        _same(res, r, res0, r, c["name"])
    with pytest.raises(RadianHipError) as ei:
        be.eventalign_banded(model=bm, budget_bytes=need[big] - 1, **bc.call_args(cases))
    assert f"read {big} " in str(ei.value) and "1 read(s) not aligned" in str(ei.value)
    res = be.eventalign_banded(model=bm, budget_bytes=need[big] - 1, allow_too_large=True, **bc.call_args(cases))
    for r, c in enumerate(cases):
        if r != big:
            _same(res, r, res0, r, c["name"])
    L = len(cases[big]["codes"])
    assert int(res.status[big]) == EVAL_TOO_LARGE and res.score[big] == 0 and res.n_edge[big] == 0 and not res.fit_sums[big].any()
    assert (int(res.m2[big]), int(res.d4[big])) == (int(res0.m2[big]), int(res0.d4[big]))      # the scale is the read's own, whatever the budget
    assert res.first_step[big].tolist() == res.last_step[big].tolist() == res.events.start[big].tolist() == res.events.end[big].tolist() == [-1] * L
    assert not res.events.sum[big].any() and not res.events.sumsq[big].any() and not res.events.min[big].any() and not res.events.max[big].any()
    # a small budget: many launches, and every read over it is reported
    small = sorted(need)[len(need) // 2]
    res = be.eventalign_banded(model=bm, budget_bytes=small, allow_too_large=True, **bc.call_args(cases))
    for r, c in enumerate(cases):
        if need[r] <= small or int(res0.status[r]) not in (ref.OK, ref.OFF_BAND):
            _same(res, r, res0, r, c["name"])
        else:
            assert int(res.status[r]) == EVAL_TOO_LARGE


def test_refusals(be):
    from radian_amd.backend import EvalModel, RadianHipError
    m = bc.backend_model()
    raw, codes, guide = [np.arange(50, dtype=np.int16)], [np.array([0, 1, 2], dtype=np.uint8)], [np.array([3, 3, 9])]
    assert be.eventalign_banded(raw, codes, guide, m).status[0] == ref.OK
    assert be.eventalign_banded([], [], [], m).status.shape == (0,)
    for kw in (dict(guides=[np.array([3, 2, 9])]), dict(seqs=[np.array([0, 4, 1], dtype=np.uint8)]), dict(t_lo=[-1]), dict(t_lo=[10], t_hi=[9]),
               dict(t_hi=[51]), dict(d4=[-1]), dict(budget_bytes=-1)):
        with pytest.raises(RadianHipError):
            be.eventalign_banded(**{**dict(raws=raw, seqs=codes, guides=guide, model=m), **kw})
    lvl = m.lvl.copy()
    lvl[5] = 1 << 14
    with pytest.raises(RadianHipError):
        be.eventalign_banded(raw, codes, guide, EvalModel(m.k, lvl, m.w, m.bias, m.bg))


# ---------------------------------------------------------------------------------------------- the command
def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]


def test_command_on_a_simulated_run(be, tmp_path, capsys):
    """24 reads of `simulate`: with --events --refine every file is bit-identical across --batch-reads 1 / 7 / all and two budgets; the rows
    are the host composition's (rd_segment_host -> rd_eventalign_events_host under the same rounds -> rd_eventalign_banded_host on the refit,
    guided by the last round's event starts); a refined read with edge = 0 whose full path is interior has exactly the rows rd_eventalign_host
    gives on that scale; the summary gains refined and edge; `compare` reads the tables; --refine without --events is refused; runs without
    --refine are byte-identical before and after a --refine run."""
    from radian_amd import compare, eventalign, fast5, segment, simulate
    from radian_amd.backend import (SegmentParams, eventalign_banded_host, eventalign_banded_workspace_bytes, eventalign_events_host,
                                    eventalign_events_workspace_bytes, eventalign_host, segment_host, segment_max_events)
    from radian_amd.label_build import encode_reference, read_ref_tsv
    rng = np.random.default_rng(12)
    fa = tmp_path / "tr.fa"
    fa.write_text("".join(f">t{i}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, n))}\n" for i, n in enumerate((700, 1500, 420))))
    sim = tmp_path / "sim"
    simulate.main([str(fa), "-o", str(sim), "--reads", "24", "--seed", "3", "--length-median", "300", "--min-length", "200", "--tail", "60",
                   "--model-seed", "7", "--reads-per-file", "13"])
    capsys.readouterr()
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    for f in sorted(os.listdir(sim)):
        if f.endswith(".fast5"):
            os.rename(sim / f, in_dir / f)
    common = [str(in_dir), str(sim / "read_ref.tsv"), "--model-seed", "7", "--bounds", str(sim / "truth.tsv")]
    refs = read_ref_tsv(str(sim / "read_ref.tsv"))
    truth = {r[0]: (int(r[4]), int(r[8])) for r in _tsv(str(sim / "truth.tsv"))[1:]}
    need = max(max(eventalign_events_workspace_bytes(segment_max_events(n - max(0, e - 32), 4), len(refs[rid])),
                   eventalign_banded_workspace_bytes(n - max(0, e - 32), len(refs[rid]))) for rid, (n, e) in truth.items())

    def run(name, extra):
        d = tmp_path / name
        st = eventalign.main(common + ["-o", str(d), "--summary", str(d / "summary.tsv"), "--kmer-table-out", str(d / "kmers.tsv")] + extra)
        return st, capsys.readouterr().out, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}

    with pytest.raises(SystemExit):
        run("refused", ["--refine"])
    capsys.readouterr()
    events_before = run("ev0", ["--events"])[2]
    outs = {}
    for name, extra in (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                        ("all", ["--batch-reads", "24", "--budget-bytes", str(3 * need)])):
        st, text, outs[name] = run(name, ["--events", "--refine"] + extra)
        assert (st["reads"], st["written"], st["ok"], st["unbounded"]) == (24, 24, 24, 0) and "reads: 24 seen, 24 written" in text
        assert st["refined"] + st["not_refined"] == 24 and f"refined: {st['refined']}; not refined: {st['not_refined']}; with bases on the band's rim: {st['edge_reads']}" in text
        assert sorted(outs[name]) == ["kmers.tsv", "sim_0000.events.tsv", "sim_0001.events.tsv", "summary.tsv"]
    assert outs["b1"] == outs["b7"] == outs["all"]
    st, text, events_after = run("ev1", ["--events", "--batch-reads", "5"])
    assert events_before == events_after and "refined" not in text and events_after != outs["all"]
    assert events_after["summary.tsv"].split(b"\n")[0].split(b"\t")[-1] == b"skipped"
    # the host composition
    model, sd_m = eventalign.model_tables(5, *simulate.standin_tables(5, 7)[:2], 1.0)
    seg = segment.window_segmenter(segment_host, SegmentParams())
    rows = [r for f in ("sim_0000.events.tsv", "sim_0001.events.tsv") for r in _tsv(str(tmp_path / "all" / f))[1:]]
    summ = {r[0]: r for r in _tsv(str(tmp_path / "all" / "summary.tsv"))}
    assert summ["read_id"][-4:] == ["rows", "skipped", "refined", "edge"] and summ["read_id"][:-4] == list(eventalign.SUMMARY_COLUMNS)
    at = n_refined = n_identical = 0
    for f in ("sim_0000.fast5", "sim_0001.fast5"):
        for rd in fast5.iter_reads(str(in_dir / f)):
            rid, raw = rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16)
            codes = encode_reference(refs[rid])
            lo = max(0, truth[rid][1] - 32)
            be_align, cut = eventalign.events_aligner(seg, eventalign_events_host, 96)
            res = eventalign.align_rounds(be_align, [raw], [codes], model, [lo], 2)
            where, fine = eventalign.refine_pass(eventalign_banded_host, [raw], [codes], model, [lo], res)
            refined = int(fine.status[where[0]]) == ref.OK
            src = fine if refined else res
            want, _, _ = eventalign.read_rows(rid, "", refs[rid], raw, codes, src, 0, model, sd_m)
            mine = rows[at: at + len(want)]
            at += len(want)
            assert [m[:1] + m[2:] for m in mine] == [list(w[:1] + w[2:]) for w in want], rid
            assert summ[rid][1] == "ok" and (int(summ[rid][10]), int(summ[rid][11]), summ[rid][12]) == (int(src.m2[0]), int(src.d4[0]), "2")
            assert (int(summ[rid][13]), int(summ[rid][14])) == (int(cut["ev"].n_events[0]), int(res.n_skipped[0]))      # the event pass's
            assert (summ[rid][15], int(summ[rid][16])) == ("1" if refined else "0", int(fine.n_edge[0]) if refined else 0)
            if not refined:
                continue
            n_refined += 1
            assert len(want) == len(codes)                                      # every base has a row
            # the same scale through the full DP: where its path is interior the rows are the same
            full = eventalign_host([raw], [codes], model, t_lo=[lo], m2=[int(fine.m2[0])], d4=[int(fine.d4[0])])
            if int(fine.n_edge[0]) == 0 and ref.interior(full.first_step[0], full.last_step[0], len(codes), res.events.start[0], lo, len(raw) - lo):
                n_identical += 1
                wf, _, _ = eventalign.read_rows(rid, "", refs[rid], raw, codes, full, 0, model, sd_m)
                assert [list(w) for w in wf] == [list(w) for w in want] and int(full.score[0]) == int(fine.score[0]), rid
    assert at == len(rows) and n_refined >= 20 and n_identical >= 20
    # compare accepts the tables
    ev_dir = tmp_path / "events"
    ev_dir.mkdir()
    for f in ("sim_0000.events.tsv", "sim_0001.events.tsv"):
        (ev_dir / f).write_bytes(outs["all"][f])
    compare.main(["--a", str(ev_dir), "--a-paf", str(sim / "truth.paf"), "--b", str(ev_dir), "--b-paf", str(sim / "truth.paf"), "-o",
                  str(tmp_path / "sites.tsv"), "--min-depth", "2"])
    capsys.readouterr()
    assert len(_tsv(str(tmp_path / "sites.tsv"))) > 1
