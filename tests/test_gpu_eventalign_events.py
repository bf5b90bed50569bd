"""GPU checks of eventalign on event rows: rd_eventalign_events against the restatement of its contract
(tests/_eventalign_events_ref.py) on the seeded cases (tests/_eventalign_events_cases.py; their defining conditions are asserted in
tests/test_eventalign_events_cpu.py), against rd_eventalign when every sample is an event and skips are off, and of
`python -m radian_amd.eventalign --events` on a small `simulate` run.  Every output field is compared for EXACT equality.

Sizes follow the DP kernel: a lane owns 16 states (one back-pointer word), a wave 1024, a workgroup pass (band) 4096 -- L + 2 on both
sides of each and in a third band, with E = ceil((L + 1) / 2) (every transition a skip), one more, L and 2 L + 3 rows; both parities of
the all-skip path; states 16, 17, 1024, 1025, 4096 and 4097 entered by a skip and by an advance; E = 1; one row short of a path; ties;
penalties -1, 0 and 256; the value bound; n_e = 1; means at the clamp; every status beside unaffected neighbours."""
import os

import numpy as np
import pytest

import _eventalign_cases as sc
import _eventalign_events_cases as ec
import _eventalign_events_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    gs = ec.groups()
    for _, _, cs in gs:
        for c in cs:
            ec.reference(c)
    return gs


@pytest.fixture(scope="module")
def whole(be, groups):
    return [be.eventalign_events(model=ec.backend_model(m), skip_pen=pen, **ec.call_args(cs)) for m, pen, cs in groups]


def _need(cases):
    from radian_amd.backend import eventalign_events_workspace_bytes
    return [eventalign_events_workspace_bytes(len(c["ev"]["start"]), len(c["codes"])) for c in cases]


def _same(a, i, b, j, what=""):
    for f in ("status", "score", "n_skipped"):
        assert int(getattr(a, f)[i]) == int(getattr(b, f)[j]), (what, f)
    assert a.fit_sums[i].tolist() == b.fit_sums[j].tolist(), what
    assert a.row_first[i].tolist() == b.row_first[j].tolist() and a.row_last[i].tolist() == b.row_last[j].tolist(), what
    for f in ("start", "end", "sum", "sumsq", "min", "max"):
        assert getattr(a.events, f)[i].tolist() == getattr(b.events, f)[j].tolist(), (what, f)


def test_the_batches_equal_the_restatement(groups, whole):
    """every case of a (model, penalty) in one call: every status sits between reads that are aligned, and none of them is affected"""
    seen = set()
    for (_, _, cases), res in zip(groups, whole):
        for r, c in enumerate(cases):
            ref.assert_read_equal(res, r, ec.reference(c), c["name"])
        seen |= {int(s) for s in res.status}
    assert seen == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH}


def test_one_read_per_call_and_reversed(be, groups, whole):
    for (model, pen, cases), res in zip(groups, whole):
        m = ec.backend_model(model)
        for r, c in enumerate(cases):
            if len(c["ev"]["start"]) * (len(c["codes"]) + 2) <= 5000000:
                _same(be.eventalign_events(model=m, skip_pen=pen, **ec.call_args([c])), 0, res, r, c["name"])
        rev = be.eventalign_events(model=m, skip_pen=pen, **ec.call_args(cases[::-1]))
        for r, c in enumerate(cases):
            _same(rev, len(cases) - 1 - r, res, r, c["name"])


def test_one_event_per_sample_without_skips_is_eventalign(be):
    """the cases of tests/_eventalign_cases.py with a sample or more, every sample an event, on the scale rd_eventalign reports: the same
    scores, steps, events and sums on the device"""
    cases = [c for c in sc.all_cases() if c["t_hi"] - c["t_lo"] >= 1]
    want = be.eventalign(model=sc.backend_model(), **sc.call_args(cases))
    got = be.eventalign_events([ec.sample_events(c) for c in cases], [c["t_hi"] - c["t_lo"] for c in cases], [c["codes"] for c in cases],
                               sc.backend_model(), want.m2, want.d4, sample_off=[c["t_lo"] for c in cases], skip_pen=-1)
    ec.assert_identity(got, want, cases)


def test_budget_from_the_workspace_formula(be, groups, whole):
    """a budget of exactly the largest read's workspace: every read is aligned, over several launches; one byte less: that read alone is
    TOO_LARGE, the call names it with RD_ERR_NOMEM and the others are as before"""
    from radian_amd.backend import EVAL_TOO_LARGE, RadianHipError
    (model, pen, cases), res0 = max(zip(groups, whole), key=lambda g: len(g[0][2]))
    m = ec.backend_model(model)
    need = _need(cases)
    big = int(np.argmax(need))
    assert sum(need) > 2 * need[big] and sorted(need)[-2] < need[big]      # three launches or more; one read is the largest
    res = be.eventalign_events(model=m, skip_pen=pen, budget_bytes=need[big], **ec.call_args(cases))
    for r, c in enumerate(cases):
        _same(res, r, res0, r, c["name"])
    with pytest.raises(RadianHipError) as ei:
        be.eventalign_events(model=m, skip_pen=pen, budget_bytes=need[big] - 1, **ec.call_args(cases))
    assert f"read {big} " in str(ei.value) and "1 read(s) not aligned" in str(ei.value)
    res = be.eventalign_events(model=m, skip_pen=pen, budget_bytes=need[big] - 1, allow_too_large=True, **ec.call_args(cases))
    for r, c in enumerate(cases):
        if r != big:
            _same(res, r, res0, r, c["name"])
    L = len(cases[big]["codes"])
    assert int(res.status[big]) == EVAL_TOO_LARGE and res.score[big] == 0 and res.n_skipped[big] == 0 and not res.fit_sums[big].any()
    assert res.row_first[big].tolist() == res.row_last[big].tolist() == res.events.start[big].tolist() == res.events.end[big].tolist() == [-1] * L
    assert not res.events.sum[big].any() and not res.events.sumsq[big].any() and not res.events.min[big].any() and not res.events.max[big].any()
    # a small budget: many launches, and every read over it is reported
    small = sorted(need)[len(need) // 2]
    res = be.eventalign_events(model=m, skip_pen=pen, budget_bytes=small, allow_too_large=True, **ec.call_args(cases))
    for r, c in enumerate(cases):
        if need[r] <= small or int(res0.status[r]) != ref.OK:
            _same(res, r, res0, r, c["name"])
        else:
            assert int(res.status[r]) == EVAL_TOO_LARGE


def test_refusals(be):
    from radian_amd.backend import RadianHipError
    m = ec.backend_model()
    good = dict(events=[ref.events_of(np.arange(600, 650), [0, 10, 30])], n_samples=[50], seqs=[np.array([0, 1, 2], dtype=np.uint8)], m2=[1200],
                d4=[240], model=m)
    assert be.eventalign_events(**good).status[0] == ref.OK
    assert be.eventalign_events([], [], [], m, [], []).status.shape == (0,)
    for kw in (dict(seqs=[np.array([0, 4], dtype=np.uint8)]), dict(d4=[-1]), dict(skip_pen=-2), dict(skip_pen=257), dict(n_samples=[30]),
               dict(sample_off=[-1]), dict(budget_bytes=-1)):
        with pytest.raises(RadianHipError):
            be.eventalign_events(**{**good, **kw})


# ---------------------------------------------------------------------------------------------- the command
def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]


def test_command_on_a_simulated_run(be, tmp_path, capsys):
    """24 reads of `simulate`: with --events every file is bit-identical across --batch-reads 1 / 7 / all and two budgets; the rows are the
    host composition's (rd_segment_host -> rd_eventalign_events_host under the same rounds), a skipped base writing none; the summary gains
    rows and skipped; `compare` reads the tables; without --events the files are what the sample-row host composition gives, byte for byte
    whether or not an --events run came before."""
    from radian_amd import compare, eventalign, fast5, segment, simulate
    from radian_amd.backend import SegmentParams, eventalign_events_host, eventalign_events_workspace_bytes, segment_host, segment_max_events
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
    need = max(eventalign_events_workspace_bytes(segment_max_events(n - max(0, e - 32), 4), len(refs[rid])) for rid, (n, e) in truth.items())

    def run(name, extra):
        d = tmp_path / name
        st = eventalign.main(common + ["-o", str(d), "--summary", str(d / "summary.tsv"), "--kmer-table-out", str(d / "kmers.tsv")] + extra)
        return st, capsys.readouterr().out, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}

    plain_before = run("plain0", [])[2]
    outs = {}
    for name, extra in (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                        ("all", ["--batch-reads", "24", "--budget-bytes", str(3 * need)])):
        st, text, outs[name] = run(name, ["--events"] + extra)
        assert (st["reads"], st["written"], st["ok"], st["unbounded"]) == (24, 24, 24, 0) and "reads: 24 seen, 24 written" in text
        assert "events per base: " in text and "bases skipped: " in text
        assert sorted(outs[name]) == ["kmers.tsv", "sim_0000.events.tsv", "sim_0001.events.tsv", "summary.tsv"]
    assert outs["b1"] == outs["b7"] == outs["all"]
    st, text, plain_after = run("plain1", ["--batch-reads", "5"])
    assert plain_before == plain_after and "events per base" not in text and plain_after != outs["all"]
    assert plain_after["summary.tsv"].split(b"\n")[0].split(b"\t")[-1] == b"rounds"
    # the host composition: rd_segment_host on the window as its own scale window, then the same rounds over rd_eventalign_events_host
    model, sd_m = eventalign.model_tables(5, *simulate.standin_tables(5, 7)[:2], 1.0)
    seg = segment.window_segmenter(segment_host, SegmentParams())
    rows = [r for f in ("sim_0000.events.tsv", "sim_0001.events.tsv") for r in _tsv(str(tmp_path / "all" / f))[1:]]
    summ = {r[0]: r for r in _tsv(str(tmp_path / "all" / "summary.tsv"))}
    assert summ["read_id"][-2:] == ["rows", "skipped"] and summ["read_id"][:-2] == list(eventalign.SUMMARY_COLUMNS)
    at = skipped = bases = 0
    for f in ("sim_0000.fast5", "sim_0001.fast5"):
        for rd in fast5.iter_reads(str(in_dir / f)):
            rid, raw = rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16)
            codes = encode_reference(refs[rid])
            lo = max(0, truth[rid][1] - 32)
            be_align, cut = eventalign.events_aligner(seg, eventalign_events_host, 96)
            res = eventalign.align_rounds(be_align, [raw], [codes], model, [lo], 2)
            want, _, _ = eventalign.read_rows(rid, "", refs[rid], raw, codes, res, 0, model, sd_m)
            assert len(want) == len(codes) - int(res.n_skipped[0])                 # a skipped base writes no row
            mine = rows[at: at + len(want)]
            at += len(want)
            assert [m[:1] + m[2:] for m in mine] == [list(w[:1] + w[2:]) for w in want], rid
            assert summ[rid][1] == "ok" and (int(summ[rid][10]), int(summ[rid][11]), summ[rid][12]) == (int(res.m2[0]), int(res.d4[0]), "2")
            assert (int(summ[rid][13]), int(summ[rid][14])) == (int(cut["ev"].n_events[0]), int(res.n_skipped[0]))
            skipped += int(res.n_skipped[0])
            bases += len(codes)
    assert at == len(rows) and 0 < skipped < bases // 4
    # the k-mer table counts the rows that were written and no skipped base: with k = 5 the two bases at either end of a span have no k-mer
    kt = _tsv(str(tmp_path / "all" / "kmers.tsv"))[1:]
    pos = {}
    for r in rows:
        pos.setdefault(r[0], set()).add(int(r[2]))
    assert sum(int(r[1]) for r in kt) == sum(len([p for p in ps if 2 <= p < len(refs[rid]) - 2]) for rid, ps in pos.items())
    # compare accepts the tables
    ev_dir = tmp_path / "events"
    ev_dir.mkdir()
    for f in ("sim_0000.events.tsv", "sim_0001.events.tsv"):
        (ev_dir / f).write_bytes(outs["all"][f])
    compare.main(["--a", str(ev_dir), "--a-paf", str(sim / "truth.paf"), "--b", str(ev_dir), "--b-paf", str(sim / "truth.paf"), "-o",
                  str(tmp_path / "sites.tsv"), "--min-depth", "2"])
    capsys.readouterr()
    assert len(_tsv(str(tmp_path / "sites.tsv"))) > 1
