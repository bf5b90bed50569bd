"""GPU checks of eventalign: rd_eventalign against the restatement of its contract (tests/_eventalign_ref.py) on
the seeded cases (tests/_eventalign_cases.py; their defining conditions are asserted in tests/test_eventalign_cpu.py), and of
`python -m radian_amd.eventalign` on a small `simulate` run.  Every output field is compared for EXACT equality.

Sizes follow the DP kernel: a lane owns 16 states, a wave 1024, a workgroup pass (band) 4096 -- L + 2 on both sides of each, with T = L,
L + 1, 2 L and about 8 L rows; T = 1 and T < L; windows at either edge of the read and empty; a given scale and the window's own; samples at
the +-2^14 clamp and costs at the cap; ties; every status beside unaffected neighbours."""
import os

import numpy as np
import pytest

import _eventalign_cases as ec
import _eventalign_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    cs = ec.all_cases()
    for c in cs:
        ec.reference(c)
    return cs


@pytest.fixture(scope="module")
def whole(be, cases):
    return be.eventalign(model=ec.backend_model(), **ec.call_args(cases))


def _need(cases):
    from radian_amd.backend import eventalign_workspace_bytes
    return [eventalign_workspace_bytes(c["t_hi"] - c["t_lo"], len(c["codes"])) for c in cases]


def _same(a, i, b, j, what=""):
    for f in ("status", "score", "m2", "d4"):
        assert int(getattr(a, f)[i]) == int(getattr(b, f)[j]), (what, f)
    assert a.fit_sums[i].tolist() == b.fit_sums[j].tolist(), what
    assert a.first_step[i].tolist() == b.first_step[j].tolist() and a.last_step[i].tolist() == b.last_step[j].tolist(), what
    for f in ("start", "end", "sum", "sumsq", "min", "max"):
        assert getattr(a.events, f)[i].tolist() == getattr(b.events, f)[j].tolist(), (what, f)


def test_the_batch_equals_the_restatement(cases, whole):
    """every case in one call: every status sits between reads that are aligned, and none of them is affected"""
    for r, c in enumerate(cases):
        ref.assert_read_equal(whole, r, ec.reference(c), c["name"])
    assert {int(s) for s in whole.status} == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH}


def test_one_read_per_call_and_reversed(be, cases, whole):
    m = ec.backend_model()
    for r, c in enumerate(cases):
        if (c["t_hi"] - c["t_lo"]) * (len(c["codes"]) + 2) <= 5000000:
            _same(be.eventalign(model=m, **ec.call_args([c])), 0, whole, r, c["name"])
    rev = be.eventalign(model=m, **ec.call_args(cases[::-1]))
    for r, c in enumerate(cases):
        _same(rev, len(cases) - 1 - r, whole, r, c["name"])


def test_budget_from_the_workspace_formula(be, cases, whole):
    """a budget of exactly the largest read's workspace: every read is aligned, over several launches; one byte less: that read alone is
    TOO_LARGE, the call names it with RD_ERR_NOMEM and the others are as before"""
    from radian_amd.backend import EVAL_TOO_LARGE, RadianHipError
    m = ec.backend_model()
    need = _need(cases)
    big = int(np.argmax(need))
    assert sum(need) > 3 * need[big] and sorted(need)[-2] < need[big]
    res = be.eventalign(model=m, budget_bytes=need[big], **ec.call_args(cases))
    for r, c in enumerate(cases):
        _same(res, r, whole, r, c["name"])
    with pytest.raises(RadianHipError) as ei:
        be.eventalign(model=m, budget_bytes=need[big] - 1, **ec.call_args(cases))
    assert f"read {big} " in str(ei.value) and "1 read(s) not aligned" in str(ei.value)
    res = be.eventalign(model=m, budget_bytes=need[big] - 1, allow_too_large=True, **ec.call_args(cases))
    for r, c in enumerate(cases):
        if r != big:
            _same(res, r, whole, r, c["name"])
    L = len(cases[big]["codes"])
    assert int(res.status[big]) == EVAL_TOO_LARGE and res.score[big] == 0 and not res.fit_sums[big].any()
    assert (int(res.m2[big]), int(res.d4[big])) == (int(whole.m2[big]), int(whole.d4[big]))      # the scale is the read's own, whatever the budget
    assert res.first_step[big].tolist() == res.last_step[big].tolist() == res.events.start[big].tolist() == res.events.end[big].tolist() == [-1] * L
    assert not res.events.sum[big].any() and not res.events.sumsq[big].any() and not res.events.min[big].any() and not res.events.max[big].any()
    # a small budget: many launches, and every read over it is reported
    small = sorted(need)[len(need) // 2]
    res = be.eventalign(model=m, budget_bytes=small, allow_too_large=True, **ec.call_args(cases))
    for r, c in enumerate(cases):
        if need[r] <= small or int(whole.status[r]) != ref.OK:
            _same(res, r, whole, r, c["name"])
        else:
            assert int(res.status[r]) == EVAL_TOO_LARGE


def test_events_and_fit_sums_follow_from_the_steps(be, cases, whole):
    from radian_amd.backend import CtcAlignResult
    aln = CtcAlignResult(whole.first_step, whole.last_step, None, None, np.where(whole.status == ref.OK, 0, 1).astype(np.int32))
    ev = be.event_stats([c["raw"] for c in cases], aln)
    for f in ("start", "end", "sum", "sumsq", "min", "max"):
        for r in range(len(cases)):
            assert getattr(ev, f)[r].tolist() == getattr(whole.events, f)[r].tolist(), (cases[r]["name"], f)
    for r, c in enumerate(cases):
        if int(whole.status[r]) != ref.OK:
            assert not whole.fit_sums[r].any()
            continue
        l = np.array([ec.MODEL.lvl[ref.kmer(c["codes"], b, ec.K)] for b in range(len(c["codes"]))], dtype=np.int64)
        n, x = (whole.events.end[r] - whole.events.start[r]).astype(np.int64), whole.events.sum[r]
        assert whole.fit_sums[r].tolist() == [int(n.sum()), int((n * l).sum()), int((n * l * l).sum()), int(x.sum()), int((x * l).sum())]
        if len(l):
            assert whole.last_step[r][:-1].tolist() == (whole.first_step[r][1:] - 1).tolist()
            assert c["t_lo"] <= whole.first_step[r][0] and whole.last_step[r][-1] < c["t_hi"]


def test_refusals(be):
    from radian_amd.backend import EvalModel, RadianHipError
    m = ec.backend_model()
    raw, codes = [np.arange(50, dtype=np.int16)], [np.array([0, 1, 2], dtype=np.uint8)]
    assert be.eventalign(raw, codes, m).status[0] == ref.OK
    assert be.eventalign([], [], m).status.shape == (0,)
    for kw in (dict(seqs=[np.array([0, 4], dtype=np.uint8)]), dict(t_lo=[-1]), dict(t_lo=[10], t_hi=[9]), dict(t_hi=[51]), dict(d4=[-1]),
               dict(budget_bytes=-1)):
        with pytest.raises(RadianHipError):
            be.eventalign(**{**dict(raws=raw, seqs=codes, model=m), **kw})
    lvl = m.lvl.copy()
    lvl[5] = 1 << 14
    with pytest.raises(RadianHipError):
        be.eventalign(raw, codes, EvalModel(m.k, lvl, m.w, m.bias, m.bg))


# ---------------------------------------------------------------------------------------------- the command
def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]


def test_command_on_a_simulated_run(be, tmp_path, capsys):
    """24 reads of `simulate` (fragments of 200 bases and more, tails of 60 A, the stand-in of seed 7): every file is bit-identical across
    --batch-reads 1 / 7 / all and two budgets; the rows are the host composition's (rd_eventalign_host under the same rounds); with --bounds
    truth.tsv the first samples meet the accuracy floors of tests/test_eventalign_cpu.py against truth_moves.tsv; `compare` reads the tables."""
    from radian_amd import compare, eventalign, fast5, simulate
    from radian_amd.backend import eventalign_host, eventalign_workspace_bytes
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
    need = max(eventalign_workspace_bytes(n - max(0, e - 32), len(refs[rid])) for rid, (n, e) in truth.items())
    outs = {}
    for name, extra in (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                        ("all", ["--batch-reads", "24", "--budget-bytes", str(3 * need)])):
        d = tmp_path / name
        st = eventalign.main(common + ["-o", str(d), "--summary", str(d / "summary.tsv"), "--kmer-table-out", str(d / "kmers.tsv")] + extra)
        text = capsys.readouterr().out
        assert (st["reads"], st["written"], st["ok"], st["unbounded"]) == (24, 24, 24, 0) and "reads: 24 seen, 24 written" in text
        assert sorted(os.listdir(d)) == ["kmers.tsv", "sim_0000.events.tsv", "sim_0001.events.tsv", "summary.tsv"]
        outs[name] = {f: open(d / f, "rb").read() for f in os.listdir(d)}
    assert outs["b1"] == outs["b7"] == outs["all"]
    # the host composition: the same rounds over rd_eventalign_host
    model, sd_m = eventalign.model_tables(5, *simulate.standin_tables(5, 7)[:2], 1.0)
    rows = [r for f in ("sim_0000.events.tsv", "sim_0001.events.tsv") for r in _tsv(str(tmp_path / "all" / f))[1:]]
    moves = {r[0]: np.array(r[2].split(","), dtype=np.int64) for r in _tsv(str(sim / "truth_moves.tsv"))[1:]}
    summ = {r[0]: r for r in _tsv(str(tmp_path / "all" / "summary.tsv"))[1:]}
    at, tot, worst = 0, np.zeros(4, dtype=np.int64), 1.0
    for f in ("sim_0000.fast5", "sim_0001.fast5"):
        for rd in fast5.iter_reads(str(in_dir / f)):
            rid, raw = rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16)
            codes = encode_reference(refs[rid])
            lo = max(0, truth[rid][1] - 32)
            res = eventalign.align_rounds(lambda *a, **kw: eventalign_host(*a, **kw), [raw], [codes], model, [lo], 2)
            want, _, _ = eventalign.read_rows(rid, "", refs[rid], raw, codes, res, 0, model, sd_m)
            mine = rows[at: at + len(want)]
            at += len(want)
            assert [m[:1] + m[2:] for m in mine] == [list(w[:1] + w[2:]) for w in want], rid
            assert summ[rid][1] == "ok" and (int(summ[rid][10]), int(summ[rid][11]), summ[rid][12]) == (int(res.m2[0]), int(res.d4[0]), "2")
            assert abs(int(res.m2[0]) - 1200) <= 8 and abs(int(res.d4[0]) - 240) <= 6, (rid, res.m2[0], res.d4[0])
            # the rows are in written order 5'->3', as truth_moves.tsv's first samples are
            acc = ec.accuracy([int(m[4]) for m in mine], moves[rid])
            tot += acc[:4]
            worst = min(worst, acc[0] / acc[3])
            assert acc[0] / acc[3] >= 0.85, (rid, acc)
    assert at == len(rows)
    with capsys.disabled():
        print(f"\npooled within 10: {tot[0] / tot[3]:.3f}, within 30: {tot[1] / tot[3]:.3f}, exact: {tot[2] / tot[3]:.3f}; worst read within 10: {worst:.3f}")
    assert tot[0] / tot[3] >= 0.90 and tot[1] / tot[3] >= 0.96
    # compare accepts the tables
    ev_dir = tmp_path / "events"
    ev_dir.mkdir()
    for f in ("sim_0000.events.tsv", "sim_0001.events.tsv"):
        (ev_dir / f).write_bytes(outs["all"][f])
    compare.main(["--a", str(ev_dir), "--a-paf", str(sim / "truth.paf"), "--b", str(ev_dir), "--b-paf", str(sim / "truth.paf"), "-o",
                  str(tmp_path / "sites.tsv"), "--min-depth", "2"])
    capsys.readouterr()
    assert len(_tsv(str(tmp_path / "sites.tsv"))) > 1
