"""GPU checks of event detection (rd_segment / rd_segment_diag_tstat, radian_amd/csrc/segment.hip) against the restatements of its
contract (tests/_segment_ref.py: plain Python for the short reads, the NumPy twin for the long ones; tests/test_segment_cpu.py holds the
two equal on every case) and of `python -m radian_amd.segment`.  Everything is compared for EXACT equality.

Sizes follow the kernels (tests/_segment_cases.py; every case's defining condition is asserted in tests/test_segment_cpu.py): the peak
kernel takes tiles of 2048 samples and recomputes a halo of two windows -- reads of 2047, 2048, 2049, 4095 and 4097 samples, steps on a
tile's first and last sample and at every distance the halo reaches; the event kernel takes runs of 64 events -- reads of one event, of
fewer than 64 and of several hundred."""
import os

import numpy as np
import pytest

import _segment_cases as sc
import _segment_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def _expected(x, p):
    return ref.segment(x, p) if len(x) < 1000 else ref.segment_np(x, p)


@pytest.fixture(scope="module")
def groups():
    gs = sc.all_groups()
    for g in gs:
        g["exp"] = [_expected(x, g["p"]) for x in g["reads"]]
    return gs


def _params(p):
    from radian_amd.backend import SegmentParams
    return SegmentParams(**p)


def _same_result(a, b, ra, rb):
    assert (int(a.status[ra]), int(a.n_events[ra]), int(a.m2[ra]), int(a.d4[ra])) == (int(b.status[rb]), int(b.n_events[rb]), int(b.m2[rb]), int(b.d4[rb]))
    for f in ref.EVENT_FIELDS:
        assert a.events[ra][f].dtype == b.events[rb][f].dtype and np.array_equal(a.events[ra][f], b.events[rb][f]), f


def test_every_field_of_every_case_equals_the_restatement(be, groups):
    for g in groups:
        got = be.segment(g["reads"], _params(g["p"]))
        for r in range(len(g["reads"])):
            sc.same(got, r, g["exp"][r])
    n_ev = [e["n_events"] for e in groups[0]["exp"]]
    assert 0 in n_ev and 1 in n_ev and any(1 < n < 64 for n in n_ev) and any(n > 128 for n in n_ev)     # the event kernel's runs


def test_one_batch_one_read_per_call_reversed_and_the_host_agree(be, groups):
    from radian_amd.backend import segment_host
    for g in groups[:2]:
        reads, p, n = g["reads"], _params(g["p"]), len(g["reads"])
        wins = [(len(x) // 3, len(x)) for x in reads]
        whole = be.segment(reads, p, wins)
        host = segment_host(reads, p, wins)
        rev = be.segment(reads[::-1], p, wins[::-1])
        for r in range(n):
            _same_result(whole, host, r, r)
            _same_result(whole, rev, r, n - 1 - r)
            _same_result(whole, be.segment([reads[r]], p, [wins[r]]), r, 0)
            if len(reads[r]) - len(reads[r]) // 3 > 0:
                assert (int(whole.m2[r]), int(whole.d4[r])) == ref.scale(reads[r][wins[r][0]:wins[r][1]])
        assert any(d > 0 for d in whole.d4)


def test_diag_tstat_equals_the_restatement_stage_by_stage(be, groups):
    for g in groups:
        p = g["p"]
        got = be.segment_diag_tstat(g["reads"], _params(p))
        for r, x in enumerate(g["reads"]):
            N, D, F = got[r]
            assert N.shape == (2, len(x)) and N.dtype == np.uint64 and F.dtype == np.uint8
            bits = np.zeros(len(x), np.uint8)
            for d, (w, th) in enumerate(((p["w1"], p["th1"]), (p["w2"], p["th2"]))):
                eN, eD = ref.tstat_np(x, w, p["v0"])
                assert np.array_equal(N[d].astype(np.int64), eN) and np.array_equal(D[d].astype(np.int64), eD), (g["name"], r, d)
                bits |= (ref.peaks_np(eN, eD, w, th).astype(np.uint8) << d)
            assert np.array_equal(F, bits), (g["name"], r)


def test_a_budget_of_exactly_the_largest_read_and_one_byte_less(be, groups):
    from radian_amd import RadianHipError
    from radian_amd.backend import SEGMENT_TOO_LARGE, segment_workspace_bytes
    g = groups[0]
    reads, p = g["reads"], _params(g["p"])
    need = [segment_workspace_bytes(len(x), p.w1) for x in reads]
    big = int(np.argmax(need))
    assert sorted(need)[-2] < need[big] and sum(need) > 3 * need[big]      # one read is excluded, and the others take several launches
    got = be.segment(reads, p, budget_bytes=need[big])
    for r in range(len(reads)):
        sc.same(got, r, g["exp"][r])
    with pytest.raises(RadianHipError) as ei:
        be.segment(reads, p, budget_bytes=need[big] - 1)
    assert f"read {big} " in str(ei.value) and "1 read(s) not segmented" in str(ei.value)
    got = be.segment(reads, p, budget_bytes=need[big] - 1, allow_too_large=True)
    for r in range(len(reads)):
        if r == big:
            assert got.status[r] == SEGMENT_TOO_LARGE and got.n_events[r] == 0
        else:
            sc.same(got, r, g["exp"][r])


def test_refusals_write_nothing_and_a_read_past_2_30_samples_is_never_read(be):
    good, bad = sc.refusal_cases()
    fn = lambda *a: be._L.rd_segment(be._h, *a)
    assert sc.raw_call(fn, budget=0, **good)[0] == 0
    for name, kw in bad:
        rc, outs = sc.raw_call(fn, budget=0, fill=77, **kw)
        assert rc == -1, name   # RD_ERR_ARG
        assert all((o == 77).all() for o in outs), name
    assert sc.raw_call(fn, budget=-1, **good)[0] == -1
    assert sc.raw_call(lambda *a: be._L.rd_segment(None, *a), budget=0, **good)[0] == -1    # a null context
    assert sc.raw_call(fn, raw=None, off=None, p=good["p"], n_reads=0, budget=0)[0] == 0   # n_reads == 0 is RD_OK
    # offsets that claim 2^30 + 1 samples behind a short read: TOO_LONG, and the short read is done
    x = sc.levels(np.random.default_rng(3), 300)
    rc, outs = sc.raw_call(fn, raw=x, off=[0, 300, 300 + ref.MAX_T + 1], p=good["p"], budget=0)
    exp = ref.segment(x, good["p"])
    assert rc == 0 and outs[0].tolist() == [ref.OK, ref.TOO_LONG] and outs[1].tolist() == [exp["n_events"], 0]
    assert outs[4][:exp["n_events"]].tolist() == exp["start"]


# ---------------------------------------------------------------------------------------------- the command
N_SIM = 12


def _simulated_run(tmp_path, capsys):
    """N_SIM reads of `simulate` over eight random transcripts -> (the simulator's directory, the directory of its three fast5 files)"""
    from radian_amd import simulate
    rng = np.random.default_rng(41)
    fa = tmp_path / "panel.fa"
    fa.write_text("".join(f">t{t}\n{''.join('ACGT'[c] for c in rng.integers(0, 4, 700))}\n" for t in range(8)))
    sim = tmp_path / "sim"
    simulate.main([str(fa), "-o", str(sim), "--reads", str(N_SIM), "--seed", "6", "--length-median", "300", "--length-sigma", "0.4", "--min-length", "100",
                   "--tail", "40", "--model-seed", "7", "--reads-per-file", "5"])
    capsys.readouterr()
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    for f in sorted(os.listdir(sim)):
        if f.endswith(".fast5"):
            os.rename(sim / f, in_dir / f)
    return sim, in_dir


def test_command_on_a_simulated_run(be, tmp_path, capsys):
    """Every file is bit-identical across --batch-reads 1 / 7 / all and two budgets; every read's rows are the host composition's
    (rd_segment_host from the bound on, the command's own row writer)"""
    from radian_amd import fast5, segment as cmd
    from radian_amd.backend import SegmentParams, segment_host, segment_workspace_bytes
    sim, in_dir = _simulated_run(tmp_path, capsys)
    reads = [(os.path.splitext(os.path.basename(f))[0], rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16))
             for f in fast5.list_files(str(in_dir)) for rd in fast5.iter_reads(f)]
    assert len(reads) == N_SIM and len({r[0] for r in reads}) == 3
    need = max(segment_workspace_bytes(len(r[2]), 4) for r in reads)
    outs = {}
    for name, extra in (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                        ("all", ["--batch-reads", str(N_SIM), "--budget-bytes", str(3 * need)])):
        d = tmp_path / name
        st = cmd.main([str(in_dir), "-o", str(d), "--bounds", str(sim / "truth.tsv"), "--summary", str(tmp_path / (name + ".summary.tsv"))] + extra)
        text = capsys.readouterr().out
        assert (st["reads"], st["ok"]) == (N_SIM, N_SIM) and f"reads: {N_SIM} seen" in text and "events per 1000 samples: " in text
        outs[name] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
        outs[name]["summary"] = open(tmp_path / (name + ".summary.tsv"), "rb").read()
    assert outs["b1"] == outs["b7"] == outs["all"] and sorted(outs["all"]) == sorted([s + ".segments.tsv" for s in {r[0] for r in reads}] + ["summary"])
    bounds = cmd.read_bounds(str(sim / "truth.tsv"))
    want, want_summary = {}, ["\t".join(cmd.SUMMARY_COLUMNS)]
    for stem, rid, raw in reads:
        t_lo = cmd.window_start(rid, len(raw), bounds, 32)[0]
        assert 0 < t_lo < len(raw)
        res = segment_host([raw[t_lo:]], SegmentParams())
        rows, lens = cmd.read_rows(rid, t_lo, len(raw) - t_lo, res.events[0])
        assert rows[0][2] == str(t_lo) and rows[-1][3] == str(len(raw)) and all(a[3] == b[2] for a, b in zip(rows, rows[1:])) and len(rows) > 50
        want.setdefault(stem, ["\t".join(cmd.COLUMNS)]).extend("\t".join(r) for r in rows)
        want_summary.append("\t".join((rid, "ok", str(len(raw)), str(len(rows)), f"{float(np.median(lens)):.1f}")))
    for stem, lines in want.items():
        assert outs["all"][stem + ".segments.tsv"].decode() == "\n".join(lines) + "\n", stem
    assert outs["all"]["summary"].decode() == "\n".join(want_summary) + "\n"


def test_sigmap_events_equals_the_host_composition_and_sample_mode_is_unchanged(be, tmp_path, capsys):
    """`sigmap --events` on the simulated run: read_ref.tsv, the PAF and the summary are bit-identical across --batch-reads and are the rows of
    the command's two passes over rd_segment_host and rd_sigmap_host; two runs without --events write the same bytes, with the summary's
    thirteen columns"""
    from radian_amd import fast5, sigmap as cmd
    from radian_amd.backend import SegmentParams, SigmapPanel, segment_host, sigmap_host
    from radian_amd.map import Transcripts
    from radian_amd.simulate import standin_tables
    sim, in_dir = _simulated_run(tmp_path, capsys)
    fa = str(tmp_path / "panel.fa")
    common = [str(in_dir), fa, "--model-seed", "7", "--bounds", str(sim / "truth.tsv"), "--query-samples", "1024"]
    outs = {}
    for name, extra in (("e1", ["--events", "--batch-reads", "1"]), ("e5", ["--events", "--batch-reads", "5"]), ("s1", ["--batch-reads", "4"]), ("s2", [])):
        d = tmp_path / name
        d.mkdir()
        st = cmd.main(common + ["-o", str(d / "read_ref.tsv"), "--paf", str(d / "map.paf"), "--summary", str(d / "summary.tsv")] + extra)
        capsys.readouterr()
        assert (st["reads"], st["ok"]) == (N_SIM, N_SIM)
        outs[name] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    assert outs["e1"] == outs["e5"] and outs["s1"] == outs["s2"] and outs["e1"]["summary.tsv"] != outs["s1"]["summary.tsv"]
    head = lambda o: o["summary.tsv"].decode().split("\n")[0].split("\t")
    assert head(outs["s1"]) == list(cmd.SUMMARY_COLUMNS) and head(outs["e1"]) == list(cmd.SUMMARY_COLUMNS) + ["n_events"]
    # the host composition of the event mode, a read per call
    panel = cmd.Panel(Transcripts.read(fa, None, None), 8)
    model = cmd.model_tables(5, *standin_tables(5, 7)[:2])[0]
    packed = SigmapPanel(panel.codes, panel.off)
    args = cmd.build_parser().parse_args(common + ["-o", "x", "--events"])
    bounds = cmd.read_bounds(str(sim / "truth.tsv"))
    sig = lambda raw, q_lo, q_hi, **kw: sigmap_host(raw, packed, model, q_lo, q_hi, **kw)
    seg = lambda raws: segment_host(raws, SegmentParams(), [(0, len(x)) for x in raws])
    reads = [(rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16)) for f in fast5.list_files(str(in_dir)) for rd in fast5.iter_reads(f)]
    rows = [cmd.map_batch(sig, [rd], panel, bounds, args, seg)[0] for rd in reads]
    assert all(r["status"] == "ok" and r["T1"] == r["T2"] == min(256, r["n_events"]) for r in rows) and sum(r["n_events"] > 256 for r in rows) >= N_SIM // 2
    assert outs["e1"]["read_ref.tsv"].decode() == cmd.TSV_HEADER + "".join(cmd.tsv_row(r, panel) for r in rows)
    assert outs["e1"]["map.paf"].decode() == "".join(cmd.paf_row(r, panel) for r in rows)
    assert outs["e1"]["summary.tsv"].decode().split("\n")[1:-1] == [cmd.summary_row(r, panel).rstrip("\n") for r in rows]
    truth = {ln.split("\t")[0]: ln.split("\t")[1] for ln in open(sim / "truth.tsv").read().split("\n")[1:-1]}
    right = sum(1 for r in rows if panel.transcripts.names[panel.tr[r["j"]]] == truth[r["id"]])
    assert right >= N_SIM - 1, right      # unrelated random transcripts: nothing to confuse them with
