"""GPU checks of sigmap: rd_sigmap against the restatement of its contract (tests/_sigmap_ref.py) on the seeded
cases (tests/_sigmap_cases.py; their defining conditions are asserted in tests/test_sigmap_cpu.py).  Every output field is compared for
EXACT equality.

Sizes follow the DP kernel: a lane owns 16 states, a wave 1024, a workgroup pass (band) 4096, a stripe reports SIGMAP_PAYLOAD ends -- state
ranges on both sides of each; T on both sides of 16 and of the 128-row tile, 300 and 2^14; ends on a stripe's first and last state with the
origin T - 1 states before it; a path across a band's edge; targets of one state, shorter than T and empty; ties; every status beside
unaffected neighbours."""
import numpy as np
import pytest

import _sigmap_cases as sc
import _sigmap_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    cs = sc.all_cases()
    for c in cs:
        sc.reference(c)
    return cs


def _run(be, cases, **kw):
    return be.sigmap(sc.raw(), sc.backend_panel(), sc.backend_model(), n_best=kw.pop("n_best", sc.N_BEST), **sc.call_args(cases), **kw)


@pytest.fixture(scope="module")
def whole(be, cases):
    return _run(be, cases)


def _need(cases):
    from radian_amd.backend import sigmap_workspace_bytes
    p = sc.panel()
    out = []
    for c in cases:
        n = c["s_hi"] - c["s_lo"]
        nt = p.tgt[c["s_hi"] - 1] - p.tgt[c["s_lo"]] + 1 if n else 0
        out.append(sigmap_workspace_bytes(c["q_hi"] - c["q_lo"], n, nt))
    return out


def _same(a, i, b, j, what=""):
    for f in ("status", "m2", "d4"):
        assert int(getattr(a, f)[i]) == int(getattr(b, f)[j]), (what, f)
    for f in ref.FIELDS:
        assert getattr(a, f)[i].tolist() == getattr(b, f)[j].tolist(), (what, f)


def test_the_batch_equals_the_restatement(cases, whole):
    """every case in one call: every status sits between queries that are mapped, and none of them is affected"""
    for q, c in enumerate(cases):
        ref.assert_query_equal(whole, q, sc.reference(c), c["name"])
    assert {int(s) for s in whole.status} == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_TARGET}


def test_one_query_per_call_reversed_and_other_n_best(be, cases, whole):
    for q, c in enumerate(cases):
        if sc.cells(c) <= 2000000:
            _same(_run(be, [c]), 0, whole, q, c["name"])
    rev = _run(be, cases[::-1])
    for q, c in enumerate(cases):
        _same(rev, len(cases) - 1 - q, whole, q, c["name"])
    for nb in (1, 3):
        res = _run(be, cases, n_best=nb)
        for q, c in enumerate(cases):
            for f in ref.FIELDS:
                assert getattr(res, f)[q].tolist() == getattr(whole, f)[q].tolist()[:nb], (c["name"], f, nb)


def test_budget_from_the_workspace_formula(be, cases, whole):
    """a budget of exactly the largest query's workspace: every query is mapped, over several launches; one byte less: the queries of that
    size are TOO_LARGE, the call names the first with RD_ERR_NOMEM and the others are as before"""
    from radian_amd.backend import SIGMAP_TOO_LARGE, RadianHipError
    need = [n if int(whole.status[q]) == ref.OK else 0 for q, n in enumerate(_need(cases))]
    big = int(np.argmax(need))
    over = [q for q, n in enumerate(need) if n == need[big]]
    assert sum(need) > 3 * need[big] and len(over) <= 2
    res = _run(be, cases, budget_bytes=need[big])
    for q, c in enumerate(cases):
        _same(res, q, whole, q, c["name"])
    with pytest.raises(RadianHipError) as ei:
        _run(be, cases, budget_bytes=need[big] - 1)
    assert f"query {big} " in str(ei.value) and f"{len(over)} query(ies) not mapped" in str(ei.value)
    res = _run(be, cases, budget_bytes=need[big] - 1, allow_too_large=True)
    for q, c in enumerate(cases):
        if q not in over:
            _same(res, q, whole, q, c["name"])
        else:
            assert int(res.status[q]) == SIGMAP_TOO_LARGE and res.tgt[q].tolist() == res.score[q].tolist() == res.end[q].tolist() == res.org[q].tolist() == [-1] * sc.N_BEST
            assert (int(res.m2[q]), int(res.d4[q])) == (int(whole.m2[q]), int(whole.d4[q]))      # the scale is the query's own, whatever the budget
    # a small budget: many launches, and every query over it is reported
    small = sorted(n for n in need if n)[len(need) // 3]
    res = _run(be, cases, budget_bytes=small, allow_too_large=True)
    for q, c in enumerate(cases):
        if need[q] <= small:
            _same(res, q, whole, q, c["name"])
        else:
            assert int(res.status[q]) == SIGMAP_TOO_LARGE


def test_many_queries_on_shared_samples_with_disjoint_ranges(be):
    """the second pass's shape: one window of samples, one given scale, a query per candidate range"""
    p = sc.panel()
    c = next(x for x in sc.all_cases() if x["name"] == "panel_given")
    J = sc.target_index()
    ranges = [(p.off[J[f"L{L}"]] + L // 3, p.off[J[f"L{L}"] + 1]) for L in sc.LENGTHS] + [(p.off[J["big"]] + 4990, p.off[J["big"] + 1])]
    n = len(ranges)
    res = be.sigmap(sc.raw(), sc.backend_panel(), sc.backend_model(), [c["q_lo"]] * n, [c["q_hi"]] * n, m2=[c["m2"]] * n, d4=[c["d4"]] * n,
                    s_lo=[r[0] for r in ranges], s_hi=[r[1] for r in ranges], n_best=1)
    for q, (lo, hi) in enumerate(ranges):
        want = ref.map_numpy(sc.raw(), p, c["q_lo"], c["q_hi"], c["q_lo"], c["q_hi"], c["m2"], c["d4"], lo, hi, 1)
        ref.assert_query_equal(res, q, want, str((lo, hi)))
    assert abs(int(res.org[n - 1, 0]) - 5000) < 8 and abs(int(res.end[n - 1, 0]) - 5099) < 8      # local to the target, not to the range


# ---------------------------------------------------------------------------------------------- the command
def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]


N_SIM = 72      # reads of the simulated run: about 0.4 of them are on a gene and extend 100 bases beyond its shared part


def _simulated_run(tmp_path, capsys):
    """N_SIM reads of `simulate` over the accuracy panel (eight genes x three isoforms that share 600 bases at the 3' end, 16 unrelated
    transcripts; tails of 60 A, the stand-in of seed 7) -> (fasta, the simulator's directory, the directory of its fast5 files)"""
    import os
    from radian_amd import simulate
    tr, _ = sc.accuracy_transcripts()
    fa = tmp_path / "panel.fa"
    fa.write_text("".join(f">{tr.names[t]}\n{tr.letters(t, 0, tr.length(t))}\n" for t in range(len(tr.names))))
    sim = tmp_path / "sim"
    simulate.main([str(fa), "-o", str(sim), "--reads", str(N_SIM), "--seed", "5", "--length-median", "900", "--length-sigma", "0.5", "--min-length", "300",
                   "--tail", "60", "--model-seed", "7", "--reads-per-file", "40"])
    capsys.readouterr()
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    for f in sorted(os.listdir(sim)):
        if f.endswith(".fast5"):
            os.rename(sim / f, in_dir / f)
    return fa, sim, in_dir


def test_command_on_a_simulated_run(be, tmp_path, capsys):
    """Every file is bit-identical across --batch-reads 1 / 7 / all and two budgets; every read's rows are the host composition's
    (the command's two passes over rd_sigmap_host); against truth.tsv the reads that extend at least 100 bases beyond their gene's shared
    part go to their isoform with both span ends near the truth (at least 24 such reads; the floors of tests/test_sigmap_cpu.py, DESIGN.md
    section 25), those that end inside it stay on their gene and tied, the reads of unrelated transcripts and the barely-beyond ones meet
    the same floor on their transcript or gene; `eventalign` on the written read_ref.tsv puts as many first samples within 30 of truth_moves.tsv as it
    does on the simulator's own read_ref.tsv, less the margin of DESIGN.md section 25."""
    import os
    from radian_amd import eventalign, fast5, sigmap as cmd
    from radian_amd.backend import SigmapPanel, sigmap_host, sigmap_workspace_bytes
    from radian_amd.simulate import standin_tables
    fa, sim, in_dir = _simulated_run(tmp_path, capsys)
    tr, gene = sc.accuracy_transcripts()
    panel = cmd.Panel(tr, sc.ACC_PAD)
    need = sigmap_workspace_bytes(sc.ACC_QUERY, panel.states, len(panel.tr))
    common = [str(in_dir), str(fa), "--model-seed", "7", "--bounds", str(sim / "truth.tsv"), "--query-samples", str(sc.ACC_QUERY), "--tail-pad", str(sc.ACC_PAD)]
    outs = {}
    for name, extra in (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                        ("all", ["--batch-reads", str(N_SIM), "--budget-bytes", str(3 * need)])):
        d = tmp_path / name
        d.mkdir()
        st = cmd.main(common + ["-o", str(d / "read_ref.tsv"), "--paf", str(d / "map.paf"), "--summary", str(d / "summary.tsv")] + extra)
        text = capsys.readouterr().out
        assert (st["reads"], st["ok"]) == (N_SIM, N_SIM) and f"states: {panel.states}" in text and "transcripts: 40 read, 40 kept, 0 skipped" in text
        outs[name] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    assert outs["b1"] == outs["b7"] == outs["all"] and sorted(outs["all"]) == ["map.paf", "read_ref.tsv", "summary.tsv"]
    rows = _tsv(str(tmp_path / "all" / "read_ref.tsv"))
    paf = {r[0]: r for r in _tsv(str(tmp_path / "all" / "map.paf"))}
    assert rows[0] == ["read_id", "transcript", "sequence"] and len(rows) == N_SIM + 1 and len(paf) == N_SIM
    # the host composition on every read: the command's two passes over rd_sigmap_host, a read per call (a row does not depend on its
    # batch), the calls side by side on the host's threads
    from concurrent.futures import ThreadPoolExecutor
    model = cmd.model_tables(sc.ACC_K, *standin_tables(sc.ACC_K, sc.ACC_MODEL_SEED)[:2])[0]
    bounds = cmd.read_bounds(str(sim / "truth.tsv"))
    reads = [(rd.read_id, np.ascontiguousarray(rd.get_raw_data(), dtype=np.int16)) for f in fast5.list_files(str(in_dir)) for rd in fast5.iter_reads(f)]
    assert [r[0] for r in reads] == [r[0] for r in rows[1:]]
    packed = SigmapPanel(panel.codes, panel.off)
    host_sig = lambda raw, q_lo, q_hi, **kw: sigmap_host(raw, packed, model, q_lo, q_hi, **kw)
    with ThreadPoolExecutor(max_workers=12) as pool:
        host = list(pool.map(lambda rd: cmd.map_batch(host_sig, [rd], panel, bounds, sc.accuracy_args())[0], reads))
    assert len(host) == N_SIM
    for row, got in zip(host, rows[1:]):
        assert cmd.tsv_row(row, panel).rstrip("\n").split("\t") == got and cmd.paf_row(row, panel).rstrip("\n").split("\t") == paf[row["id"]], row["id"]
    # against the truth
    truth = {r[0]: (r[1], int(r[2]), int(r[3])) for r in _tsv(str(sim / "truth.tsv"))[1:]}
    name_of = {n: t for t, n in enumerate(tr.names)}
    counted = right = others = others_right = 0
    d5, d3 = [], []
    for rid, name, seq in rows[1:]:
        t_true, S, E = name_of[truth[rid][0]], truth[rid][1], truth[rid][2]
        t = name_of[name]
        p = paf[rid]
        assert seq == tr.letters(t, int(p[7]), int(p[8])) and int(p[6]) == tr.length(t)
        beyond = gene[t_true] >= 0 and S <= tr.length(t_true) - sc.ACC_SHARED - sc.ACC_BEYOND
        inside = gene[t_true] >= 0 and S >= tr.length(t_true) - sc.ACC_SHARED
        if beyond:
            counted += 1
            if t == t_true:
                right += 1
                d5.append(int(p[7]) - S)
                d3.append(int(p[8]) - E)
        elif inside:
            assert gene[t] == gene[t_true] and p[15] == "nt:i:3", rid
        else:       # an unrelated transcript: the transcript itself; a gene read that ends 0 .. 99 bases beyond the shared part: its gene
            others += 1
            others_right += t == t_true if gene[t_true] < 0 else gene[t] == gene[t_true]
    with capsys.disabled():
        print(f"\nsigmap on the simulated run: isoform right {right} of {counted}; 5' end {min(d5)} .. {max(d5)}, 3' end {min(d3)} .. {max(d3)}; "
              f"unrelated and barely-beyond reads right {others_right} of {others}")
    # the floors of tests/test_sigmap_cpu.py: 26 of 28 reads, 31 and 6 bases
    assert counted >= 24 and 28 * right >= 26 * counted
    assert others >= 12 and 28 * others_right >= 26 * others
    assert max(abs(d) for d in d5) <= 31 and max(abs(d) for d in d3) <= 6
    # eventalign on sigmap's read_ref.tsv against eventalign on the simulator's
    moves = {r[0]: np.array(r[2].split(","), dtype=np.int64) for r in _tsv(str(sim / "truth_moves.tsv"))[1:]}
    share = {}
    for which, rr in (("sigmap", tmp_path / "all" / "read_ref.tsv"), ("truth", sim / "read_ref.tsv")):
        d = tmp_path / ("ea_" + which)
        st = eventalign.main([str(in_dir), str(rr), "-o", str(d), "--model-seed", "7", "--bounds", str(sim / "truth.tsv")])
        capsys.readouterr()
        assert st["ok"] >= N_SIM - 2
        ev = [r for f in sorted(os.listdir(d)) for r in _tsv(str(d / f))[1:]]
        near = total = 0
        for rid in moves:
            mine = [r for r in ev if r[0] == rid]
            total += len(moves[rid])
            if not mine:
                continue
            # a row's ref_pos counts from its span's start, the truth's moves from the fragment's: both as the distance from the transcript's
            # 3' end, which isoforms that tie on their shared part have in common
            t_map = name_of[mine[0][1]]
            S_map = int(paf[rid][7]) if which == "sigmap" else truth[rid][1]
            first = {tr.length(t_map) - (S_map + int(r[2])): int(r[4]) for r in mine}
            L_true = tr.length(name_of[truth[rid][0]])
            near += sum(abs(first.get(L_true - (truth[rid][1] + b), -10 ** 9) - int(m)) <= 30 for b, m in enumerate(moves[rid]))
        share[which] = near / total
    with capsys.disabled():
        print(f"eventalign first samples within 30: {share['sigmap']:.4f} on sigmap's read_ref.tsv, {share['truth']:.4f} on the simulator's")
    assert share["sigmap"] >= share["truth"] - 0.12      # two reads of 28 on another transcript (the floor above), 31 of 700 bases at the 5' end
