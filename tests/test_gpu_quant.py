"""GPU checks of transcript quantification: rd_quant_em == the host twin == the restatement (tests/_quant_ref.py)
on every seeded case of tests/_quant_cases.py -- counts, shares and stats[0..5] --, under a permutation of the reads and without the
shares; rd_map_candidates == the restatement on every candidate case and every field, row 0 == rd_map_batch's hit, the same rows one
read per call and under a budget that forces several launches, one read over the budget; the refusals; and python -m radian_amd.quant
end to end.  Every comparison of integers is for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _map_ref as mr
import _quant_cases as qc
import _quant_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGT"


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in qc.em_cases():
        count, shares, iters, last = ref.em(c["reads"], c["n_tx"], c["max_iter"], c["tol_q20"])
        out.append(dict(c, count=count, shares=shares, iters=iters, last=last))
    return out


@pytest.fixture(scope="module")
def sim():
    """the simulated set of the mapping tests and the restatement's candidates under the command's defaults, once"""
    transcripts, reads, truth = mr.simulate()
    index = mr.build_index(transcripts, 14, 8)
    lengths = [len(t) for t in transcripts]
    return transcripts, reads, [ref.candidates(r, index, lengths) for r in reads]


def _offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.concatenate(seqs), off


def _index(be, transcripts):
    return be.map_index(*_offsets(transcripts), 14, 8, 500)


def _assert_cands(res, exp, K, what):
    assert len(res.status) == len(exp)
    for i, e in enumerate(exp):
        got = (int(res.status[i]), int(res.n_qual[i]), int(res.n_cand[i]))
        assert got == (e["status"], e["n_qual"], e["n_cand"]), f"{what}: read {i}: (status, n_qual, n_cand) = {got}, the restatement gives {e}"
        rows = [tuple(int(v) for v in row) for row in res.cands[i]]
        assert rows == e["rows"] + [(0,) * 8] * (K - len(e["rows"])), f"{what}: read {i}: rows"


# ---------------------------------------------------------------------------------------------- the EM
def test_quant_em_equals_the_host_twin_and_the_restatement_on_every_case(be, cases):
    from radian_amd.backend import quant_em_host
    rng = np.random.default_rng(6)
    for c in cases:
        args = ref.csr(c["reads"]) + (c["n_tx"], c["max_iter"], c["tol_q20"])
        res, host = be.quant_em(*args), quant_em_host(*args)
        ref.assert_em_equal(res, c, "rd_quant_em")
        assert np.array_equal(res.count, host.count) and np.array_equal(res.share, host.share), c["name"]
        assert {k: v for k, v in res.stats.items() if k != "stage_us"} == {k: v for k, v in host.stats.items() if k != "stage_us"}, c["name"]
        # without the shares: the same counts
        bare = be.quant_em(*args, with_share=False)
        assert bare.share is None and np.array_equal(bare.count, res.count), c["name"]
        # a permutation of the reads: the same counts, iterations and last delta
        perm = rng.permutation(len(c["reads"]))
        p = be.quant_em(*ref.csr([c["reads"][i] for i in perm]), c["n_tx"], c["max_iter"], c["tol_q20"])
        assert [int(v) for v in p.count] == c["count"] and p.stats["iterations"] == c["iters"] and p.stats["last_delta"] == c["last"], c["name"]
        inv = np.argsort(perm)
        rows = np.split(p.share, np.cumsum([len(c["reads"][i]) for i in perm])[:-1]) if len(perm) else []
        assert [int(v) for i in inv for v in rows[i]] == [s for row in c["shares"] for s in row] if len(perm) else True, c["name"]


def test_quant_em_refusals_leave_the_outputs_untouched(be):
    assert ref.check_refusals(be._L.rd_quant_em, be._h) >= 15


# ---------------------------------------------------------------------------------------------- the candidates
def test_map_candidates_equals_the_restatement_on_the_simulated_set(be, sim):
    transcripts, reads, exp = sim
    _index(be, transcripts)
    res = be.map_candidates(reads, with_stats=True)
    _assert_cands(res, exp, 16, "simulated set")
    assert sum(1 for e in exp if e["n_qual"] > 1) > 30 and res.stats["stage_us"]["best"] == 0
    # row 0 is rd_map_batch's hit
    hit = be.map_batch(reads)
    assert np.array_equal(hit.status, res.status)
    assert np.array_equal(hit.hits[:, [0, 1, 3, 4, 5, 6, 7]], res.cands[:, 0, :7])
    # one read per call, and a budget that forces several launches
    for i in range(0, len(reads), 7):
        one = be.map_candidates([reads[i]])
        assert int(one.status[0]) == int(res.status[i]) and int(one.n_qual[0]) == int(res.n_qual[i]) and np.array_equal(one.cands[0], res.cands[i]), i
    small = be.map_candidates(reads, budget_bytes=(1 << 20) + 64 * 4000, with_stats=True)
    assert small.stats["launches"] > 4 * res.stats["launches"]
    for name in ("status", "n_qual", "n_cand", "cands"):
        assert np.array_equal(getattr(small, name), getattr(res, name)), name


def test_map_candidates_keeps_the_smallest_t_of_70_equal_chains(be):
    transcripts, reads = qc.copies_case()
    _index(be, transcripts)
    index = mr.build_index(transcripts, 14, 8)
    for K in (64, 2, 1):
        exp = [ref.candidates(reads[0], index, [len(t) for t in transcripts], max_cand=K)]
        assert exp[0]["n_qual"] == 70 and exp[0]["n_cand"] == K
        _assert_cands(be.map_candidates(reads, max_cand=K), exp, K, f"70 copies, K = {K}")


def test_map_candidates_of_a_read_with_thousands_of_segments(be):
    transcripts, reads = qc.many_segments_case()
    be.map_index(*_offsets(transcripts), 14, 8, 4000)
    index = mr.build_index(transcripts, 14, 8)
    exp = ref.candidates(reads[0], index, [len(t) for t in transcripts], max_occ=4000, max_cand=64, min_frac_q10=0)
    assert exp["n_qual"] == 2100 and [r[0] for r in exp["rows"]] == list(range(64)) and len({r[1] for r in exp["rows"]}) == 1
    _assert_cands(be.map_candidates(reads, max_cand=64, min_frac_q10=0), [exp], 64, "2100 copies, K = 64")
    # every chain scores the same: at min_frac_q10 = 1024 all 2100 stay candidates, and K = 7 keeps the first seven
    _assert_cands(be.map_candidates(reads, max_cand=7, min_frac_q10=1024), [dict(exp, n_cand=7, rows=exp["rows"][:7])], 7, "2100 copies, K = 7")


def test_map_candidates_fraction_and_three_prime_filter(be):
    transcripts, reads = qc.edge_case()
    _index(be, transcripts)
    index = mr.build_index(transcripts, 14, 8)
    lengths = [len(t) for t in transcripts]
    seen = set()
    for p in qc.CAND_PARAMS:
        exp = [ref.candidates(r, index, lengths, **p) for r in reads]
        _assert_cands(be.map_candidates(reads, **p), exp, p["max_cand"], str(p))
        seen |= {e["status"] for e in exp}
        if p["max_3p"] >= 0:
            assert exp[0]["status"] == mr.NO_CHAIN      # its only chain fails the filter
        else:
            assert exp[2]["rows"][0][7] == -60          # the read runs past the transcript's end
    assert seen == {mr.OK, mr.NO_SEED, mr.NO_CHAIN}


def test_map_candidates_too_large_for_exactly_one_read(be, sim):
    from radian_amd import RadianHipError
    from radian_amd.backend import MAP_TOO_LARGE
    transcripts, reads, exp = sim
    _index(be, transcripts)
    whole = be.map_candidates(reads[:40], with_stats=True)
    big = np.concatenate([transcripts[i] for i in range(12)])          # far more anchors than any read of the set
    batch = reads[:20] + [big] + reads[20:40]
    full = be.map_candidates(batch, with_stats=True)
    anchors_big = full.stats["anchors"] - whole.stats["anchors"]
    budget = (1 << 20) + 64 * (anchors_big - 1)
    with pytest.raises(RadianHipError, match="read 20 has"):
        be.map_candidates(batch, budget_bytes=budget)
    res = be.map_candidates(batch, budget_bytes=budget, allow_too_large=True)
    assert [i for i, s in enumerate(res.status) if s == MAP_TOO_LARGE] == [20]
    assert int(res.n_qual[20]) == 0 and int(res.n_cand[20]) == 0 and not res.cands[20].any()
    keep = [i for i in range(41) if i != 20]
    assert np.array_equal(res.cands[keep], whole.cands) and np.array_equal(res.status[keep], whole.status) and np.array_equal(res.n_qual[keep], whole.n_qual)


def test_map_candidates_refusals_leave_the_outputs_untouched(be, sim):
    import ctypes
    transcripts, reads, exp = sim
    _index(be, transcripts)
    buf, off = _offsets(reads[:3])
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(K=16, frac=922, m3=-1, min_anchors=3, null=None, off_=off):
        out = dict(status=np.full(3, 0x4D, np.int32), n_qual=np.full(3, 0x4D, np.int32), n_cand=np.full(3, 0x4D, np.int32),
                   cands=np.full(3 * 64 * 8, 0x4D, np.int32), stats=np.full(16, 0x4D, np.int64))
        a = {k: (None if k == null else v) for k, v in out.items()}
        rc = be._L.rd_map_candidates(be._h, p(buf), p(off_), 3, min_anchors, 40, 1000, 500, 0, K, frac, m3, p(a["status"]), p(a["n_qual"]), p(a["n_cand"]),
                                     p(a["cands"]), p(a["stats"]))
        assert all((v == 0x4D).all() for v in out.values()), (K, frac, m3, null)
        return rc

    bad_off = off.copy()
    bad_off[1] = off[2] + 1
    for kw in (dict(K=0), dict(K=65), dict(frac=-1), dict(frac=1025), dict(m3=-2), dict(min_anchors=0), dict(null="status"), dict(null="n_qual"),
               dict(null="n_cand"), dict(null="cands"), dict(off_=bad_off)):
        assert call(**kw) == -1, kw


# ---------------------------------------------------------------------------------------------- the command
def _write_fasta(path, records):
    with open(path, "w") as f:
        for rid, seq in records:
            f.write(f">{rid}\n{seq}\n")


def test_quant_command_end_to_end(be, tmp_path, capsys):
    """on the accuracy generator's first setting: the files equal what this test composes from Backend calls, they are bit-identical
    across --batch-reads and --budget-bytes, and the device's counts meet the accuracy condition"""
    from radian_amd import quant
    mode, seed = ref.ACCURACY_SETTINGS[0]
    transcripts, reads, truth, true = ref.accuracy_set(mode, seed)
    letters = lambda codes: "".join(LETTERS[c] for c in codes)
    names = [f"tx{t}|gene{t // 3}" for t in range(len(transcripts))]
    records = [(f"read{i}", letters(r)) for i, r in enumerate(reads)] + [("withN", "ACGTNACGT" * 30), ("short", "ACGT")]
    _write_fasta(tmp_path / "reads.fasta", records)
    _write_fasta(tmp_path / "tx.fa", [(f"{n} extra words", letters(t)) for n, t in zip(names, transcripts)])
    # the command, as a command
    base = ["radian_amd.quant", str(tmp_path / "reads.fasta"), str(tmp_path / "tx.fa"), "--tol", str(ref.ACCURACY_PARAMS["tol_q20"] / ref.ONE)]
    p = subprocess.run([sys.executable, "-m", *base, "-o", str(tmp_path / "q0.tsv"), "--assign", str(tmp_path / "a0.tsv")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONPATH": ROOT})
    assert p.returncode == 0, p.stdout + p.stderr
    q0, a0 = open(tmp_path / "q0.tsv").read(), open(tmp_path / "a0.tsv").read()
    # other batches and budgets, in this process
    for tag, extra in (("1", ["--batch-reads", "37"]), ("2", ["--batch-reads", "150", "--budget-bytes", str((1 << 20) + 64 * 6000)])):
        quant.main(base[1:] + ["-o", str(tmp_path / f"q{tag}.tsv"), "--assign", str(tmp_path / f"a{tag}.tsv")] + extra)
        assert open(tmp_path / f"q{tag}.tsv").read() == q0 and open(tmp_path / f"a{tag}.tsv").read() == a0, extra
    capsys.readouterr()
    # what the Backend gives, composed here
    P = ref.ACCURACY_PARAMS
    _index(be, transcripts)
    res = be.map_candidates(reads, P["max_cand"], P["min_frac_q10"], P["max_3p"])
    qreads = [[(int(res.cands[i, j, 0]), 1) for j in range(int(res.n_cand[i]))] for i in range(len(reads))] + [[], []]
    em = be.quant_em(*ref.csr(qreads), len(transcripts), P["max_iter"], P["tol_q20"])
    count = [int(c) for c in em.count]
    total = sum(count)
    dec = lambda v: f"{v >> 20}.{(v % ref.ONE) * 10 ** 6 // ref.ONE:06d}"
    lines = ["ref_name\tlength\test_count\ttpm\tn_unique\tn_multi\n"]
    for t, name in enumerate(names):
        m = count[t] * 10 ** 9 // total
        lines.append(f"{name}\t{len(transcripts[t])}\t{dec(count[t])}\t{m // 1000}.{m % 1000:03d}\t{sum(1 for r in qreads if len(r) == 1 and r[0][0] == t)}\t"
                     f"{sum(1 for r in qreads if len(r) > 1 and t in [c[0] for c in r])}\n")
    assert q0 == "".join(lines)
    lines, at = ["read_id\tstatus\tn_qual\tn_cand\tref_name\tshare\n"], 0
    status_names = {mr.OK: "ok", mr.NO_SEED: "no-seed", mr.NO_CHAIN: "no-chain"}
    for i, (rid, _) in enumerate(records):
        r = qreads[i]
        if i >= len(reads):
            lines.append(f"{rid}\t{'non-ACGT' if rid == 'withN' else 'no-seed'}\t0\t0\t*\t0.000000\n")
            continue
        sh = [int(v) for v in em.share[at: at + len(r)]]
        at += len(r)
        if not r:
            lines.append(f"{rid}\t{status_names[int(res.status[i])]}\t0\t0\t*\t0.000000\n")
            continue
        j = max(range(len(r)), key=lambda c: (sh[c], -r[c][0]))
        lines.append(f"{rid}\t{status_names[int(res.status[i])]}\t{int(res.n_qual[i])}\t{int(res.n_cand[i])}\t{names[r[j][0]]}\t{dec(sh[j])}\n")
    assert a0 == "".join(lines)
    # the command's summary names the figures
    for word in ("reads: 402 seen", "reads with more than one candidate:", "truncated at --max-cand: 0", "iterations", "lost mass", "non-zero count"):
        assert word in p.stdout, (word, p.stdout)
    # the accuracy condition on the device's output
    l1_hit, l1_em = ref.l1_errors(true, count, [r[0][0] for r in qreads if r])
    print(f"{mode} seed {seed} on the device: multi-candidate reads {sum(1 for r in qreads if len(r) > 1)}, iterations {em.stats['iterations']}, "
          f"L1 best-hit {l1_hit}, L1 EM {l1_em:.1f}")
    assert 2 * l1_em <= l1_hit, (l1_em, l1_hit)
