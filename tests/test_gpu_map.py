"""GPU checks of read-to-transcript mapping: rd_map_index + rd_map_batch (map.hip) against the restatement of their contract
(tests/_map_ref.py) on every output field -- the simulated set and the contract's edge cases --, the same arrays under other budgets
and batch sizes, the spans of radian_amd.map against the restatement's, and python -m radian_amd.map end to end: byte-identical
files across runs, `align` on the result, the --stats counts, label_build's reader."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _map_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T0 = time.perf_counter()
LETTERS = "ACGT"


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def sim():
    transcripts, reads, truth = mr.simulate()
    hits, index = mr.map_reads(reads, transcripts)
    return transcripts, reads, truth, hits, index


def _offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return (np.concatenate(seqs) if off[-1] else np.zeros(0, dtype=np.uint8)), off


def _index(be, transcripts, **p):
    p = dict(mr.DEFAULTS, **p)
    codes, off = _offsets(transcripts)
    return be.map_index(codes, off, p["k"], p["w"], p["max_occ"])


def _map(be, reads, budget=0, allow=False, **p):
    p = dict(mr.DEFAULTS, **p)
    return be.map_batch(reads, p["min_anchors"], p["min_score"], p["max_gap"], p["bandwidth"], budget, allow_too_large=allow, with_stats=True)


def _assert_equal(res, hits, what):
    assert len(res.status) == len(hits)
    for i, h in enumerate(hits):
        got = (int(res.status[i]),) + tuple(int(v) for v in res.hits[i])
        exp = (h["status"],) + tuple(h[f] for f in mr.FIELDS)
        assert got == exp, f"{what}: read {i}: (status, {', '.join(mr.FIELDS)}) = {got}, the restatement gives {exp}"


def _edge_set():
    """transcripts and reads of the contract's edge cases (see the test below for the list)"""
    rng = np.random.default_rng(77)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    motif = rnd(40)
    t0 = rnd(1500)
    t1 = rnd(800)
    t3 = rnd(1000)
    t3[300:310] = 255
    t3[600] = 255
    t4 = np.concatenate([rnd(200), np.tile(np.array([0, 1], dtype=np.uint8), 300), rnd(100), np.zeros(200, dtype=np.uint8), rnd(100),
                         np.tile(np.array([0, 1, 2], dtype=np.uint8), 100), rnd(200)])
    t5 = rnd(3000)
    transcripts = [t0, t1, t1.copy(), t3, t4, t5] + [np.concatenate([rnd(300), motif, rnd(300)]) for _ in range(6)]
    reads = [
        rnd(5), np.zeros(0, dtype=np.uint8), rnd(13),                       # shorter than k (one of them empty)
        rnd(600), np.full(300, 255, dtype=np.uint8),                        # no seed: unrelated, all N
        motif.copy(),                                                       # only the repeated motif (a key above a small max_occ)
        t1.copy(),                                                          # two identical transcripts: tie, the smaller t, score2 = score
        t0.copy(),                                                          # a read equal to a whole transcript
        t3[200:900][t3[200:900] <= 3], mr.mutate(rng, t3[100:950][t3[100:950] <= 3], 0.12),   # across the transcript's N
        t5[700:2200].copy(), mr.mutate(rng, t5[200:2900], 0.12),            # segments of far more than 64 anchors
        t4[500:1000].copy(), np.zeros(100, dtype=np.uint8), np.tile(np.array([0, 1], dtype=np.uint8), 300), t4[1000:1500].copy(),   # low complexity
        np.concatenate([rnd(100), t0[500:530], rnd(100)]),                  # one or two anchors: no chain
        np.concatenate([t0[100:400], rnd(50), t5[1000:1400]]),              # two transcripts in one read
        np.concatenate([rnd(80), transcripts[7][250:400]]),                 # the motif and its surroundings
    ]
    return transcripts, reads


def test_map_batch_equals_the_restatement_on_the_simulated_set(be, sim):
    transcripts, reads, truth, hits, index = sim
    st = _index(be, transcripts)
    assert st["entries"] == mr.index_stats(index, 500)["entries"] and st["keys"] == len(index) and st["keys_dropped"] == 0
    res = _map(be, reads)
    _assert_equal(res, hits, "simulated set")
    assert res.stats["anchors"] == sum(len(mr.anchors(r, index, 14, 8, 500)) for r in reads)
    assert all(h["status"] == mr.OK for h in hits)


def test_map_batch_equals_the_restatement_on_the_edge_cases(be):
    """reads shorter than k; no usable seed; a key above max_occ; two identical transcripts; a read equal to a whole transcript;
    transcripts with N; segments of more than 64 anchors; low-complexity repeats -- at the default max_occ and at max_occ = 4"""
    transcripts, reads = _edge_set()
    for max_occ in (500, 4):
        hits, index = mr.map_reads(reads, transcripts, max_occ=max_occ)
        st = _index(be, transcripts, max_occ=max_occ)
        assert {k: st[k] for k in ("entries", "keys", "keys_dropped")} == mr.index_stats(index, max_occ)
        res = _map(be, reads)
        _assert_equal(res, hits, f"edge cases, max_occ {max_occ}")
        if max_occ == 4:
            assert st["keys_dropped"] > 0 and hits[5]["status"] == mr.NO_SEED
        else:
            assert hits[6]["status"] == mr.OK and hits[6]["t"] == 1 and hits[6]["score2"] == hits[6]["score"]
            assert hits[7]["t"] == 0 and hits[7]["n_anchors"] > 64 and hits[10]["n_anchors"] > 64
            assert hits[0]["status"] == hits[1]["status"] == hits[2]["status"] == hits[3]["status"] == hits[4]["status"] == mr.NO_SEED
            assert mr.NO_CHAIN in [h["status"] for h in hits]
    # other seed shapes
    for k, w in ((8, 1), (11, 5), (15, 20)):
        hits, index = mr.map_reads(reads, transcripts, k=k, w=w, max_occ=50)
        _index(be, transcripts, k=k, w=w, max_occ=50)
        _assert_equal(_map(be, reads), hits, f"edge cases, k {k} w {w}")


def test_map_batch_does_not_depend_on_budget_or_batches(be, sim):
    transcripts, reads, truth, hits, index = sim
    _index(be, transcripts)
    whole = _map(be, reads)
    small = _map(be, reads, budget=(1 << 20) + 64 * 4000)
    assert small.stats["launches"] > 4 * whole.stats["launches"]
    assert np.array_equal(small.status, whole.status) and np.array_equal(small.hits, whole.hits)
    parts = [_map(be, reads[a: a + 77]) for a in range(0, len(reads), 77)]
    assert np.array_equal(np.concatenate([p.status for p in parts]), whole.status)
    assert np.array_equal(np.concatenate([p.hits for p in parts]), whole.hits)


def test_map_batch_too_large_leaves_the_others_mapped(be):
    from radian_amd import RadianHipError
    from radian_amd.backend import MAP_TOO_LARGE
    transcripts, reads = _edge_set()
    hits, index = mr.map_reads(reads, transcripts)
    n_anchors = [len(mr.anchors(r, index, 14, 8, 500)) for r in reads]
    big = int(np.argmax(n_anchors))
    second = sorted(n_anchors)[-2]
    budget = (1 << 20) + 64 * (second + 1)
    assert n_anchors[big] > second + 1
    _index(be, transcripts)
    with pytest.raises(RadianHipError) as ei:
        _map(be, reads, budget=budget)
    assert f"read {big}" in str(ei.value) and "over the budget" in str(ei.value)
    res = _map(be, reads, budget=budget, allow=True)
    assert res.status[big] == MAP_TOO_LARGE and not res.hits[big].any()
    keep = [i for i in range(len(reads)) if i != big]
    _assert_equal(type(res)(res.status[keep], res.hits[keep]), [hits[i] for i in keep], "beside a read over the budget")


def _args(**over):
    from radian_amd import map as rmap
    return rmap.check_args(rmap.build_parser().parse_args(["reads.fasta", "tr.fa", "-o", "out.tsv"] + [str(x) for kv in over.items() for x in kv]))


def _records(reads):
    return [(f"read{i:04d}", "".join(LETTERS[c] for c in r)) for i, r in enumerate(reads)]


def _transcripts(transcripts):
    from radian_amd import map as rmap
    codes, off = _offsets(transcripts)
    return rmap.Transcripts(codes, off, [f"tx{t:03d}|gene{t}" for t in range(len(transcripts))])


def test_spans_equal_the_restatement_and_lie_at_the_true_ends(be, sim, capsys):
    """S and E of every read of the simulated set equal the restatement's (chain ends from _map_ref, pieces fitted by _fit_ref.fit_rows).
    On the unrelated transcripts the restatement's own S and E lie within 2 bases of the ends the read was drawn from (measured on
    this set: S - start in -2..2, E - end in -2..2, 146 reads); the bound asserted is that maximum, taken from the restatement at run time."""
    from radian_amd import map as rmap
    transcripts, reads, truth, hits, index = sim
    tr = _transcripts(transcripts)
    be.map_index(tr.codes, tr.offsets, 14, 8, 500)
    rows = rmap.map_records(be, tr, _records(reads), _args(**{"--batch-reads": 64}))
    worst, mine = 0, 0
    for i, (row, h, (t, start, end)) in enumerate(zip(rows, hits, truth)):
        S, E = mr.span(reads[i], transcripts[h["t"]], h)
        assert row["status"] == mr.OK and (row["t"], row["S"], row["E"]) == (h["t"], S, E), f"read {i}: {row} against {(h['t'], S, E)}"
        if t < 30:
            assert h["t"] == t
            worst = max(worst, abs(S - start), abs(E - end))
            mine = max(mine, abs(row["S"] - start), abs(row["E"] - end))
    with capsys.disabled():
        print(f"\n[test_gpu_map] span ends on the unrelated transcripts: restatement within {worst} bases of the truth, the GPU path within {mine}")
    assert mine <= worst


def _write_fasta(path, records, width=None):
    with open(path, "w") as f:
        for rid, seq in records:
            f.write(f">{rid}\n")
            if width:
                for a in range(0, len(seq), width):
                    f.write(seq[a: a + width] + "\n")
            else:
                f.write(seq + "\n")


def _run(args, cwd):
    p = subprocess.run([sys.executable, "-m", *args], cwd=cwd, capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONPATH": ROOT})
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_map_command_end_to_end(be, sim, tmp_path, capsys):
    from radian_amd import align as ralign, label_build
    transcripts, reads, truth, hits, index = sim
    records = _records(reads) + [("short", "ACGT"), ("withN", "ACGTNACGT" * 20), ("noise", "".join(LETTERS[c] for c in np.random.default_rng(3).integers(0, 4, 500)))]
    records[5] = (records[5][0], records[5][1].replace("T", "U"))
    d = str(tmp_path)
    _write_fasta(os.path.join(d, "reads.fasta"), records)
    _write_fasta(os.path.join(d, "tr.fa"), [(f"tx{t:03d}|gene{t} some text", "".join(LETTERS[c] for c in s)) for t, s in enumerate(transcripts)], width=60)
    out1 = _run(["radian_amd.map", "reads.fasta", "tr.fa", "-o", "a.tsv", "--mapped-fasta", "mapped.fasta", "--paf", "a.paf", "--stats", "a.stats"], d)
    _run(["radian_amd.map", "reads.fasta", "tr.fa", "-o", "b.tsv", "--batch-reads", "37", "--budget-bytes", str((1 << 20) + 64 * 3000), "--paf", "b.paf"], d)
    a = open(os.path.join(d, "a.tsv"), "rb").read()
    assert a == open(os.path.join(d, "b.tsv"), "rb").read() and open(os.path.join(d, "a.paf"), "rb").read() == open(os.path.join(d, "b.paf"), "rb").read()
    assert "reads: 303 seen, 300 mapped, 3 unmapped" in out1 and "non-ACGT: 1" in out1 and "N mapped reads: 300" in out1 and "N unmapped reads: 3" in out1
    # the file against the restatement's spans
    spans = [mr.span(reads[i], transcripts[h["t"]], h) for i, h in enumerate(hits)]
    exp = {f"read{i:04d}": "".join(LETTERS[c] for c in transcripts[h["t"]][S:E]) for i, (h, (S, E)) in enumerate(zip(hits, spans))}
    lines = a.decode().split("\n")
    assert lines[0] == "read_id\ttranscript\tsequence" and lines[-1] == "" and len(lines) == 302
    for i, line in enumerate(lines[1:-1]):
        rid, name, seq = line.split("\t")
        assert rid == f"read{i:04d}" and name == f"tx{hits[i]['t']:03d}|gene{hits[i]['t']}" and seq == exp[rid]
    assert label_build.read_ref_tsv(os.path.join(d, "a.tsv")) == exp == ralign.read_ref_tsv(os.path.join(d, "a.tsv"))
    paf = [ln.split("\t") for ln in open(os.path.join(d, "a.paf")).read().split("\n")[:-1]]
    assert len(paf) == 300 and all(len(c) == 15 and c[4] == "+" and c[11] == "255" for c in paf)
    for c, h, (S, E) in zip(paf, hits, spans):
        assert (int(c[7]), int(c[8]), c[12], c[13], c[14]) == (S, E, f"s1:i:{h['score']}", f"s2:i:{h['score2']}", f"cn:i:{h['n_anchors']}")
    # align on the result; its counts are Backend.align's of the restatement's spans, and so are --stats'
    _run(["radian_amd.align", "mapped.fasta", "a.tsv"], d)
    res = be.align([exp[f"read{i:04d}"] for i in range(300)], [records[i][1].replace("U", "T") for i in range(300)])
    want = [f"read{i:04d}\t{c[0]}\t{c[2]}\t{c[3]}\t{c[1]}" for i, c in enumerate(res.counts.tolist())]
    got = open(os.path.join(d, "mapped.tsv")).read().split("\n")
    assert got[0] == "read_id\tn_match\tn_ins\tn_del\tn_sub" and got[1:-1] == want
    stats = open(os.path.join(d, "a.stats")).read().split("\n")
    assert stats[0] == "read_id\tref_name\tn_match\tn_ins\tn_del\tn_sub"
    assert stats[1:-1] == [w.split("\t")[0] + f"\ttx{hits[i]['t']:03d}\t" + "\t".join(w.split("\t")[1:]) for i, w in enumerate(want)]
    with capsys.disabled():
        print("\n[test_gpu_map] the command's summary:\n" + out1)


def test_zz_duration_of_this_file(capsys):
    with capsys.disabled():
        print(f"\n[test_gpu_map] {time.perf_counter() - _T0:.1f} s for the whole file")
    assert time.perf_counter() - _T0 < 600
