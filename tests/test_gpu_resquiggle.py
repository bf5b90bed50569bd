"""GPU checks of the fused signal-to-reference route rd_resquiggle_raw (Backend.resquiggle_raw) against its parts and against
rd_basecall_raw_global_q, and of `python -m radian_amd.resquiggle` on tests/golden/reads.fast5.  Seeded synthetic weights with a soft head
(labelings of hundreds of bases), as tests/test_gpu_fastq.py.  Everything is compared for EXACT equality.

"A reference that is not the call" is the read's own call with 12 % substitutions / insertions / deletions (tests/_events_ref.mutate): none
of them may come back without a path."""
import json
import os
import shutil

import numpy as np
import pytest

import _events_ref as ref
from _events_cases import same_events

pytestmark = pytest.mark.gpu

CHUNK, STEP, CLIP, W = 1024, 128, 4, 6


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _soft_weights():
    from radian_amd import weights
    flat = weights.synthetic_weights(seed=1234)
    flat[-645:-5] *= np.float32(0.05)          # soft head: labelings of hundreds of bases
    return flat


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    b.load_weights(_soft_weights())
    yield b
    b.close()


@pytest.fixture(scope="module")
def reads(golden_dir, be):
    """a multi-window read (assembled float64 rows), a single-coverage read shorter than a chunk (float32 rows), a read of exactly chunk_len
    samples and two more multi-window reads; their own calls and the calls' forced alignments (rd_basecall_raw_global_q); the calls with
    12 % mutations"""
    ids = json.load(open(os.path.join(golden_dir, "reads_fast5_ids.json")))["read_ids"]
    sig = np.load(os.path.join(golden_dir, "reads_fast5_signals.npz"))
    raws = [np.ascontiguousarray(sig[ids[k]][a:b]) for k, (a, b) in enumerate([(0, 6000), (100, 800), (0, CHUNK), (500, 4863), (0, 3000)])]
    calls, status, aln = be.basecall_raw_global_q(raws, CLIP, CHUNK, STEP, W, False)
    assert status.tolist() == [0] * len(raws) and sum(len(c) for c in calls) > 300
    rng = np.random.default_rng(7)
    mutated = [np.array(ref.mutate(c, 0.12, rng), dtype=np.uint8) for c in calls]
    return raws, calls, aln, mutated


def _same_alignment(a, i, b, j):
    assert int(a.status[i]) == int(b.status[j]) and _bits(a.score[i]) == _bits(b.score[j])
    assert np.array_equal(a.first_step[i], b.first_step[j]) and np.array_equal(a.last_step[i], b.last_step[j])
    assert np.array_equal(a.qual[i], b.qual[j])


def _same_events(a, i, b, j):
    for name in ("start", "end", "sum", "sumsq", "min", "max"):
        assert np.array_equal(getattr(a, name)[i], getattr(b, name)[j]), name


def test_fused_route_equals_its_parts(be, reads):
    from radian_amd.backend import CTCALIGN_OK
    raws, calls, _, mutated = reads
    aln, ev, rst = be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP)
    assert rst.tolist() == [0] * len(raws)
    norm, nst = be.normalise_reads(raws, CLIP)
    assert nst.tolist() == [0] * len(raws)
    probs = be.forward_reads(norm, CHUNK, STEP)
    dtypes = []
    for r, p in enumerate(probs):
        N = len(raws[r])
        m = be.assemble(p, (p.shape[0] - 1) * STEP + CHUNK - N, STEP)
        assert m.shape == (N, 5)
        dtypes.append(m.dtype)
        one = be.ctc_align(m, [0], [N], [mutated[r]])
        _same_alignment(aln, r, one, 0)
        assert int(aln.status[r]) == CTCALIGN_OK and len(aln.qual[r]) == len(mutated[r])
        _same_events(ev, r, be.event_stats([raws[r]], one), 0)
        same_events(ev, r, ref.events(raws[r], one.first_step[0], one.last_step[0]))
    assert dtypes[0] == np.float64 and dtypes[1] == np.float32       # both kinds of rows were aligned


@pytest.mark.parametrize("logits", ["f32", "f16"])
def test_own_call_as_reference_equals_the_q_route(be, reads, logits):
    """with the read's own call as the labels, the fused route gives rd_basecall_raw_global_q's steps, qualities and score -- also with the
    softmax rows kept as f16 (whose parts no host-pointer call exposes)"""
    raws = reads[0]
    be.set_logits(logits)
    try:
        calls, status, q = be.basecall_raw_global_q(raws, CLIP, CHUNK, STEP, W, False)
        aln, ev, rst = be.resquiggle_raw(raws, calls, CLIP, CHUNK, STEP)
    finally:
        be.set_logits("f32")
    assert rst.tolist() == status.tolist()
    for r in range(len(raws)):
        _same_alignment(aln, r, q, r)
        same_events(ev, r, ref.events(raws[r], q.first_step[r], q.last_step[r], int(q.status[r])))
    if logits == "f32":
        for r in range(len(raws)):
            _same_alignment(q, r, reads[2], r)


def test_mutated_references_have_a_path_and_partition_the_signal(be, reads):
    from radian_amd.backend import CTCALIGN_OK
    raws, calls, _, mutated = reads
    assert any(len(m) != len(c) or (np.asarray(m) != np.asarray(c)).any() for m, c in zip(mutated, calls))
    aln, ev, _ = be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP)
    assert aln.status.tolist() == [CTCALIGN_OK] * len(raws)            # no no-path read at all
    for r in range(len(raws)):
        got = {k: [int(v) for v in getattr(ev, k)[r]] for k in ("start", "end", "n")}
        assert ref.partitions(got, aln.first_step[r], aln.last_step[r]), r
        assert all(0 <= s < e <= len(raws[r]) for s, e in zip(got["start"], got["end"]))


def test_reference_longer_than_the_read_and_a_budget_that_excludes_one_read(be, reads):
    from radian_amd.backend import CTCALIGN_NO_PATH, CTCALIGN_OK, CTCALIGN_TOO_LARGE, RadianHipError, ctc_align_workspace_bytes
    raws, calls, _, mutated = reads
    free, _ = be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP)[:2]
    # a reference longer than the read: no path, the neighbours unaffected
    labs = list(mutated)
    labs[1] = np.arange(len(raws[1]) + 5, dtype=np.uint8) % 4
    aln, ev, rst = be.resquiggle_raw(raws, labs, CLIP, CHUNK, STEP)
    assert aln.status.tolist() == [CTCALIGN_OK, CTCALIGN_NO_PATH, CTCALIGN_OK, CTCALIGN_OK, CTCALIGN_OK] and aln.score[1] == -np.inf
    assert aln.first_step[1].tolist() == [-1] * len(labs[1]) and ev.start[1].tolist() == ev.end[1].tolist() == [-1] * len(labs[1])
    assert not ev.sum[1].any() and not ev.sumsq[1].any() and not ev.min[1].any() and not ev.max[1].any() and not aln.qual[1].any()
    for r in (0, 2, 3, 4):
        _same_alignment(aln, r, free, r)
    # an empty reference is valid: the all-blank path, no events
    labs[1] = np.zeros(0, dtype=np.uint8)
    aln, ev, _ = be.resquiggle_raw(raws, labs, CLIP, CHUNK, STEP)
    assert int(aln.status[1]) == CTCALIGN_OK and len(ev.start[1]) == 0 and aln.score[1] < 0
    # a code above 3 is refused
    labs[1] = np.array([0, 4], dtype=np.uint8)
    with pytest.raises(RadianHipError):
        be.resquiggle_raw(raws, labs, CLIP, CHUNK, STEP)
    # a budget that excludes exactly the read with the largest workspace
    need = [ctc_align_workspace_bytes(len(x), len(m)) for x, m in zip(raws, mutated)]
    big = int(np.argmax(need))
    budget = sorted(need)[-2]
    assert budget < need[big]
    with pytest.raises(RadianHipError):
        be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP, budget_bytes=budget)
    aln, ev, _ = be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP, budget_bytes=budget, allow_too_large=True)
    assert [int(s) for s in aln.status] == [CTCALIGN_TOO_LARGE if r == big else CTCALIGN_OK for r in range(len(raws))]
    assert ev.start[big].tolist() == [-1] * len(mutated[big]) and not ev.sum[big].any()
    free_aln, free_ev = be.resquiggle_raw(raws, mutated, CLIP, CHUNK, STEP)[:2]
    for r in range(len(raws)):
        if r != big:
            _same_alignment(aln, r, free_aln, r)
            _same_events(ev, r, free_ev, r)


def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]


def test_cli_resquiggle(golden_dir, tmp_path, monkeypatch, capsys):
    from test_gpu_fastq import _read_fasta, _write_default_artifacts
    from radian_amd import basecall, resquiggle
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    shutil.copy(os.path.join(golden_dir, "reads.fast5"), str(in_dir / "reads.fast5"))
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    _write_default_artifacts(cwd, 1234, 3)
    monkeypatch.chdir(cwd)
    fa = tmp_path / "fa"
    fa.mkdir()
    basecall.main([str(in_dir), str(fa), "--context-len", "3"])
    capsys.readouterr()
    recs = _read_fasta(str(fa))
    assert len(recs) == 5
    # the TSV from basecall's own FASTA: one id removed, one span with an N
    spans = {rid: seq for rid, seq in recs}
    gone, with_n = recs[1][0], recs[3][0]
    spans[with_n] = spans[with_n][:3] + "N" + spans[with_n][3:]
    tsv = tmp_path / "read_ref.tsv"
    tsv.write_text("read_id\ttranscript\tspan\n" + "".join(f"{rid}\ttx{k}\t{spans[rid]}\n" for k, (rid, _) in enumerate(recs) if rid != gone))
    outs = {}
    for b in (1, 5):
        d = tmp_path / f"out{b}"
        st = resquiggle.main([str(in_dir), str(tsv), "-o", str(d), "--summary", str(d / "summary.tsv"), "--kmer-table", str(d / "kmers.tsv"),
                              "--kmer", "3", "--batch-reads", str(b)])
        out = capsys.readouterr().out
        assert (st["reads"], st["written"], st["ok"], st["no-reference"], st["has-N"]) == (5, 3, 3, 1, 1)
        assert st["no-path"] == st["too-large"] == st["signal"] == 0
        assert "reads: 5 seen, 3 written" in out and "status: ok: 3; no-reference: 1; has-N: 1; no-path: 0; too-large: 0; signal: 0" in out
        assert sorted(os.listdir(str(d))) == ["kmers.tsv", "reads.events.tsv", "summary.tsv"]
        outs[b] = {f: open(str(d / f), "rb").read() for f in os.listdir(str(d))}
    assert outs[1] == outs[5]                                    # byte-identical across --batch-reads
    rows = _tsv(str(tmp_path / "out5" / "reads.events.tsv"))
    assert tuple(rows[0]) == resquiggle.EVENT_COLUMNS
    ok = [(rid, seq) for rid, seq in recs if rid not in (gone, with_n)]
    at = 1
    for rid, seq in ok:                                          # one row per reference base of each ok read, in input order
        mine = rows[at: at + len(seq)]
        at += len(seq)
        assert [r[0] for r in mine] == [rid] * len(seq) and [int(r[2]) for r in mine] == list(range(len(seq)))
        assert "".join(r[3] for r in mine) == seq
        for r, nxt in zip(mine, mine[1:] + [None]):
            start, end, n = int(r[4]), int(r[5]), int(r[6])
            assert 0 <= start < end and n == end - start and float(r[8]) >= 0 and int(r[9]) <= float(r[7]) <= int(r[10]) and 0 <= int(r[12]) <= 50
            assert np.isfinite(float(r[11]))
            assert nxt is None or int(nxt[5]) == start          # start / end chain: the next base's event ends where this one begins
    assert at == len(rows) and st["bases"] == len(rows) - 1
    summ = _tsv(str(tmp_path / "out5" / "summary.tsv"))
    assert tuple(summ[0]) == resquiggle.SUMMARY_COLUMNS and [s[0] for s in summ[1:]] == [rid for rid, _ in recs]
    assert [s[1] for s in summ[1:]] == ["no-reference" if rid == gone else "has-N" if rid == with_n else "ok" for rid, _ in recs]
    for s in summ[1:]:
        if s[1] == "ok" and int(s[3]):
            assert float(s[4]) < 0 and 0 <= int(s[7]) <= int(s[8]) < int(s[2])
    kmers = _tsv(str(tmp_path / "out5" / "kmers.tsv"))
    assert tuple(kmers[0]) == resquiggle.KMER_COLUMNS and [k[0] for k in kmers[1:]] == sorted(k[0] for k in kmers[1:])
    assert sum(int(k[1]) for k in kmers[1:]) == sum(max(0, len(seq) - 2) for _, seq in ok)
