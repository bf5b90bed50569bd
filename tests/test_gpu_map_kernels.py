"""GPU checks of map.hip stage by stage, through the two diagnostic seams of include/radian_hip_diag.h (they launch the kernels rd_map_index
and rd_map_batch launch): the chain kernel on every segment of tests/_map_cases.py's chain set -- far winners at every i mod 64, ties across
the lane wrap, candidates at the limits -- against _map_ref.chain, every field of every segment; the minimizer kernel and the compaction on
images that put segment starts, breaks, short segments and tied hashes on the tile edges, against the library's host seed code and the
restatement; the split of a call of more than 65 535 reads into launches, through rd_map_batch; what the seams refuse.  Integer arithmetic
throughout: every comparison is array equality."""
import numpy as np
import pytest

import _map_cases as mc
import _map_ref as mr

pytestmark = pytest.mark.gpu

SEG_FIELDS = ("start", "score", "first", "count", "end")


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def _offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return (np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if off[-1] else np.zeros(0, dtype=np.uint8)), off


def _chain_mismatches(call, got, exp):
    out = []
    if got.shape != exp.shape:
        return [f"{call['name']}: {got.shape[0]} segments, the restatement has {exp.shape[0]}"]
    for s in np.flatnonzero((got != exp).any(axis=1)):
        c = int(np.flatnonzero(got[s] != exp[s])[0])
        out.append(f"{call['name']} (k {call['k']}, min_anchors {call['min_anchors']}, max_gap {call['max_gap']}, bandwidth {call['bandwidth']}): segment {s} of "
                   f"{len(call['segs'][s])} anchors: {SEG_FIELDS[c]} = {got[s, c]}, the restatement gives {exp[s, c]} "
                   f"(all fields {got[s].tolist()} against {exp[s].tolist()}; the chain ends at i mod 64 = {got[s, 4] % 64} against {exp[s, 4] % 64})")
    return out


def test_chain_kernel_equals_the_restatement_on_every_segment(be, capsys):
    calls = mc.chain_calls()
    bad, n_seg, n_anchors = [], 0, 0
    for call in calls:
        t, r, q = mc.arrays(call)
        got = be.map_diag_chain(t, r, q, call["k"], call["min_anchors"], call["max_gap"], call["bandwidth"])
        bad += _chain_mismatches(call, got, mc.expected(call))
        n_seg += len(call["segs"])
        n_anchors += len(t)
    with capsys.disabled():
        print(f"\n[test_gpu_map_kernels] chain kernel: {len(calls)} calls, {n_seg} segments, {n_anchors} anchors, {len(bad)} segments differ")
        for line in bad[:40]:
            print("  " + line)
    assert not bad, f"{len(bad)} segments differ from _map_ref.chain; the first: {bad[0]}"


def test_chain_seam_with_no_anchors_and_with_one(be):
    e = np.zeros(0, dtype=np.uint32)
    assert be.map_diag_chain(e, e, e, 14).shape == (0, 5)
    one = np.array([7], dtype=np.uint32)
    assert be.map_diag_chain(one, one, one, 14, min_anchors=1).tolist() == [[0, 14, 0, 1, 0]]
    assert be.map_diag_chain(one, one, one, 14, min_anchors=2).tolist() == [[0, 0, 0, 0, 0]]


@pytest.mark.parametrize("k, w", mc.SEEDS)
def test_minimizer_kernel_and_compaction_equal_the_host_twin_and_the_restatement(be, k, w):
    from radian_amd.backend import map_minimizers
    for name, recs in mc.minimizer_images(k, w):
        codes, off = _offsets(recs)
        got = be.map_diag_minimizers(codes, off, k, w)
        flat, starts = mc.flat_image(recs)
        assert starts == [int(off[r]) + r for r in range(len(recs))]
        twin = np.concatenate([map_minimizers(rec, k, w)[0].astype(np.int64) + s for rec, s in zip(recs, starts)])
        assert np.array_equal(got, twin), (f"k {k} w {w}, image '{name}' of {len(flat)} codes: the device gives {len(got)} positions, the host twin {len(twin)}; "
                                           f"only the device {sorted(set(got.tolist()) - set(twin.tolist()))[:8]}, only the twin {sorted(set(twin.tolist()) - set(got.tolist()))[:8]}")
        assert len(flat) <= 5001
        assert got.tolist() == [p for p, _ in mr.minimizers(flat, k, w)], (k, w, name)


def test_minimizer_seam_leaves_the_index_alone(be):
    rng = np.random.default_rng(9)
    transcripts = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (900, 1400, 700)]
    reads = [transcripts[1][200:900], transcripts[2][50:650], rng.integers(0, 4, size=500, dtype=np.uint8)]
    be.map_index(*_offsets(transcripts), 14, 8, 500)
    before = be.map_batch(reads)
    assert before.status.tolist() == [h["status"] for h in mr.map_reads(reads, transcripts)[0]] and before.status[0] == mr.OK
    be.map_diag_minimizers(*_offsets(reads), 9, 3)
    t = np.arange(3, dtype=np.uint32)
    be.map_diag_chain(t, t, t, 9, 1)
    after = be.map_batch(reads)
    assert np.array_equal(after.status, before.status) and np.array_equal(after.hits, before.hits)


def _split_case(n=66000):
    """(transcripts, reads, real, index, status, hits): n reads too short for a seed, except the ~200 at `real` -- the call's first two, 65 534
    (the last of the first launch), 65 535 and 65 536 (the first of the second), the last, and 194 drawn at random -- which are cut from
    the transcripts; status and hits by the restatement, which is run on the real reads only"""
    rng = np.random.default_rng(66000)
    p = mr.DEFAULTS
    transcripts = [rng.integers(0, 4, size=int(m), dtype=np.uint8) for m in rng.integers(600, 1500, size=8)]
    real = sorted({0, 1, 65534, 65535, 65536, n - 1} | {int(i) for i in rng.choice(n, size=194, replace=False)})
    reads = [rng.integers(0, 4, size=int(m), dtype=np.uint8) for m in rng.integers(0, p["k"], size=n)]
    for i in real:
        t = transcripts[int(rng.integers(0, len(transcripts)))]
        a = int(rng.integers(0, len(t) - 300))
        reads[i] = mr.mutate(rng, t[a: a + int(rng.integers(200, 300))], 0.08)
    index = mr.build_index(transcripts, p["k"], p["w"])
    status = np.full(n, mr.NO_SEED, dtype=np.int32)
    hits = np.zeros((n, 8), dtype=np.int32)
    for i in real:
        h = mr.map_read(reads[i], index, **p)
        status[i] = h["status"]
        hits[i] = [h[f] for f in mr.FIELDS]
    return transcripts, reads, real, index, status, hits


def test_a_call_of_66000_reads_is_split_at_65535_reads_per_launch(be):
    """the read's index within a launch is the sort key's top 16 bits, and the sort's last bit is derived from the launch's read count"""
    n, p = 66000, mr.DEFAULTS
    transcripts, reads, real, index, exp_status, exp_hits = _split_case(n)
    assert len(reads) == n and (exp_status[real] == mr.OK).sum() > 150 and all(exp_status[i] == mr.OK for i in (0, 1, 65534, 65535, 65536, n - 1))
    be.map_index(*_offsets(transcripts), p["k"], p["w"], p["max_occ"])
    codes, off = _offsets(reads)
    res = be.map_batch_flat(codes, off, p["min_anchors"], p["min_score"], p["max_gap"], p["bandwidth"], with_stats=True)
    wrong = np.flatnonzero((res.status != exp_status) | (res.hits != exp_hits).any(axis=1))
    assert wrong.size == 0, (f"{wrong.size} reads differ from the restatement, the first at index {wrong[0]}: status {res.status[wrong[0]]}, "
                             f"{res.hits[wrong[0]].tolist()} against {exp_status[wrong[0]]}, {exp_hits[wrong[0]].tolist()}")
    assert res.stats["launches"] == 2
    n_anchors = max(len(mr.anchors(reads[i], index, p["k"], p["w"], p["max_occ"])) for i in real)
    small = be.map_batch_flat(codes, off, p["min_anchors"], p["min_score"], p["max_gap"], p["bandwidth"], (1 << 20) + 64 * 3 * n_anchors, with_stats=True)
    assert small.stats["launches"] > 20
    assert np.array_equal(small.status, res.status) and np.array_equal(small.hits, res.hits)


def test_the_seams_refuse_what_they_do_not_take(be):
    from radian_amd import RadianHipError
    a = np.array([0, 0, 1, 1], dtype=np.uint32), np.array([5, 9, 2, 2], dtype=np.uint32), np.array([7, 3, 8, 9], dtype=np.uint32)
    assert be.map_diag_chain(*a, 14, 1).shape == (2, 5)
    for what, (t, r, q) in {"t descends": (a[0][::-1], a[1], a[2]), "r descends": (a[0], a[1][[1, 0, 2, 3]], a[2]),
                            "q descends": (a[0], a[1], a[2][[0, 1, 3, 2]]), "an anchor twice": (a[0], a[1], a[2][[0, 1, 2, 2]])}.items():
        with pytest.raises(RadianHipError, match="strictly ascending"):
            be.map_diag_chain(t, r, q, 14, 1)
    for col in range(3):
        big = [c.copy() for c in a]
        big[col][3] = 1 << 24
        with pytest.raises(RadianHipError, match="below 2\\^24"):
            be.map_diag_chain(*big, 14, 1)
        big[col][3] = (1 << 24) - 1   # the largest value is taken
        assert be.map_diag_chain(*big, 14, 1).shape[1] == 5
    for kw, word in (dict(k=7), "k = 7"), (dict(k=16), "k = 16"), (dict(min_anchors=0), "min_anchors"), (dict(max_gap=0), "max_gap"), (dict(bandwidth=-1), "bandwidth"):
        with pytest.raises(RadianHipError, match=word):
            be.map_diag_chain(*a, **dict(dict(k=14, min_anchors=1), **kw))
    codes, off = np.zeros(100, dtype=np.uint8), np.array([0, 40, 100], dtype=np.int64)
    assert be.map_diag_minimizers(codes, off, 8, 64).tolist() == [0, 41]   # two short homopolymer segments: the smallest position of each
    for (k, w), word in ((7, 8), "k = 7"), ((16, 8), "k = 16"), ((14, 0), "w = 0"), ((14, 65), "w = 65"):
        with pytest.raises(RadianHipError, match=word):
            be.map_diag_minimizers(codes, off, k, w)
