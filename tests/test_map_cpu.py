"""No-GPU checks of read-to-transcript mapping: the library's seed code (rd_map_minimizers, the host twin of the device's) against the
restatement of the contract (tests/_map_ref.py); the restatement itself against ground truth on the simulated set; the writers and the
argument checks of radian_amd.map; what the shared cases of tests/_map_cases.py (the inputs of tests/test_gpu_map_kernels.py) have to contain."""
import os

import numpy as np
import pytest

import _map_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from radian_amd import build, _lib
    build.build()
    return _lib.load()


def _twin(codes, k, w):
    from radian_amd.backend import map_minimizers
    pos, hs = map_minimizers(codes, k, w)
    return [(int(p), int(h)) for p, h in zip(pos, hs)]


def test_hash_is_the_contracts_and_invertible_on_2k_bits():
    import re
    header = open(os.path.join(ROOT, "include", "radian_hip.h")).read()
    c1 = int(re.search(r"#define RD_MAP_HASH_C1 (0x[0-9A-Fa-f]+)u", header).group(1), 16)
    c2 = int(re.search(r"#define RD_MAP_HASH_C2 (0x[0-9A-Fa-f]+)u", header).group(1), 16)
    assert (c1, c2) == (mr.C1, mr.C2) and c1 & 1 and c2 & 1
    assert int(re.search(r"#define RD_MAP_LOOKBACK (\d+)", header).group(1)) == mr.LOOKBACK
    for k in (8, 9):   # a bijection on 2k bits: checked in full where that is small
        hs = {mr.kmer_hash(x, k) for x in range(1 << (2 * k))}
        assert len(hs) == 1 << (2 * k) and max(hs) < 1 << (2 * k)


@pytest.mark.parametrize("k", range(8, 16))
def test_minimizers_equal_the_restatement(lib, k):
    rng = np.random.default_rng(100 + k)
    for w in (1, 2, 8, 19, 64):
        cases = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (0, 1, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w, 300, 1500)]
        cases += [np.full(200, c, dtype=np.uint8) for c in range(4)]                          # homopolymers
        cases += [np.tile(np.array([0, 1], dtype=np.uint8), 150), np.tile(np.array([2, 3, 1], dtype=np.uint8), 90)]
        broken = rng.integers(0, 4, size=900, dtype=np.uint8)
        broken[[0, 50, 51, 52 + k - 1, 52 + 2 * k, 400, 400 + k + w - 1, 899]] = 255          # segments of k - 1, k, k + w - 2 codes and longer
        broken[600:640] = 4
        cases += [broken, np.full(50, 255, dtype=np.uint8)]
        for codes in cases:
            assert _twin(codes, k, w) == mr.minimizers(codes, k, w), (k, w, len(codes))


def test_minimizer_definition_on_a_worked_example(lib):
    """every window's choice is in the set, nothing else is, and a short segment gives its single minimum"""
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 4, size=400, dtype=np.uint8)
    k, w = 10, 6
    got = dict(_twin(codes, k, w))
    hs = [mr.kmers(codes, k)[0][p][1] for p in range(400 - k + 1)]
    want = set()
    for s in range(len(hs) - w + 1):
        want.add(min(range(s, s + w), key=lambda p: (hs[p], p)))
    assert set(got) == want and all(got[p] == hs[p] for p in want)
    short = codes[: k + 2]
    (p, h), = _twin(short, k, w)
    assert h == min(hs[:3]) and p == hs[:3].index(h)
    from radian_amd import RadianHipError
    from radian_amd.backend import map_minimizers
    for bad in ((7, 8), (16, 8), (14, 0), (14, 65)):
        with pytest.raises(RadianHipError):
            map_minimizers(codes, *bad)


@pytest.fixture(scope="module")
def sim():
    transcripts, reads, truth = mr.simulate()
    hits, index = mr.map_reads(reads, transcripts)
    return transcripts, reads, truth, hits


def test_the_restatement_maps_the_simulated_set_to_the_truth(sim):
    """30 unrelated transcripts and 10 genes of three exon-skipping isoforms, 300 reads at 12 % error: no read unmapped; every read's
    transcript is the true one, or scores what the true one scores with score2 == score (an isoform tie)"""
    transcripts, reads, truth, hits = sim
    assert len(transcripts) == 60 and len(reads) == 300 and all(e - s >= 400 for _, s, e in truth)
    ties = 0
    for i, (h, (t, s, e)) in enumerate(zip(hits, truth)):
        assert h["status"] == mr.OK, f"read {i} of transcript {t} is unmapped (status {h['status']})"
        if h["t"] != t:
            assert t in h["chains"] and h["chains"][t][0] == h["score"] and h["score2"] == h["score"], (i, t, h)
            assert t >= 30 and h["t"] >= 30 and h["t"] < t
            ties += 1
        assert h["n_anchors"] >= 3 and h["score"] >= 40 and h["q0"] <= h["q1"] and h["r0"] <= h["r1"]
    assert ties < 60


def test_the_restatements_spans_reach_the_true_ends(sim):
    transcripts, reads, truth, hits = sim
    worst = 0
    for i in range(0, 300, 5):
        t, s, e = truth[i]
        if t >= 30:
            continue
        S, E = mr.span(reads[i], transcripts[t], hits[i])
        worst = max(worst, abs(S - s), abs(E - e))
    assert worst <= 8   # the chain ends alone are within the minimizer spacing; the fitted ends are far inside it


def test_chain_rules_on_small_cases():
    k = 14
    # colinear anchors 10 apart: each adds min(dq, dr, k) = 10
    seg = [(100 + 10 * i, 5 + 10 * i) for i in range(5)]
    assert mr.chain(seg, k, 1000, 500) == (14 + 40, 0, 5, 4)
    # a gap of |dr - dq| = 64 costs (64 * 14 >> 6) + (6 >> 1) = 17 > 14: the anchor starts its own chain, the first keeps the end (smallest i)
    assert mr.gap_cost(64, k) == 17 and mr.gap_cost(1, k) == 0 and mr.gap_cost(0, k) == 0
    assert mr.chain([(100, 5), (214, 55)], k, 1000, 500) == (14, 0, 1, 0)
    # max_gap and bandwidth cut predecessors off
    assert mr.chain([(100, 5), (1200, 1105)], k, 1000, 500)[2] == 1
    assert mr.chain([(100, 5), (700, 55)], k, 1000, 500)[2] == 1
    # look-back: 70 anchors on one q cannot chain (dq = 0); the one after them only sees the last 64
    seg = [(100, 50)] + [(200 + i, 60) for i in range(70)] + [(300, 70)]
    score, first, n, end = mr.chain(seg, k, 1000, 500)
    assert first != 0 and n == 2


def _rows_and_transcripts():
    from radian_amd import map as rmap
    codes = np.array([0, 1, 2, 3, 255, 0, 0, 1, 1, 2, 2, 3, 3], dtype=np.uint8)
    tr = rmap.Transcripts(codes, np.array([0, 8, 13]), ["ENST1|ENSG1|-|-|T-201|G|8|protein_coding|", "tx2"])
    rows = [{"id": "r1", "seq": "ACGUAA", "status": 0, "t": 0, "S": 1, "E": 7, "score": 41, "score2": 41, "n_anchors": 3},
            {"id": "r2", "seq": "NN", "status": -1},
            {"id": "r3", "seq": "AACCG", "status": 0, "t": 1, "S": 0, "E": 5, "score": 50, "score2": 0, "n_anchors": 4},
            {"id": "r4", "seq": "ACGT", "status": 2}]
    return rmap, tr, rows


def test_writers_round_trip(tmp_path):
    from radian_amd import align, label_build
    rmap, tr, rows = _rows_and_transcripts()
    args = rmap.check_args(rmap.build_parser().parse_args(["reads.fasta", "tr.fa", "-o", str(tmp_path / "o.tsv"), "--mapped-fasta", str(tmp_path / "m.fasta"),
                                                           "--paf", str(tmp_path / "o.paf")]))
    assert rmap.write_outputs(args, tr, rows) == ""
    want = {"r1": "CGTNAA", "r3": "CGGTT"}
    assert open(tmp_path / "o.tsv").read() == "read_id\ttranscript\tsequence\nr1\tENST1|ENSG1|-|-|T-201|G|8|protein_coding|\tCGTNAA\nr3\ttx2\tCGGTT\n"
    assert align.read_ref_tsv(str(tmp_path / "o.tsv")) == want == label_build.read_ref_tsv(str(tmp_path / "o.tsv"))
    assert align.read_fasta(str(tmp_path / "m.fasta")) == [("r1", "ACGUAA"), ("r3", "AACCG")]
    paf = [ln.split("\t") for ln in open(tmp_path / "o.paf").read().split("\n")[:-1]]
    assert paf[0] == ["r1", "6", "0", "6", "+", "ENST1|ENSG1|-|-|T-201|G|8|protein_coding|", "8", "1", "7", "6", "6", "255", "s1:i:41", "s2:i:41", "cn:i:3"]
    assert paf[1] == ["r3", "5", "0", "5", "+", "tx2", "5", "0", "5", "5", "5", "255", "s1:i:50", "s2:i:0", "cn:i:4"]
    assert rmap.stats_row(rows[0], tr, (5, 1, 0, 2)) == "r1\tENST1\t5\t0\t2\t1\n"
    text = rmap.summary(tr, {"entries": 7, "keys": 6, "keys_dropped": 1}, rows, {})
    assert "transcripts: 2 read, 2 kept; bases: 13" in text and "minimizers indexed: 7 on 6 keys; keys dropped by --max-occ: 1" in text
    assert "reads: 4 seen, 2 mapped, 2 unmapped (no-seed: 0, no-chain: 1, too-large: 0, empty-span: 0, non-ACGT: 1)" in text
    assert "ambiguous between transcripts (s2 = s1): 1" in text


def test_span_pieces_follow_the_rule():
    from radian_amd import map as rmap
    # a long read: the head is the piece that ends at q0 + k, the tail the piece that starts at q1
    head, tail = rmap.pieces(L=3000, n=5000, k=14, piece=512, q0=700, r0=1700, q1=2900, r1=3905)
    assert head == (202, 714, 1714 - 1024, 1714) and tail == (2900, 3000, 3905, 4105)
    # a short one near the transcript's ends: everything clamps
    head, tail = rmap.pieces(L=300, n=320, k=14, piece=512, q0=3, r0=5, q1=280, r1=290)
    assert head == (0, 17, 0, 19) and tail == (280, 300, 290, 320)


def test_fasta_names_follow_the_scanners_filter(tmp_path, lib):
    from radian_amd import map as rmap
    p = tmp_path / "t.fa"
    p.write_text(">A|x|y|z|a|b|c|protein_coding| extra words\nACGTNNAC\nGT\n>B|x|y|z|a|b|c|lncRNA|\nACGT\n>C one\r\nacgu\r\n")
    assert rmap.fasta_names(str(p)) == ["A|x|y|z|a|b|c|protein_coding|", "B|x|y|z|a|b|c|lncRNA|", "C"]
    tr = rmap.Transcripts.read(str(p), 7, "protein_coding")
    assert tr.names == ["A|x|y|z|a|b|c|protein_coding|"] and tr.info == {"records": 3, "kept": 1, "bases": 10}
    assert tr.letters(0, 0, 10) == "ACGTNNACGT"
    tr = rmap.Transcripts.read(str(p))
    assert tr.names[2] == "C" and tr.letters(2, 0, 4) == "ACGT"
    assert list(rmap.encode_read("ACGUacgtNx")) == [0, 1, 2, 3, 0, 1, 2, 3, 255, 255]


@pytest.mark.parametrize("argv, word", [
    (["--k", "7"], "--k"), (["--k", "16"], "--k"), (["--w", "0"], "--w"), (["--w", "65"], "--w"), (["--max-occ", "0"], "--max-occ"),
    (["--min-anchors", "0"], "--min-anchors"), (["--min-score", "-1"], "--min-score"), (["--max-gap", "0"], "--max-gap"),
    (["--bandwidth", "-1"], "--bandwidth"), (["--piece", "1025"], "--piece"), (["--piece", "0"], "--piece"), (["--batch-reads", "0"], "--batch-reads"),
    (["--budget-bytes", "-1"], "--budget-bytes"), (["--field", "3"], "--value"), (["--value", "x"], "--field"),
    (["--protein-coding", "--field", "7", "--value", "x"], "--protein-coding"), (["--paf", "o.tsv"], "--paf"), (["--stats", "reads.fasta"], "reads.fasta"),
])
def test_argument_errors_name_the_flag(argv, word):
    from radian_amd import map as rmap
    with pytest.raises(SystemExit) as ei:
        rmap.check_args(rmap.build_parser().parse_args(["reads.fasta", "tr.fa", "-o", "o.tsv"] + argv))
    assert word in str(ei.value)


def test_map_needs_the_gpu_library_only(lib):
    """the command has no CPU path: its mapping calls are the library's (no minimizer, chain or alignment code of its own)"""
    src = open(os.path.join(ROOT, "radian_amd", "map.py")).read()
    for call in ("be.map_index(", "be.map_batch(", "be.fit_batch(", "be.align("):
        assert call in src


# ---- the shared cases of tests/_map_cases.py: what they have to contain, from the restatement alone ---------------------------------------
def test_chain_cases_meet_their_conditions():
    """The chain set of tests/test_gpu_map_kernels.py is built to make the chain kernel's rarely taken paths common.  These are conditions on
    the generators, counted with an instrumented copy of _map_ref.chain's loop (_map_cases.steps): an edit that empties a case fails here."""
    import collections
    import _map_cases as mc
    calls = mc.chain_calls()
    assert sum(len(s) for c in calls for s in c["segs"]) <= 50000
    assert {c["k"] for c in calls} == {8, 15} and {1, 3, 65} <= {c["min_anchors"] for c in calls}
    limits = {(c["max_gap"], c["bandwidth"]) for c in calls}
    assert {(50, 10), (50, 0), (mr.DEFAULTS["max_gap"], mr.DEFAULTS["bandwidth"])} == limits
    lattices = [c for c in calls if c["name"].startswith("lattice x")]
    assert [len(c["segs"]) for c in lattices] == list(mc.SEGMENT_COUNTS)
    assert {len(s) for c in lattices for s in c["segs"]} == set(mc.LENGTHS)
    assert all({len(s) for s in c["segs"]} == set(mc.LENGTHS) for c in calls if c["min_anchors"] == 65)
    win, kinds, dds = collections.Counter(), collections.Counter(), set()
    tied = wrapped = beyond = equal_k = negative = 0
    for c in calls:
        k, G, B = c["k"], c["max_gap"], c["bandwidth"]
        for seg in c["segs"]:
            assert seg == sorted(set(seg)) and all(0 <= v < 1 << 24 for a in seg for v in a)
            st, res = mc.steps(seg, k, G, B)
            assert res == mr.chain(seg, k, G, B)   # the instrumented loop is the restatement's
            for s in st:
                li = s["i"] % 64
                if s["win"] is not None:
                    win[s["win"]] += 1
                if len(s["tied"]) >= 2:
                    tied += 1
                    wrapped += any(j % 64 > li for j in s["tied"]) and any(j % 64 < li for j in s["tied"])
                beyond += s["beyond"]
                equal_k += s["best"] == k
                negative += s["best"] is not None and s["best"] < 0
                for dr, dq, ok in s["pairs"]:   # a pair counts at a limit when that limit alone decides it
                    if ok:
                        dds.add(abs(dr - dq))
                    kinds["dq == max_gap"] += dq == G and ok
                    kinds["dr == max_gap"] += dr == G and ok
                    kinds["dq == max_gap + 1"] += dq == G + 1 and 0 < dr <= G and abs(dr - dq) <= B
                    kinds["dr == max_gap + 1"] += dr == G + 1 and 0 < dq <= G and abs(dr - dq) <= B
                    kinds["|dr - dq| == bandwidth"] += abs(dr - dq) == B and ok
                    kinds["|dr - dq| == bandwidth + 1"] += abs(dr - dq) == B + 1 and 0 < dq <= G and 0 < dr <= G
    assert all(win[d] >= 20 for d in range(1, 65)), {d: win[d] for d in range(1, 65) if win[d] < 20}
    assert max(win) == 64
    assert tied >= 100 and wrapped >= 30 and beyond >= 100 and equal_k >= 20 and negative >= 20, (tied, wrapped, beyond, equal_k, negative)
    assert len(kinds) == 6 and all(n >= 20 for n in kinds.values()), kinds
    assert set(range(1, 11)) <= dds


@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 62, 63, 64, 65, 66])
def test_planted_far_winners_are_what_they_claim(d):
    """the probe's only valid predecessor lies exactly d anchors back, the probes fall on every i mod 64, and beyond the look-back (65, 66)
    the probe starts a chain of its own although its target would have extended it"""
    import _map_cases as mc
    (call,) = [c for c in mc.chain_calls() if c["name"] == f"planted d{d}"]
    seg, probes = mc.planted(d)
    assert call["segs"] == [seg] and (call["max_gap"], call["bandwidth"]) == (50, 10) and d in mc.PLANTED_D
    assert sorted(i % 64 for i in probes) == list(range(64))
    st, (score, first, count, end) = mc.steps(seg, call["k"], 50, 10)
    for i in probes:
        assert all(dq <= 0 for dr, dq, ok in st[i]["pairs"][: d - 1])   # the decoys between the probe and its target
        if d <= 64:
            assert st[i]["pairs"][d - 1][2] and st[i]["win"] == d and st[i]["valid"] == 1
        else:
            assert st[i]["win"] is None and st[i]["valid"] == 0 and st[i]["beyond"]
    if d <= 64:   # one chain through every target and probe: a probe that misses its target shows in the segment's result
        assert (first, count, end) == (0, 2 * len(probes), probes[-1])
    else:
        assert (first, count, end) == (probes[0], 2, probes[0] + 1 + (d % 2))   # the next target, past the block's extra decoy where it has one


@pytest.mark.parametrize("k, w", [(8, 1), (8, 64), (15, 1), (15, 8), (15, 64)])
def test_minimizer_images_meet_their_conditions(lib, k, w):
    """sizes, tile edges and whole images as tests/test_gpu_map_kernels.py needs them, and on every image the library's host seed code
    equals the restatement (record by record, and the restatement on the flat image: a record's end is a break)"""
    import _map_cases as mc
    assert (k, w) in mc.SEEDS and len(mc.SEEDS) == 5
    images = dict(mc.minimizer_images(k, w))
    flats = {name: mc.flat_image(recs) for name, recs in images.items()}
    sizes = {len(f) for f, _ in flats.values()}
    assert {1, k - 1, k, 1023, 1024, 1025, 2047, 2048, 2049, 3072} <= sizes
    kmer_at = lambda f, p: p + k <= len(f) and (f[p: p + k] <= 3).all()
    for edge in (1024, 2048):
        for p in (edge - 1, edge, edge + 1):
            f, starts = flats[f"segment starts at {p}"]
            assert starts[1] == p and f[p - 1] == 255 and kmer_at(f, p)
        for p in (edge - 1, edge):
            f, _ = flats[f"break at {p}"]
            assert f[p] == 255 and kmer_at(f, p - k) and kmer_at(f, p + 1)
        if w > 1:
            f, _ = flats[f"{w - 1} k-mers across {edge}"]
            (seg,) = [s for s in mr.kmers(f, k) if s[0][0] < edge <= s[-1][0] + k - 1 and len(s) < w]
            assert len(seg) == w - 1 and seg[0][0] < edge < seg[-1][0] + k
        f, _ = flats[f"homopolymer across {edge}"]
        run = f[edge - (w + k): edge + (w + k)]
        assert (run == run[0]).all() and run[0] <= 3
        picked = [p for p, _ in mr.minimizers(f, k, w) if edge - (w + k) <= p < edge + w]
        assert edge - 1 in picked and edge in picked   # equal hashes: every window's smallest position, on both sides of the edge
    assert (flats["all breaks"][0] == 255).all() and mr.minimizers(flats["all breaks"][0], k, w) == []
    if w == 1:
        f, _ = flats["every k-mer flagged"]
        assert len(mr.minimizers(f, k, w)) == len(f) - k > 4096
    for name, recs in images.items():
        f, starts = flats[name]
        assert len(f) <= 5001
        twin = [(s + p, h) for s, rec in zip(starts, recs) for p, h in _twin(rec, k, w)]
        assert twin == mr.minimizers(f, k, w), (name, k, w)
