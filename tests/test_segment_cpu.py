"""No-GPU checks of event detection: the restatements of the contract (tests/_segment_ref.py) on toys worked by
hand and against each other, every seeded case's defining condition (tests/_segment_cases.py), rd_segment_host against the restatement,
the consequences the contract states (spacing, non-empty events, the event bound), the refusals, the workspace formula, the row rounding of
sigmap --events, the host code under the sanitizers as a stand-alone program (tests/asan_segment.cpp) and the detector's quality on
simulated reads.  Every comparison of integers is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _segment_cases as sc
import _segment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def groups():
    gs = sc.all_groups()
    for g in gs:
        g["exp"] = [ref.segment(x, g["p"]) for x in g["reads"]]
    return gs


def _params(p):
    from radian_amd.backend import SegmentParams
    return SegmentParams(**p)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_on_a_single_step_with_w1_2():
    """x = 0 0 0 0 10 10 10 10, w = 2, v0 = 1: the floor is 2 w^2 v0 = 8.  i = 2: both windows 0 0 -> N = 0, D = 8.  i = 3: 0 0 | 0 10 ->
    N = 2 * 10^2 = 200, D = (2 * 100 - 100) + 8 = 108.  i = 4: 0 0 | 10 10 -> N = 2 * 20^2 = 800, D = (2 * 200 - 400) + 8 = 8.  i = 5 mirrors
    i = 3, i = 6 mirrors i = 2.  th = 16 (t^2 >= 1): 3, 4 and 5 are candidates (t^2 = 1.85, 100, 1.85); 4 suppresses both"""
    x = np.array([0, 0, 0, 0, 10, 10, 10, 10], np.int16)
    p = ref.params(w1=2, w2=0, th1=16)
    assert ref.tstat(x, 2, 1) == ([0, 0, 0, 200, 800, 200, 0, 0], [1, 1, 8, 108, 8, 108, 8, 1])
    assert ref.flags(x, p)[0] == [0, 0, 0, 0, 1, 0, 0, 0]
    o = ref.segment(x, p)
    assert (o["status"], o["n_events"], o["start"], o["sum"], o["sumsq"], o["min"], o["max"], o["src"]) == (ref.OK, 2, [0, 4], [0, 40], [0, 400], [0, 10], [0, 10], [0, 1])
    assert ref.segment(x, dict(p, th1=1601)) ["n_events"] == 1 and ref.segment(x, dict(p, th1=1600))["n_events"] == 2     # 16 * 800 = 1600 * 8


def test_restatement_breaks_ties_towards_the_smaller_index():
    """x = 0 0 0 10 0 0 0, w = 2: every i in 2..5 has one 10 in one of its windows: N = 200, D = 108 four times.  2 has only zeros (t = 0)
    before it and ties behind it: a peak.  3, 4 and 5 have a tie before them: none"""
    x = np.array([0, 0, 0, 10, 0, 0, 0], np.int16)
    assert ref.tstat(x, 2, 1) == ([0, 0, 200, 200, 200, 200, 0], [1, 1, 108, 108, 108, 108, 1])
    assert ref.flags(x, ref.params(w1=2, w2=0, th1=16))[0] == [0, 0, 1, 0, 0, 0, 0]
    assert ref.segment_np(x, ref.params(w1=2, w2=0, th1=16))["start"] == [0, 2]


def test_every_case_meets_its_condition_and_the_twin_equals_the_plain_restatement(groups):
    seen = set()
    for g in groups:
        assert ref.params_ok(g["p"])
        for r, x in enumerate(g["reads"]):
            assert ref.segment_np(x, g["p"]) == g["exp"][r], (g["name"], r)
            seen.add(g["exp"][r]["status"])
        for r, c in g["cond"].items():
            assert c(g["exp"][r], g["reads"][r]), (g["name"], r)
    assert seen == {ref.OK, ref.EMPTY}     # TOO_LONG: test_refusals...; TOO_LARGE exists on the device only
    lens = sorted(len(x) for x in groups[0]["reads"])
    assert lens[:5] == [0, 1, 7, 8, 9] and {sc.TILE - 1, sc.TILE, sc.TILE + 1, 2 * sc.TILE - 1, 2 * sc.TILE + 1} <= set(lens)


def test_host_equals_the_restatement_on_every_case(groups):
    from radian_amd.backend import segment_host
    for g in groups:
        wins = [(len(x) // 4, len(x)) for x in g["reads"]]
        got = segment_host(g["reads"], _params(g["p"]), wins)
        for r, x in enumerate(g["reads"]):
            sc.same(got, r, g["exp"][r])
            want = ref.scale(x[wins[r][0]:wins[r][1]]) if wins[r][1] > wins[r][0] else (0, 0)
            assert (int(got.m2[r]), int(got.d4[r])) == want
        bare = segment_host(g["reads"], _params(g["p"]))
        assert not bare.m2.any() and not bare.d4.any()


def test_consequences_spacing_non_empty_events_and_the_bound(groups):
    n_kept2 = 0
    for g in groups:
        p = g["p"]
        for r, x in enumerate(g["reads"]):
            o, T = g["exp"][r], len(x)
            fl = ref.flags(x, p)[0] if T < 1000 else None
            k1 = [s for s, d in zip(o["start"], o["src"]) if d == 1]
            k2 = [s for s, d in zip(o["start"], o["src"]) if d == 2]
            if fl is not None:
                assert k1 == [i for i, f in enumerate(fl) if f & 1]     # every peak of detector 1 is a boundary
            assert all(b - a > p["w1"] for a, b in zip(k1, k1[1:]))
            assert all(b - a > p["w2"] for a, b in zip(k2, k2[1:]))
            assert all(abs(a - b) >= p["w2"] for a in k2 for b in k1)
            n_kept2 += len(k2)
            ends = o["start"][1:] + [T]
            assert all(e > s for s, e in zip(o["start"], ends))
            assert all(p["w1"] <= s <= T - p["w1"] for s in o["start"][1:])
            assert o["n_events"] <= ref.max_events(T, p["w1"])
    assert n_kept2 > 50
    # the bound is met: boundaries every w1 + 1 samples from w1 on (a square wave of period 2 (w1 + 1))
    w1 = 3
    x = np.tile(np.repeat([0, 100], w1 + 1), 40)[1:]
    o = ref.segment(x, ref.params(w1=w1, w2=0))
    assert o["start"][:4] == [0, 3, 7, 11] and o["n_events"] == len(x) // (w1 + 1) + 1 == ref.max_events(len(x), w1)


def test_refusals_statuses_and_the_workspace_formula():
    from radian_amd import _lib
    from radian_amd.backend import segment_max_events, segment_workspace_bytes
    L = _lib.load()
    good, bad = sc.refusal_cases()
    assert sc.raw_call(L.rd_segment_host, **good)[0] == 0
    for name, kw in bad:
        rc, outs = sc.raw_call(L.rd_segment_host, fill=77, **kw)
        assert rc == -1, name
        assert all((o == 77).all() for o in outs), name
    assert sc.raw_call(L.rd_segment_host, raw=None, off=None, p=good["p"], n_reads=0)[0] == 0
    # offsets that claim 2^30 + 1 samples behind a short read: TOO_LONG without a sample of it being read; 2^30 itself would be looked at
    x = sc.levels(np.random.default_rng(3), 300)
    rc, outs = sc.raw_call(L.rd_segment_host, raw=x, off=[0, 300, 300 + ref.MAX_T + 1, 300 + ref.MAX_T + 1], p=good["p"])
    assert rc == 0 and outs[0].tolist() == [ref.OK, ref.TOO_LONG, ref.EMPTY] and outs[1].tolist() == [ref.segment(x, good["p"])["n_events"], 0, 0]
    for T in (0, 1, 7, 2047, 2048, 2049, 10 ** 6, 1 << 30):
        for w1 in (2, 4, 32):
            assert segment_workspace_bytes(T, w1) == ref.workspace_bytes(T, w1) and segment_max_events(T, w1) == ref.max_events(T, w1)
    assert segment_workspace_bytes(-1, 4) == -1 and segment_workspace_bytes(5, 1) == -1 and segment_max_events(5, 33) == -1


def test_event_rows_round_half_up():
    from radian_amd.segment import event_rows
    sums = np.array([7, -7, -9, 5, 0, -32768 * 5, 32767 * 3, 1, -1], np.int64)
    ns = np.array([2, 2, 3, 3, 4, 5, 3, 2, 2], np.int64)
    got = event_rows(sums, ns)
    assert got.dtype == np.int16 and got.tolist() == [4, -3, -3, 2, 0, -32768, 32767, 1, 0]
    assert got.tolist() == [ref.event_row(int(s), int(n)) for s, n in zip(sums, ns)]
    rng = np.random.default_rng(9)
    ns = rng.integers(1, 40, 500)
    sums = np.array([int(rng.integers(-32768, 32768, n).sum()) for n in ns], np.int64)
    assert event_rows(sums, ns).tolist() == [ref.event_row(int(s), int(n)) for s, n in zip(sums, ns)]


def test_asan_segment_host(tmp_path):
    """tests/asan_segment.cpp: the host side of segment.hip (argument checks, the rules, the host twin) built with AddressSanitizer + UBSan
    as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_segment"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_segment.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "60"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 120 and int(last[2]) >= 800          # "<n> accepted <m> refused"


# ---------------------------------------------------------------------------------------------- the detector's quality on simulated reads
def quality(raw, truth, res_events, t_lo):
    """-> (events, bases, base starts with a boundary within 3 samples, events that hold two or more base starts) over the fragment"""
    starts = res_events["start"].astype(np.int64) + t_lo
    lo, hi = int(truth[0]), len(raw)
    inside = starts[(starts >= lo) & (starts < hi)]
    near = np.abs(inside[np.clip(np.searchsorted(inside, truth), 0, len(inside) - 1)] - truth)
    near = np.minimum(near, np.abs(inside[np.clip(np.searchsorted(inside, truth) - 1, 0, len(inside) - 1)] - truth))
    per_event = np.bincount(np.searchsorted(inside, truth, side="right"), minlength=len(inside) + 1)[1:]
    return len(inside), len(truth), int((near <= 3).sum()), int((per_event >= 2).sum())


def test_detector_quality_on_simulated_reads():
    """The 16 simulated reads of the eventalign accuracy test (tests/_eventalign_cases.py: fragments of 200 or 300 bases, mean dwell 30
    samples), `segment`'s default parameters, rd_segment_host from 32 samples before the fragment on.  MEASURED:
    see QUALITY below.  The floors are the measured values less one read's worth: 1 / 16 of the measured value."""
    import _eventalign_cases as ec
    from radian_amd.backend import SegmentParams, segment_host
    tot = np.zeros(4, np.int64)
    for seed in ec.SIM_SEEDS:
        raw, codes, t_lo, truth = ec.sim_read(seed)
        res = segment_host([raw[t_lo:]], SegmentParams())
        q = quality(raw, truth, res.events[0], t_lo)
        print(f"seed {seed}: events/base {q[0] / q[1]:.3f} found {q[2] / q[1]:.3f} merged {q[3] / q[0]:.3f}")
        tot += q
    per_base, found, merged = tot[0] / tot[1], tot[2] / tot[1], tot[3] / tot[0]
    print(f"pooled: events per base {per_base:.3f}, base starts with a boundary within 3 samples {found:.3f}, events with two or more base starts {merged:.3f}")
    m_per_base, m_found, m_merged = QUALITY
    assert per_base >= m_per_base * 15 / 16 and found >= m_found * 15 / 16 and merged <= m_merged * 17 / 16


# MEASURED on rd_segment_host with the defaults (w1 4, t1 2.5, w2 12, t2 5.0, floor 1), pooled over the 16 reads: 1.734 events per base, 0.822
# of the base starts with a boundary within 3 samples, 0.059 of the events holding two or more base starts
QUALITY = (1.734, 0.822, 0.059)


# ---------------------------------------------------------------------------------------------- sigmap --events on the host twins
def test_sigmap_events_accuracy_on_simulated_reads():
    """The panel and the reads of tests/test_sigmap_cpu.py's accuracy test (eight genes x three isoforms that share their last 600 bases, 16
    unrelated transcripts; 28 reads that extend at least 100 bases beyond the shared part, eight that end inside it) through the command's
    two passes with --events, on rd_segment_host and rd_sigmap_host, the defaults (256 events per pass).  Sample mode (2048 samples per
    pass, eight times the rows) gets 27 of the 28 right and is the reference.  MEASURED in event mode: 28 of 28 go
    to their isoform, span ends within -2 .. +23 bases (5') and -6 .. 0 bases (3') of the truth.  The floor is that count less one read;
    the ends get the five bases of margin the sample-mode test gives them.  Reads that end inside the shared part still tie."""
    import _sigmap_cases as smc
    from radian_amd import sigmap as cmd
    from radian_amd.backend import SegmentParams, SigmapPanel, segment_host, sigmap_host
    from radian_amd.simulate import standin_tables
    tr, gene = smc.accuracy_transcripts()
    reads = smc.accuracy_reads()
    panel = cmd.Panel(tr, smc.ACC_PAD)
    model = cmd.model_tables(smc.ACC_K, *standin_tables(smc.ACC_K, smc.ACC_MODEL_SEED)[:2])[0]
    packed = SigmapPanel(panel.codes, panel.off)
    sig = lambda raw, q_lo, q_hi, **kw: sigmap_host(raw, packed, model, q_lo, q_hi, **kw)
    seg = lambda raws: segment_host(raws, SegmentParams(), [(0, len(x)) for x in raws])
    args = smc.accuracy_args(query_events=256)
    rows = cmd.map_batch(sig, [(r["id"], r["raw"]) for r in reads], panel, {r["id"]: r["tail_end"] for r in reads}, args, seg)
    assert all(row["status"] == "ok" and row["T1"] == row["T2"] == 256 and row["n_events"] >= 512 for row in rows)
    counted = [(r, row) for r, row in zip(reads, rows) if r["beyond"]]
    right = [(r, row) for r, row in counted if panel.tr[row["j"]] == r["t"]]
    d5 = [row["S"] - r["start"] for r, row in right]
    d3 = [row["E"] - tr.length(r["t"]) for r, row in right]
    print("event mode: isoform right:", len(right), "of", len(counted), "5' end:", min(d5), max(d5), "3' end:", min(d3), max(d3))
    assert len(counted) == 28 and len(right) >= 27
    assert max(abs(d) for d in d5) <= 28 and max(abs(d) for d in d3) <= 11
    for r, row in zip(reads, rows):
        if not r["beyond"]:
            assert gene[panel.tr[row["j"]]] == gene[r["t"]] and row["n_tied"] == 3, r["id"]
    # the rows handed to rd_sigmap: the events' rounded means, in the order of the samples
    x = reads[0]["raw"][reads[0]["tail_end"] - 32:]
    arr, first, cnt, ev = cmd.event_arrays(seg, [x, x[:0], x])
    e = ev.events[0]
    ends = np.concatenate([e["start"][1:], [len(x)]])
    assert cnt.tolist() == [len(e["start"]), 0, len(e["start"])] and first.tolist() == [0, cnt[0], cnt[0]] and len(arr) == 2 * cnt[0]
    assert arr[:cnt[0]].tolist() == [ref.event_row(int(s), int(n)) for s, n in zip(e["sum"], ends - e["start"])]
