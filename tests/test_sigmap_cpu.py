"""No-GPU checks of sigmap: the plain-Python restatement of the contract (tests/_sigmap_ref.py) by hand on toys, its
NumPy twin against it, every seeded case's defining condition (tests/_sigmap_cases.py), the stripe argument the kernel rests on,
rd_sigmap_host against the restatement on every case, every refusal, the workspace formula, and the host side of rd_sigmap under the
sanitizers as a stand-alone program (tests/asan_sigmap.cpp).  Every comparison of integers is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _sigmap_cases as sc
import _sigmap_ref as ref
from _eventalign_ref import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def toy_panel():
    """k = 1: A at 0, C at 10, G at 20, T at 30; w = 2^30, so a cell costs floor(d^2 / 4); no bias.  Two targets of three states:
    ACG (levels 0 10 20, states 0 1 2) and GAT (20 0 30, states 3 4 5)"""
    return ref.Panel([[0, 1, 2], [2, 0, 3]], Model(1, [0, 10, 20, 30], [1 << 30] * 4, [0] * 4, (0, 0, 0)))


def toy(x, s_lo=0, s_hi=6, n_best=2, **kw):
    # m2 = 0, d4 = 1024: u = 1024 x, zq = floor((2048 x + 1024) / 2048) = x
    return ref.map_plain(np.array(x, dtype=np.int16), toy_panel(), 0, len(x), 0, len(x), 0, 1024, s_lo, s_hi, n_best, **kw)


def test_restatement_on_two_targets_three_states_three_rows():
    """Rows 0, 10, 20.  Costs per row: [0 25 100 | 100 0 225], [25 0 25 | 25 25 100], [100 25 0 | 0 100 25].
    V0 = [0 25 100 | 100 0 225]
    V1 = [25, 0 (from 0), 50 (from 1) | 125 (a head: stays), 25 (100 is not smaller than 0: stays), 100 (from 4)]   O1 = [0 0 1 | 3 4 4]
    V2 = [125, 25 (25 is not smaller than 0), 0 (from 1) | 125 (a head: 50 to its left is another target's), 125, 50 (from 4)]   O2 = [0 0 0 | 3 4 4]"""
    o = toy([0, 10, 20], keep_final=True)
    assert o["final"] == [125, 25, 0, 125, 125, 50] and o["final_org"] == [0, 0, 0, 3, 4, 4]
    assert (o["status"], o["tgt"], o["score"], o["end"], o["org"]) == (ref.OK, [0, 1], [0, 50], [2, 2], [0, 1])
    # were the path allowed across the join, state 3 would take 50 from state 2 and target 1 would end in its first state
    j = toy([0, 10, 20], join=True, keep_final=True)
    assert j["final"][3] == 50 and j["final_org"][3] == 1
    # s_lo inside target 0: states 1 .. 4.  V0 = [25 100 | 100 0]; V1 = [25 (a head), 50 (from 1) | 125, 25]; V2 = [50, 25 (from 1) | 125, 125]:
    # target 1 ties with itself and ends in the smaller state
    o = toy([0, 10, 20], 1, 5, keep_final=True)
    assert o["final"] == [50, 25, 125, 125] and o["final_org"] == [1, 1, 3, 4]
    assert (o["tgt"], o["score"], o["end"], o["org"]) == ([0, 1], [25, 125], [2, 0], [1, 0])
    # one row: both targets hold a state on the sample's level: the tie between targets goes to the smaller index
    o = toy([0], n_best=3)
    assert (o["tgt"], o["score"], o["end"], o["org"]) == ([0, 1, -1], [0, 0, -1], [0, 1, -1], [0, 1, -1])
    # n_best = 1; a range of one state; the statuses
    assert toy([0, 10, 20], n_best=1)["tgt"] == [0] and toy([0, 10, 20], 4, 5)["end"] == [1, -1]
    assert toy([])["status"] == ref.EMPTY and toy([1, 2], 3, 3)["status"] == ref.NO_TARGET
    assert ref.map_plain(np.full(9, 5, dtype=np.int16), toy_panel(), 0, 9, 0, 9, 0, 0, 0, 6, 1)["status"] == ref.MAD_ZERO


def test_twin_equals_plain():
    small = sc.small_cases()
    assert len(small) >= 12
    for c in small:
        a = ref.map_plain(sc.raw(), sc.panel(), c["q_lo"], c["q_hi"], c["sc_lo"], c["sc_hi"], c["m2"], c["d4"], c["s_lo"], c["s_hi"], sc.N_BEST)
        assert a == sc.reference(c), c["name"]


def test_every_case_meets_its_condition():
    p = sc.panel()
    assert 0 in [len(t) for t in p.targets[1:-1]] and 1 in [len(t) for t in p.targets] and p.R < 60000
    from _eventalign_ref import kmer
    used = {kmer(t, b, sc.K) for t in p.targets for b in range(len(t))}
    assert {0, 63} <= used and sc.MODEL.w[0] == 2 ** 32 - 1 and sc.MODEL.w[63] == 0 and min(sc.MODEL.bias) == -256     # the ends of the ranges are met
    for c in sc.all_cases():
        assert sc.cells(c) <= 3e7, c["name"]
        assert c["cond"](sc.reference(c)), (c["name"], {k: v for k, v in sc.reference(c).items()})
    rows = {c["q_hi"] - c["q_lo"] for c in sc.all_cases()}
    assert {0, 1, 2, 15, 16, 17, 127, 128, 129, 300, 1 << 14, (1 << 14) + 1} <= rows
    ranges = {c["s_hi"] - c["s_lo"] for c in sc.all_cases()}
    assert set(sc.LENGTHS) | {0, 1} <= ranges
    assert {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_TARGET} == {sc.reference(c)["status"] for c in sc.all_cases()}


def test_a_stripe_alone_equals_the_whole_dp_on_its_ends():
    """What the kernel rests on: the states [a - (T - 1), b) computed alone, the first of them a head, give row T - 1 of the whole range's DP
    on [a, b) -- values and origins"""
    p, raw = sc.panel(), sc.raw()
    for name in ("panel_given", "L6146_T300", "s_lo_inside", "join"):
        c = next(x for x in sc.all_cases() if x["name"] == name)
        T, lo, hi = c["q_hi"] - c["q_lo"], c["s_lo"], c["s_hi"]
        args = (raw, p, c["q_lo"], c["q_hi"], c["sc_lo"], c["sc_hi"], c["m2"], c["d4"])
        whole = ref.map_numpy(*args, lo, hi, 1, keep_final=True)
        for a, b in ((lo + 1, min(lo + 50, hi)), (lo + T - 1, min(lo + T + 30, hi)), (max(lo, hi - 77), hi), (lo + (hi - lo) // 2, lo + (hi - lo) // 2 + 1)):
            left = max(lo, a - (T - 1))
            part = ref.map_numpy(*args, left, b, 1, keep_final=True)
            assert part["final"][a - left:] == whole["final"][a - lo:b - lo], (name, a, b)
            assert part["final_org"][a - left:] == whole["final_org"][a - lo:b - lo], (name, a, b)
        # and one state too few in front is not enough in general: the argument is tight only as a bound, so nothing is asserted there


# ---------------------------------------------------------------------------------------------- the host twin
def test_host_equals_the_restatement_on_every_case():
    from radian_amd.backend import sigmap_host
    cases = sc.all_cases()
    res = sigmap_host(sc.raw(), sc.backend_panel(), sc.backend_model(), n_best=sc.N_BEST, **sc.call_args(cases))
    for q, c in enumerate(cases):
        ref.assert_query_equal(res, q, sc.reference(c), c["name"])
    # another n_best, another order
    sub = [c for c in cases if sc.cells(c) <= 2e6][::-1]
    for nb in (1, 3):
        res = sigmap_host(sc.raw(), sc.backend_panel(), sc.backend_model(), n_best=nb, **sc.call_args(sub))
        for q, c in enumerate(sub):
            want = sc.reference(c)
            ref.assert_query_equal(res, q, {k: (v[:nb] if isinstance(v, list) else v) for k, v in want.items()}, c["name"])


def test_host_on_the_toys():
    from radian_amd.backend import EvalModel, sigmap_host
    m = EvalModel(1, [0, 10, 20, 30], [1 << 30] * 4, [0] * 4, (0, 0, 0))
    tg = [np.array([0, 1, 2], np.uint8), np.array([2, 0, 3], np.uint8)]
    res = sigmap_host(np.array([0, 10, 20], np.int16), tg, m, [0, 0, 0], [3, 3, 1], m2=[0] * 3, d4=[1024] * 3, s_lo=[0, 1, 0], s_hi=[6, 5, 6], n_best=3)
    assert res.tgt.tolist() == [[0, 1, -1]] * 3 and res.score.tolist() == [[0, 50, -1], [25, 125, -1], [0, 0, -1]]
    assert res.end.tolist() == [[2, 2, -1], [2, 0, -1], [0, 1, -1]] and res.org.tolist() == [[0, 1, -1], [1, 0, -1], [0, 1, -1]]
    # two targets in a tuple are two targets, never a packed pair
    two = sigmap_host(np.array([0, 10, 20], np.int16), tuple(tg), m, [0], [3], m2=[0], d4=[1024], n_best=3)
    assert two.tgt.tolist() == [[0, 1, -1]] and two.score.tolist() == [[0, 50, -1]]


def test_refusals():
    from radian_amd.backend import EvalModel, RadianHipError, SigmapPanel, sigmap_host
    m = EvalModel(1, [0, 10, 20, 30], [1 << 30] * 4, [0] * 4, (0, 0, 0))
    tg = [np.array([0, 1, 2], np.uint8), np.array([2, 0, 3], np.uint8)]
    x = np.array([0, 10, 20], np.int16)
    ok = dict(q_lo=[0], q_hi=[3], m2=[0], d4=[1024], s_lo=[0], s_hi=[6], n_best=2)
    assert sigmap_host(x, tg, m, **ok).status.tolist() == [0]
    assert sigmap_host(x, tg, m, [], [], n_best=1).status.size == 0                                  # no query is no error
    bad_model = EvalModel(1, [0, 10, 20, 1 << 14], [1 << 30] * 4, [0] * 4, (0, 0, 0))
    bad_bias = EvalModel(1, [0, 10, 20, 30], [1 << 30] * 4, [0, 0, 257, 0], (0, 0, 0))
    for what, kw, tgs, mdl in (("n_best 0", dict(n_best=0), tg, m), ("n_best 9", dict(n_best=9), tg, m),
                               ("window out of order", dict(q_lo=[2], q_hi=[1]), tg, m), ("window past the samples", dict(q_hi=[4]), tg, m),
                               ("negative window", dict(q_lo=[-1]), tg, m), ("scale window past the samples", dict(sc_lo=[0], sc_hi=[4]), tg, m),
                               ("scale window out of order", dict(sc_lo=[2], sc_hi=[1]), tg, m),
                               ("range out of order", dict(s_lo=[4], s_hi=[3]), tg, m), ("range past the states", dict(s_hi=[7]), tg, m),
                               ("negative range", dict(s_lo=[-1]), tg, m), ("d4 negative", dict(d4=[-1]), tg, m),
                               ("d4 too large", dict(d4=[(1 << 20) + 1]), tg, m), ("m2 too large", dict(m2=[(1 << 17) + 1]), tg, m),
                               ("a code above 3", {}, [tg[0], np.array([2, 4, 3], np.uint8)], m), ("a level out of range", {}, tg, bad_model),
                               ("a bias out of range", {}, tg, bad_bias),
                               ("offsets not monotone", {}, SigmapPanel(np.zeros(6, np.uint8), [0, 4, 3, 6]), m),
                               ("offsets not from 0", {}, SigmapPanel(np.zeros(6, np.uint8), [1, 3, 6]), m)):
        with pytest.raises(RadianHipError):
            sigmap_host(x, tgs, mdl, **{**ok, **kw})
            pytest.fail(what)
    with pytest.raises(ValueError):
        sigmap_host(x, tg, m, [0, 0], [3], n_best=1)


def test_workspace_formula():
    """rd_sigmap_workspace_bytes is the header's closed formula"""
    from radian_amd.backend import SIGMAP_BAND, SIGMAP_PAYLOAD, sigmap_workspace_bytes
    r = lambda v: (v + 255) // 256 * 256
    P = SIGMAP_PAYLOAD
    assert (P, SIGMAP_BAND) == (6145, 4096)
    for T in (1, 2, 63, 64, 65, 300, 2048, 1 << 14):
        for n in (1, 16, 4096, 4097, P - 1, P, P + 1, 2 * P, 2 * P + 1, 10 ** 6):
            for nt in (1, 32, 33, 5000):
                cols = -(-n // P) * r(16 * T) if min(n, P + T - 1) > SIGMAP_BAND else 0
                assert sigmap_workspace_bytes(T, n, nt) == r(4 * T) + r(4 * n) + r(8 * nt) + cols, (T, n, nt)
    assert sigmap_workspace_bytes(0, 0, 0) == 0 and sigmap_workspace_bytes(-1, 5, 1) == -1
    txt = open(os.path.join(ROOT, "radian_amd", "csrc", "sigmap_rules.h")).read()
    assert f"SM_PAYLOAD = {P};" in txt and f"SM_BAND = {SIGMAP_BAND};" in txt                       # the mirrored constants


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_sigmap_host(tmp_path):
    """tests/asan_sigmap.cpp: the host side of sigmap.hip (argument checks, the rules, the host twin) built with AddressSanitizer + UBSan
    as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_sigmap"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_sigmap.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "60"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 60 and int(last[2]) >= 600          # "<n> accepted <m> refused"


# ---------------------------------------------------------------------------------------------- the command's two passes, on the host twin
def test_span_orientation_and_pad_clipping():
    from radian_amd import sigmap as cmd
    from radian_amd.map import Transcripts
    tr = Transcripts(np.array([0, 1, 2, 3, 3, 2, 1, 0, 1, 1, 4, 2], np.uint8), np.array([0, 5, 5, 10, 12]), ["a", "empty", "b", "has_n"])
    p = cmd.Panel(tr, 3)
    assert p.tr == [0, 2] and p.skipped == 2 and p.off.tolist() == [0, 8, 16] and p.states == 16
    assert p.codes.tolist() == [0, 0, 0, 3, 3, 2, 1, 0, 0, 0, 0, 1, 1, 0, 1, 2]      # the pad, then the transcript as the pore sees it: reversed
    # state pad + i is base L - 1 - i: origin state 3 (the 3' end) .. end state 7 (the 5' end) is the whole transcript
    assert p.span(0, 3, 7) == (0, 5) and p.span(0, 4, 6) == (1, 4) and p.span(1, 5, 5) == (2, 3)
    assert p.span(0, 0, 7) == (0, 5) and p.span(0, 1, 2) == (4, 5)                   # states of the pad are clipped to the 3' end
    row = dict(id="r", j=1, S=1, E=4, n=900, t_lo=100, score=-7, score2=-1, n_cand=1, n_tied=1)
    assert cmd.tsv_row(row, p) == "r\tb\tCAC\n"
    assert cmd.paf_row(row, p) == "r\t900\t100\t900\t+\tb\t5\t1\t4\t3\t3\t255\ts1:i:-7\ts2:i:-1\tcn:i:1\tnt:i:1\n"


def test_two_pass_composition_and_accuracy_on_simulated_reads():
    """Reads simulated from fragments of a panel of eight genes x three isoforms that share their last 600 bases, plus 16 unrelated
    transcripts (tests/_sigmap_cases.py), through the command's two passes on rd_sigmap_host.  MEASURED on the host twin with 2048-sample
    queries: of the 28 reads that extend at least 100 bases beyond the shared part, 27 go to their isoform (the
    28th, whose own median is 0.12 z off, goes to an unrelated transcript: sigmap does not refit the scale); the span ends of the 27 are
    within -26 .. +4 bases (5' end, the free end of the second pass) and -1 .. 0 bases (3' end) of the truth.  The floors are these with a
    margin of one read and five bases.  The eight reads that end inside the shared part tie between their gene's three isoforms."""
    from radian_amd.backend import SIGMAP_OK
    tr, gene = sc.accuracy_transcripts()
    reads = sc.accuracy_reads()
    panel, rows = sc.accuracy_rows()
    assert [r["status"] for r in rows[-2:]] == ["no-bound", "no-bound"] and "j" not in rows[-1]
    counted = [(r, row) for r, row in zip(reads, rows) if r["beyond"]]
    assert len(counted) >= 24 and all(row["status"] == "ok" for row in rows[:-2])
    right = [(r, row) for r, row in counted if panel.tr[row["j"]] == r["t"]]
    d5 = [row["S"] - r["start"] for r, row in right]
    d3 = [row["E"] - tr.length(r["t"]) for r, row in right]
    print("isoform right:", len(right), "of", len(counted), "5' end:", min(d5), max(d5), "3' end:", min(d3), max(d3))
    assert len(counted) == 28 and len(right) >= 26
    assert max(abs(d) for d in d5) <= 31 and max(abs(d) for d in d3) <= 6
    for r, row in right:
        assert row["n_tied"] == 1 and row["n_cand"] >= 3 and row["score2"] > row["score"]      # the other isoforms were candidates: pass 1 ties them
    for r, row in zip(reads, rows):
        if not r["beyond"]:
            assert gene[panel.tr[row["j"]]] == gene[r["t"]] and row["n_tied"] == 3 and row["score2"] == row["score"], r["id"]
            assert panel.tr[row["j"]] == gene[r["t"]] * sc.ACC_ISOFORMS                           # the smaller index on ties
    # the rows' arithmetic: both windows, the sum, the span's letters
    for r, row in zip(reads, rows):
        n = len(r["raw"])
        assert row["t_lo"] == r["tail_end"] - 32 and row["T1"] == row["T2"] == sc.ACC_QUERY and row["score"] == row["s1"] + row["s2"] and n > 2 * sc.ACC_QUERY
        assert 0 <= row["S"] < row["E"] <= tr.length(panel.tr[row["j"]])
