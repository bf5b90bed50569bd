"""No-GPU checks of eventalign on event rows: the plain-Python restatement of the contract
(tests/_eventalign_events_ref.py) by hand on toys, its NumPy twin against it, every seeded case's defining condition
(tests/_eventalign_events_cases.py), rd_eventalign_events_host against the restatement on every case and every refusal, the identity with
rd_eventalign_host when every sample is an event and skips are off, the host code under the sanitizers as a stand-alone program
(tests/asan_eventalign_events.cpp) and the accuracy of the restatement on simulated reads.  Every comparison of integers is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _eventalign_cases as sc
import _eventalign_events_cases as ec
import _eventalign_events_ref as ref
import _eventalign_ref as sref
import _segment_ref as seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W100 = 16 * 2 ** 32 // 10000          # sd 100
W_BG = 16 * 2 ** 32 // (380 * 380)    # sd 380


def toy_model():
    """k = 1: A at -1000, C at +1000, G and T at 0; sd 100 and bias -43 each; the background at 0 with sd 380 and bias 0"""
    return ref.Model(1, [-1000, 1000, 0, 0], [W100] * 4, [-43] * 4, (0, W_BG, 0))


def toy(levels, ns, codes, pen, off=0):
    # m2 = 0, d4 = 1024: zq = x
    x = np.repeat(levels, ns)
    ev = ref.events_of(x, np.concatenate([[0], np.cumsum(ns)[:-1]]))
    return ref.align_plain(ev, len(x), codes, toy_model(), 0, 1024, pen, off)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_on_two_bases_and_three_events():
    """A then C, events of 2, 3 and 4 samples on A's level, C's level and the background's: a row on its state's level costs n times the
    bias, -43; the trail at the background's level costs 0.  Score 2 * -43 + 3 * -43."""
    assert ref.row_mean(7, 2) == 4 and ref.row_mean(-7, 2) == -3 and ref.row_mean(6, 4) == 2 and ref.row_mean(-6, 4) == -1   # halves round up
    o = toy([-1000, 1000, 0], [2, 3, 4], [0, 1], 96, off=100)
    assert (o["status"], o["score"], o["n_skipped"]) == (ref.OK, -215, 0)
    assert (o["row_first"], o["row_last"], o["start"], o["end"]) == ([0, 1], [0, 1], [100, 102], [102, 105])
    assert (o["sum"], o["sumsq"], o["min"], o["max"]) == ([-2000, 3000], [2 * 10 ** 6, 3 * 10 ** 6], [-1000, 1000], [-1000, 1000])
    assert o["sums"] == [5, 1000, 5 * 10 ** 6, 1000, 5 * 10 ** 6]
    # the weight: the same three levels with other counts
    assert toy([-1000, 1000, 0], [5, 1, 1], [0, 1], 96)["score"] == 6 * -43
    # without skips nothing changes here
    assert toy([-1000, 1000, 0], [2, 3, 4], [0, 1], -1, off=100) == o


def test_restatement_on_three_bases_and_two_events_needs_a_skip():
    """A G C on two events, A's level and C's: row 1 reaches state 3 only from state 1, over G.  The skipped base has no rows, its start
    and end are the start of the row that jumped over it, and it adds nothing to the sums."""
    o = toy([-1000, 1000], [2, 3], [0, 2, 1], 96)
    assert (o["status"], o["score"], o["n_skipped"]) == (ref.OK, -215 + 96, 1)
    assert (o["row_first"], o["row_last"], o["start"], o["end"]) == ([0, -1, 1], [0, -1, 1], [0, 2, 2], [2, 2, 5])
    assert (o["sum"], o["min"], o["max"]) == ([-2000, 0, 3000], [-1000, 0, 1000], [-1000, 0, 1000])
    assert o["sums"] == [5, 1000, 5 * 10 ** 6, 1000, 5 * 10 ** 6]
    assert toy([-1000, 1000], [2, 3], [0, 2, 1], 0)["score"] == -215 and toy([-1000, 1000], [2, 3], [0, 2, 1], 256)["score"] == -215 + 256
    assert toy([-1000, 1000], [2, 3], [0, 2, 1], -1)["status"] == ref.NO_PATH           # E < L without skips
    assert toy([-1000, 1000], [2, 3], [0, 2, 1, 0], 96)["status"] == ref.NO_PATH        # 2 E - 1 < L with them
    # lead to base 2 is a skip of base 1: the first event on the background's level, then C's; A is jumped over at row 1
    o = toy([0, 1000], [4, 3], [0, 1], 96)
    assert (o["score"], o["row_first"], o["start"], o["end"], o["n_skipped"]) == (96 - 129, [-1, 1], [4, 4], [4, 7], 1)


def test_restatement_tie_break_is_stay_advance_skip():
    """Everything ties (w = 0 and bias 0 everywhere, pen 0): stay wins over advance wins over skip, so the path advances only where it
    must -- never -- and ends in L because the trail is not strictly smaller: base 1 takes row 0, base 2 every other row."""
    flat = ref.Model(1, [0] * 4, [0] * 4, [0] * 4, (0, 0, 0))
    ev = ref.events_of(np.zeros(10, dtype=np.int64), [0, 2, 4, 6, 8])
    o = ref.align_plain(ev, 10, [2, 2], flat, 0, 1024, 0)
    assert (o["score"], o["row_first"], o["row_last"], o["n_skipped"]) == (0, [0, 1], [0, 4], 0)


# ---------------------------------------------------------------------------------------------- the cases
def test_twin_equals_plain():
    small = ec.small_cases()
    assert len(small) >= 30
    for c in small:
        plain = ref.align_plain(c["ev"], c["T"], c["codes"], c["model"], c["m2"], c["d4"], c["pen"], c["off"])
        assert plain == ec.reference(c), c["name"]


def test_every_case_meets_its_condition():
    cases = ec.all_cases()
    assert set(ec.STATE_COUNTS) <= {len(c["codes"]) + 2 for c in cases}
    for c in cases:
        assert c["cond"](ec.reference(c)), c["name"]
        E, L = len(c["ev"]["start"]), len(c["codes"])
        # the contract's bounds: sum n_e = T <= 2^19 for an OK read, every n_e < 2^23, finite values below 0.75 * 2^30
        if ec.reference(c)["status"] == ref.OK:
            n = np.diff(np.concatenate([c["ev"]["start"], [c["T"]]]))
            assert n.sum() == c["T"] <= 1 << 19 and n.min() >= 1 and n.max() < 1 << 23 and E <= c["T"]
            assert abs(ec.reference(c)["score"]) < 3 * (1 << 28)
    assert {ec.reference(c)["status"] for c in cases} == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH}
    assert {c["pen"] for c in cases} >= {-1, 0, 96, 256}
    for S in ec.STATE_COUNTS:                                             # E = ceil((L + 1) / 2), + 1, L and 2 L + 3 at every boundary
        L = S - 2
        assert {len(c["ev"]["start"]) for c in cases if len(c["codes"]) == L} >= {(L + 2) // 2, (L + 2) // 2 + 1, L, 2 * L + 3}
    # both halves of the pair cross every kind of boundary: a lane (16, 17), a wave (1024, 1025) and a band (4096, 4097)
    by = {c["name"]: ec.reference(c) for c in cases if c["name"].startswith("enter_")}
    assert all(ec.entered_by_skip(by["enter_even_by_skip"], s) and ec.entered_by_advance(by["enter_by_advance"], s) for s in (16, 1024, 4096))
    assert all(ec.entered_by_skip(by["enter_odd_by_skip"], s) and ec.entered_by_advance(by["enter_even_by_skip"], s)
               and ec.entered_by_advance(by["enter_by_advance"], s) for s in (17, 1025, 4097))


def test_no_path_is_where_the_rows_stop_reaching():
    """Row e reaches the states up to 2 e + 1 with skips and e + 1 without: the status rule against the restated DP itself, which asserts
    that every cell it keeps is reachable and ends in a reachable state."""
    rng = np.random.default_rng(5)
    for L in range(0, 12):
        for E in range(1, 9):
            ev = ref.events_of(rng.integers(500, 700, 3 * E), 3 * np.arange(E))
            for pen in (-1, 0, 96):
                o = ref.align_plain(ev, 3 * E, rng.integers(0, 4, L), ec.MODEL, ec.M2, ec.D4, pen)
                assert (o["status"] == ref.NO_PATH) == ((E if pen < 0 else 2 * E - 1) < L), (L, E, pen)
                assert o["status"] == ref.NO_PATH or abs(o["score"]) < 1 << 28


def test_host_equals_restatement_on_every_case():
    from radian_amd.backend import eventalign_events_host
    for model, pen, cases in ec.groups():
        res = eventalign_events_host(model=ec.backend_model(model), skip_pen=pen, **ec.call_args(cases))
        for r, c in enumerate(cases):
            ref.assert_read_equal(res, r, ec.reference(c), c["name"])
    # one read per call and the reverse order give the same
    for model, pen, few in ec.groups(ec.small_cases()[::-1]):
        res = eventalign_events_host(model=ec.backend_model(model), skip_pen=pen, **ec.call_args(few))
        for r, c in enumerate(few):
            ref.assert_read_equal(res, r, ec.reference(c), c["name"])
            ref.assert_read_equal(eventalign_events_host(model=ec.backend_model(model), skip_pen=pen, **ec.call_args([c])), 0, ec.reference(c), c["name"])


def test_host_refusals_and_the_workspace_formula():
    from radian_amd.backend import EvalModel, RadianHipError, eventalign_events_host, eventalign_events_workspace_bytes
    m = ec.backend_model()
    x = np.arange(600, 650)
    good = dict(events=[ref.events_of(x, [0, 10, 30])], n_samples=[50], seqs=[np.array([0, 1, 2], dtype=np.uint8)], m2=[1200], d4=[240], model=m)
    assert eventalign_events_host(**good).status[0] == ref.OK
    assert eventalign_events_host([], [], [], m, [], []).status.shape == (0,)

    def ev(**kw):
        e = {k: np.array(v) for k, v in good["events"][0].items()}
        for k, (i, v) in kw.items():
            e[k][i] = v
        return [e]

    bad = [dict(seqs=[np.array([0, 4], dtype=np.uint8)]), dict(d4=[-1]), dict(d4=[(1 << 20) + 1]), dict(m2=[(1 << 17) + 1]), dict(skip_pen=-2),
           dict(skip_pen=257), dict(n_samples=[-1]), dict(sample_off=[-1]), dict(sample_off=[(1 << 31) - 50]), dict(n_samples=[30]),   # a start >= T
           dict(events=ev(start=(0, 1))), dict(events=ev(start=(1, 30))), dict(events=ev(start=(1, 0))), dict(events=ev(start=(2, 50))),
           dict(events=ev(sum=(0, 32768 * 10))), dict(events=ev(sum=(2, -32769 * 20))), dict(n_samples=[0])]
    for kw in bad:
        with pytest.raises(RadianHipError):
            eventalign_events_host(**{**good, **kw})
    assert eventalign_events_host(**{**good, "events": ev(sum=(0, 32767 * 10)), "sample_off": [(1 << 31) - 51]}).status[0] == ref.OK
    for field, value in (("lvl", 1 << 14), ("bias", 257), ("bias", -257)):
        t = dict(lvl=m.lvl.copy(), w=m.w.copy(), bias=m.bias.copy())
        t[field][9] = value
        with pytest.raises(RadianHipError):
            eventalign_events_host(**{**good, "model": EvalModel(m.k, t["lvl"], t["w"], t["bias"], m.bg)})
    # the workspace formula: 8 E + 4 E ceil((L + 2) / 16) + (16 E when L + 2 > 4096), each term rounded up to 256
    up = lambda v: (v + 255) // 256 * 256
    for E, L in ((1, 0), (1000, 14), (1000, 15), (30000, 1000), (777, 4094), (777, 4095), (1 << 19, 4000)):
        assert eventalign_events_workspace_bytes(E, L) == up(8 * E) + up(4 * E * ((L + 2 + 15) // 16)) + (up(16 * E) if L + 2 > 4096 else 0)
    assert eventalign_events_workspace_bytes(-1, 0) == -1 and eventalign_events_workspace_bytes(0, -1) == -1


# ---------------------------------------------------------------------------------------------- the identity with sample rows
def test_one_event_per_sample_without_skips_is_eventalign():
    from radian_amd.backend import eventalign_events_host, eventalign_host
    cases = [c for c in sc.all_cases() if c["t_hi"] - c["t_lo"] >= 1]
    assert len(cases) >= 70
    want = eventalign_host(model=sc.backend_model(), **sc.call_args(cases))
    got = eventalign_events_host([ec.sample_events(c) for c in cases], [c["t_hi"] - c["t_lo"] for c in cases], [c["codes"] for c in cases],
                                 sc.backend_model(), want.m2, want.d4, sample_off=[c["t_lo"] for c in cases], skip_pen=-1)
    assert {int(s) for s in want.status} == {sref.OK, sref.TOO_LONG, sref.MAD_ZERO, sref.NO_PATH}
    ec.assert_identity(got, want, cases)


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_eventalign_events_host(tmp_path):
    """tests/asan_eventalign_events.cpp: the host side of rd_eventalign_events (argument checks, the rules, the host twin) built with
    AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_eventalign_events"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_eventalign_events.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 200 and int(last[2]) >= 200          # "<n> accepted <m> refused"


# ---------------------------------------------------------------------------------------------- accuracy on simulated reads
# MEASURED with the restatement: the 16 simulated reads of section 24, _segment_ref.segment_np at `segment`'s
# defaults from t_lo on, round 0 on the window's own scale and two refits; pooled over the bases of all 16 fragments.
# pen 96: within 10 0.8841, within 30 0.9785, skipped 0.0544 at 1.744 events per base; without skips 0.8271 / 0.9412.
MEASURED = {"within10": 0.8841, "within30": 0.9785, "skipped": 0.0544}
DEFAULT_PEN = 96


def sim_model():
    from radian_amd.eventalign import model_tables
    from radian_amd.simulate import standin_tables
    level, sd, _ = standin_tables(sc.SIM_K, sc.SIM_MODEL_SEED)
    return sref.as_ref_model(model_tables(sc.SIM_K, level, sd, 1.0)[0])


_sim_events = {}
COMMAND_DEFAULTS = dict(w1=4, w2=12, th1=100, th2=400, v0=1)      # `segment`'s: t1 2.5 and t2 5.0 as 16 t^2


def sim_events(seed, params=None):
    """the events of a simulated read's window, cut once"""
    params = seg.params(**(params or COMMAND_DEFAULTS))
    key = (seed, tuple(sorted(params.items())))
    if key not in _sim_events:
        raw, _, t_lo, _ = sc.sim_read(seed)
        _sim_events[key] = seg.segment_np(raw[t_lo:], params, (0, len(raw) - t_lo))
    return _sim_events[key]


def sim_accuracy(pen, params=None, rounds=2):
    """-> (within 10, within 30, skipped share, events per base, the last read's fitted m2 and d4) pooled over the 16 reads: a base's first
    sample is its event's start"""
    from radian_amd.eventalign import refit
    model = sim_model()
    tot = np.zeros(5, dtype=np.int64)
    for seed in sc.SIM_SEEDS:
        raw, codes, t_lo, truth = sc.sim_read(seed)
        ev = sim_events(seed, params)
        m2, d4 = ev["m2"], ev["d4"]
        for _ in range(rounds + 1):
            used = (m2, d4)
            o = ref.align_numpy(ev, len(raw) - t_lo, codes, model, m2, d4, pen, t_lo)
            assert o["status"] == ref.OK
            m2, d4 = refit(o["sums"], m2, d4)
        err = np.abs(np.asarray(o["start"], dtype=np.int64) - truth)
        tot += (int((err <= 10).sum()), int((err <= 30).sum()), o["n_skipped"], len(ev["start"]), len(codes))
    return tot[0] / tot[4], tot[1] / tot[4], tot[2] / tot[4], tot[3] / tot[4], *used


def test_accuracy_of_the_restatement_on_simulated_reads():
    """The floors for within 10 and within 30 samples at the default penalty are the restatement's own measured values less one read's
    worth, 1 / 16 of the measured value (section 27's convention); with skips within 10 is not below what it is without; the share of
    skipped bases stays under its measured value plus one read's worth."""
    w10, w30, sk, epb, m2, d4 = sim_accuracy(DEFAULT_PEN)
    n10, n30, nsk, _, _, _ = sim_accuracy(-1)
    print(f"pen {DEFAULT_PEN}: within10 {w10:.4f} within30 {w30:.4f} skipped {sk:.4f} events/base {epb:.3f} m2 {m2} d4 {d4}; no skips: within10 {n10:.4f} within30 {n30:.4f}")
    assert nsk == 0
    assert w10 >= MEASURED["within10"] * 15 / 16 and w30 >= MEASURED["within30"] * 15 / 16
    assert w10 >= n10
    assert sk <= MEASURED["skipped"] * 17 / 16       # the cap: 17 / 16 of the measured share
