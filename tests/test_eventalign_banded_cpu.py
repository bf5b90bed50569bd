"""No-GPU checks of banded eventalign: the plain-Python restatement of the contract (tests/_eventalign_banded_ref.py)
by hand on toys, its NumPy twin against it, every seeded case's defining condition (tests/_eventalign_banded_cases.py),
rd_eventalign_banded_host against the restatement on every case, the identity with rd_eventalign, every refusal, the workspace formula, the
host code under the sanitizers, and the accuracy of event rounds followed by one banded pass on simulated reads.  Every comparison of
integers is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _eventalign_banded_cases as bc
import _eventalign_banded_ref as ref
import _eventalign_cases as sc
import _eventalign_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W100 = 16 * 2 ** 32 // 10000          # sd 100
W_BG = 16 * 2 ** 32 // (380 * 380)    # sd 380


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_window_rule_by_hand():
    assert [ref.lo_of(g, 64) for g in (0, 31, 32, 33, 34, 64)] == [0, 0, 1, 2, 2, 2]          # L + 2 = 66: the window slides twice, then stops
    assert [ref.lo_of(g, 62) for g in (0, 40, 62)] == [0, 0, 0]                               # L + 2 = 64: it never moves
    assert [ref.lo_of(g, 1000) for g in (31, 32, 500, 969, 970, 1000)] == [0, 1, 469, 938, 938, 938]
    # g(t) counts the guide values <= the row's sample in READ coordinates; equal values move it by several in one row
    assert ref.window_rows([100, 100, 103] + [200] * 61, 64, 100, 5) == [0] * 5
    assert ref.window_rows([5] * 40 + [12] * 24, 64, 10, 4) == [2, 2, 2, 2] and ref.window_rows([5] * 32 + [12] * 32, 64, 10, 4) == [1, 1, 2, 2]


def _toy66():
    """k = 1, L = 64 (66 states): bases ACAC..., two samples per base on the base's level, no lead and no trail.  m2 = 0, d4 = 1024: zq = x."""
    model = fref.Model(1, [-1000, 1000, 0, 0], [W100] * 4, [-43] * 4, (0, W_BG, 0))
    codes = [b & 1 for b in range(64)]
    x = np.repeat([(-1000, 1000)[c] for c in codes], 2).astype(np.int16)
    return model, codes, x


def test_restatement_on_a_window_that_slides_twice():
    """66 states: lo is 0 until 32 bases have started, 1 until 33 have, then 2.  With the guide on the truth the path (state b + 1 at rows
    2 b, 2 b + 1) is always 30 or 31 states above lo, and the result is the full DP's: every sample on its level, 128 * -43."""
    model, codes, x = _toy66()
    guide = [2 * b for b in range(64)]
    assert ref.window_rows(guide, 64, 0, 128)[60:68] == [0, 0, 1, 1, 2, 2, 2, 2]
    o = ref.align_plain(x, codes, guide, model, m2=0, d4=1024)
    f = fref.align_plain(x, codes, model, m2=0, d4=1024)
    assert o["status"] == ref.OK and o["score"] == 128 * -43 and o["first"] == guide and o["n_edge"] == 0
    assert all(o[k] == f[k] for k in f)
    # the guide a whole read early: lo = 2 from row 0 on.  States 0 and 1 are outside win(0): nothing starts, OFF_BAND
    o = ref.align_plain(x, codes, [-1] * 64, model, m2=0, d4=1024)
    assert o["status"] == ref.OFF_BAND and o["score"] == 0 and o["first"] == [-1] * 64 and o["n_edge"] == 0 and (o["m2"], o["d4"]) == (0, 1024)
    # the guide a whole read late: lo = 0 for ever, the window ends at state 63 and never holds states 64 (base 64) or 65 (the trail)
    assert ref.align_plain(x, codes, [500] * 64, model, m2=0, d4=1024)["status"] == ref.OFF_BAND


def test_restatement_lowest_state_has_no_advance_edge():
    """lo(0) = 1: state 1 is in win(0) and starts the path (V = c(0, 1)); state 0 is not.  Then the guide makes lo = 2 at the row base 2
    would be entered: state 2 is the window's lowest, has no advance edge, and its stay edge comes from outside the window: the path is
    lost although state 2 is inside the window; a row later it costs one capped sample; two rows later nothing."""
    model, codes, x = _toy66()
    g32 = [-1] * 32 + [1000] * 32                              # 32 bases at or before row 0: lo = 1 throughout
    assert set(ref.window_rows(g32, 64, 0, 128)) == {1}
    o = ref.align_plain(x, codes, g32, model, m2=0, d4=1024)
    assert o["status"] == ref.OK and o["first"][0] == 0        # base 1 (state 1) from row 0 on; the window [1, 64] holds base 64, state 64
    assert o["n_edge"] >= 1 and o["first"][:2] == [0, 2]       # base 1 sat on the lower rim (lo == 1 == s)
    early = [-1] * 32 + [1] + [1000] * 31                      # lo = 2 from row 1 on, a row before state 2 can be entered from inside the window
    assert ref.window_rows(early, 64, 0, 128)[:4] == [1, 2, 2, 2]
    o = ref.align_plain(x, codes, early, model, m2=0, d4=1024)
    assert o["status"] == ref.OFF_BAND                         # state 2 at row 1: no advance (the lowest), and its stay is row 0's 2^30
    tight = [-1] * 32 + [2] + [1000] * 31                      # lo = 2 from row 2 on: state 2 was entered at row 1, on base 1's second sample,
    o = ref.align_plain(x, codes, tight, model, m2=0, d4=1024)  # ... which costs it the cap once, and is kept: state 1 is gone at row 2
    assert o["status"] == ref.OK and o["first"][:3] == [0, 1, 4] and o["score"] == 127 * -43 + 981 and o["n_edge"] >= 1
    late = [-1] * 32 + [3] + [1000] * 31                       # a row later state 2 has been entered from state 1 inside the window, at its own row
    o = ref.align_plain(x, codes, late, model, m2=0, d4=1024)
    assert o["status"] == ref.OK and o["first"][:3] == [0, 2, 4] and o["score"] == 128 * -43


# ---------------------------------------------------------------------------------------------- the cases
def test_twin_equals_plain():
    small = bc.small_cases()
    assert len(small) >= 60
    for c in small:
        plain = ref.align_plain(c["raw"], c["codes"], c["guide"], c["model"], c["t_lo"], c["t_hi"], c["m2"], c["d4"])
        assert plain == bc.reference(c), c["name"]


def test_every_case_meets_its_condition():
    cases = bc.all_cases()
    assert set(bc.STATE_COUNTS) <= {len(c["codes"]) + 2 for c in cases}
    seen, rim = set(), []
    n_inside = 0
    for c in cases:
        o, f = bc.reference(c), bc.full_reference(c)
        assert c["cond"](o, f), c["name"]
        seen.add(o["status"])
        if f is not None and bc.is_interior(c, f):            # the identity
            n_inside += 1
            assert bc.same(o, f), c["name"]
        if c["kind"] == "rim" and len(c["codes"]) + 2 >= 127:
            rim.append((o["status"], o["n_edge"] > 0, o["status"] == ref.OK and o["score"] > f["score"]))
        if c["kind"] == "events":
            print(c["name"], "status", o["status"], "n_edge", o["n_edge"], "interior", bc.is_interior(c, f), "same", bc.same(o, f))
    assert seen == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH, ref.OFF_BAND}
    assert n_inside >= 80
    # the rim from both sides: a path on it is counted, a path beyond it costs more or is lost
    assert any(s == ref.OK and e for s, e, _ in rim) and any(s == ref.OFF_BAND for s, _, _ in rim) and any(w for _, _, w in rim)
    # lo(0) > 0 occurs, and so do jumps of exactly 63, 64 and 65 states and of a whole read
    assert any(bc.lo_rows(c)[0] > 0 for c in cases if c["kind"] == "before" and len(c["codes"]) + 2 > 64)
    jumps = {int(np.diff(bc.lo_rows(c)).max()) for c in cases if c["kind"] in ("jump", "const") and c["t_hi"] - c["t_lo"] > 1}
    assert {63, 64, 65, 4097 - 64} <= jumps


def test_host_equals_restatement_on_every_case():
    from radian_amd.backend import eventalign_banded_host
    for model, cases in bc.groups():
        res = eventalign_banded_host(model=bc.backend_model(model), **bc.call_args(cases))
        for r, c in enumerate(cases):
            ref.assert_read_equal(res, r, bc.reference(c), c["name"])
    # one read per call and the reverse order give the same
    few = bc.small_cases()[::-1]
    res = eventalign_banded_host(model=bc.backend_model(), **bc.call_args(few))
    for r, c in enumerate(few):
        ref.assert_read_equal(res, r, bc.reference(c), c["name"])
        ref.assert_read_equal(eventalign_banded_host(model=bc.backend_model(), **bc.call_args([c])), 0, bc.reference(c), c["name"])


def _same_as_full(banded, i, full, j, what):
    assert int(banded.status[i]) == int(full.status[j]) and int(banded.score[i]) == int(full.score[j]), what
    assert (int(banded.m2[i]), int(banded.d4[i])) == (int(full.m2[j]), int(full.d4[j])) and banded.fit_sums[i].tolist() == full.fit_sums[j].tolist(), what
    assert banded.first_step[i].tolist() == full.first_step[j].tolist() and banded.last_step[i].tolist() == full.last_step[j].tolist(), what
    for f in ("start", "end", "sum", "sumsq", "min", "max"):
        assert getattr(banded.events, f)[i].tolist() == getattr(full.events, f)[j].tolist(), (what, f)


def test_identity_with_eventalign_host():
    """every case whose full path is interior equals rd_eventalign_host field for field; every case of _eventalign_cases with L + 2 <= 64
    equals it under three arbitrary guides"""
    from radian_amd.backend import eventalign_banded_host, eventalign_host
    inside = [c for c in bc.all_cases() if c["model"] is bc.MODEL and bc.full_reference(c) is not None and bc.is_interior(c, bc.full_reference(c))]
    assert len(inside) >= 80
    banded = eventalign_banded_host(model=bc.backend_model(), **bc.call_args(inside))
    full = eventalign_host(model=bc.backend_model(), **bc.full_args(inside))
    for r, c in enumerate(inside):
        _same_as_full(banded, r, full, r, c["name"])
        assert banded.n_edge[r] == 0 or len(c["codes"]) + 2 > 64        # (the upper rim itself is inside: an interior path may touch it)
    short = [c for c in sc.all_cases() if len(c["codes"]) + 2 <= 64]
    assert len(short) >= 30
    full = eventalign_host(model=sc.backend_model(), **sc.call_args(short))
    rng = np.random.default_rng(9)
    for guide_of in (lambda c: np.zeros(len(c["codes"])), lambda c: np.sort(rng.integers(-10 ** 6, 10 ** 6, len(c["codes"]))),
                     lambda c: np.full(len(c["codes"]), 2 ** 31 - 1)):
        banded = eventalign_banded_host(model=sc.backend_model(), guides=[guide_of(c) for c in short], **sc.call_args(short))
        for r, c in enumerate(short):
            _same_as_full(banded, r, full, r, c["name"])
            assert banded.n_edge[r] == 0


def test_host_refusals_and_the_workspace_formula():
    from radian_amd.backend import EvalModel, RadianHipError, eventalign_banded_host, eventalign_banded_workspace_bytes
    m = bc.backend_model()
    raw, codes, guide = [np.arange(50, dtype=np.int16)], [np.array([0, 1, 2], dtype=np.uint8)], [np.array([3, 3, 9])]
    assert eventalign_banded_host(raw, codes, guide, m).status[0] == ref.OK
    assert eventalign_banded_host([], [], [], m).status.shape == (0,)
    bad = [dict(guides=[np.array([3, 2, 9])]), dict(guides=[np.array([3, 9, 8])]),                         # a guide that decreases
           dict(seqs=[np.array([0, 4, 1], dtype=np.uint8)]), dict(t_lo=[-1]), dict(t_lo=[10], t_hi=[9]), dict(t_hi=[51]), dict(d4=[-1]),
           dict(d4=[(1 << 20) + 1]), dict(m2=[(1 << 17) + 1], d4=[5])]                                  # whatever rd_eventalign refuses
    for kw in bad:
        with pytest.raises(RadianHipError):
            eventalign_banded_host(**{**dict(raws=raw, seqs=codes, guides=guide, model=m), **kw})
    with pytest.raises(ValueError):
        eventalign_banded_host(raw, codes, [np.array([3, 3])], m)
    # a decrease ACROSS two reads is no decrease
    two = eventalign_banded_host(raw * 2, codes * 2, [np.array([30, 30, 40]), np.array([1, 2, 3])], m)
    assert two.status.tolist() == [ref.OK, ref.OK]
    for field, value in (("lvl", 1 << 14), ("bias", -257)):
        t = dict(lvl=m.lvl.copy(), w=m.w.copy(), bias=m.bias.copy())
        t[field][9] = value
        with pytest.raises(RadianHipError):
            eventalign_banded_host(raw, codes, guide, EvalModel(m.k, t["lvl"], t["w"], t["bias"], m.bg))
    # the workspace formula: 4 T + 8 T + 4 T + 12 (L + 2 + 128), each term rounded up to 256: O(T + L)
    up = lambda v: (v + 255) // 256 * 256
    for T, L in ((1, 0), (1000, 30), (1000, 62), (1000, 63), (30000, 1000), (777, 4095), (1 << 19, 4000), (120000, 4000)):
        assert eventalign_banded_workspace_bytes(T, L) == up(4 * T) + up(8 * T) + up(4 * T) + up(12 * (L + 2 + 128))
    assert eventalign_banded_workspace_bytes(-1, 0) == -1 and eventalign_banded_workspace_bytes(120000, 4000) < 2 * 1024 * 1024


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_eventalign_banded_host(tmp_path):
    """tests/asan_eventalign_banded.cpp: the host side of rd_eventalign_banded (argument checks, the rules, the host twin) built with
    AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_eventalign_banded"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_eventalign_banded.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 200 and int(last[2]) >= 200          # "<n> accepted <m> refused"


# ---------------------------------------------------------------------------------------------- accuracy on simulated reads
# MEASURED with the restatements: the 16 simulated reads of section 24; `segment`'s defaults; three event rounds
# at pen 96 (section 28), refit of the last round's sums, one banded pass guided by that round's ev_start.  Pooled over the bases of all
# 16 fragments: within 10 0.9332, within 30 0.9834; the event pass it started from 0.8841 / 0.9785.  The full DP's path never leaves the
# guide by more than 4 states (31 are allowed).
MEASURED = {"within10": 0.9332, "within30": 0.9834}


def test_accuracy_of_events_then_band_on_simulated_reads():
    import _eventalign_events_ref as eref
    import test_eventalign_events_cpu as te
    from radian_amd.eventalign import refit
    model = te.sim_model()
    tot = np.zeros(4, dtype=np.int64)
    worst = 0
    for seed in sc.SIM_SEEDS:
        raw, codes, t_lo, truth = sc.sim_read(seed)
        ev = te.sim_events(seed)
        m2, d4 = ev["m2"], ev["d4"]
        for _ in range(3):
            e = eref.align_numpy(ev, len(raw) - t_lo, codes, model, m2, d4, te.DEFAULT_PEN, t_lo)
            assert e["status"] == eref.OK
            m2, d4 = refit(e["sums"], m2, d4)
        guide = np.asarray(e["start"], dtype=np.int64)
        full = fref.align_numpy(raw, codes, model, t_lo, None, m2, d4)
        o = ref.align_numpy(raw, codes, guide, model, t_lo, None, m2, d4)
        # every read meets the interior condition, so the banded pass IS the full DP on that scale
        assert ref.interior(full["first"], full["last"], len(codes), guide, t_lo, len(raw) - t_lo), seed
        assert o["status"] == ref.OK and o["n_edge"] == 0 and all(o[k] == full[k] for k in full), seed
        t = t_lo + np.arange(len(raw) - t_lo)
        s = np.where(t > full["last"][-1], len(codes) + 1, np.searchsorted(np.asarray(full["first"]), t, side="right"))
        worst = max(worst, int(np.abs(s - np.searchsorted(guide, t, side="right"))[t <= full["last"][-1]].max()))
        err, err_ev = np.abs(np.asarray(o["first"], dtype=np.int64) - truth), np.abs(guide - truth)
        tot += (int((err <= 10).sum()), int((err <= 30).sum()), int((err_ev <= 10).sum()), len(codes))
    w10, w30, e10 = tot[0] / tot[3], tot[1] / tot[3], tot[2] / tot[3]
    print(f"banded after three event rounds: within10 {w10:.4f} within30 {w30:.4f}; the event pass: within10 {e10:.4f}; the full path leaves the guide by at most {worst} states")
    assert worst <= 31
    assert w10 >= MEASURED["within10"] * 15 / 16 and w30 >= MEASURED["within30"] * 15 / 16
    assert w10 >= e10
