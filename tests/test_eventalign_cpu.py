"""No-GPU checks of eventalign: the plain-Python restatement of the contract (tests/_eventalign_ref.py) by hand on
toys, its NumPy twin against it, every seeded case's defining condition (tests/_eventalign_cases.py), rd_eventalign_host against the
restatement on every case and every refusal, the host formulas of radian_amd/eventalign.py (model_tables, the rational refit, --bounds) and
the accuracy of the restatement on simulated reads.  Every comparison of integers is for equality."""
import os

import numpy as np
import pytest

import _eventalign_cases as ec
import _eventalign_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W100 = 16 * 2 ** 32 // 10000          # sd 100
W_BG = 16 * 2 ** 32 // (380 * 380)    # sd 380


def toy_model():
    """k = 1: A at -1000, C at +1000, G and T at 0; sd 100 and bias -43 each; the background at 0 with sd 380 and bias 0"""
    return ref.Model(1, [-1000, 1000, 0, 0], [W100] * 4, [-43] * 4, (0, W_BG, 0))


def toy(x, codes):
    # m2 = 0, d4 = 1024: u = 1024 x, zq = floor((2048 x + 1024) / 2048) = x
    return ref.align_plain(np.array(x, dtype=np.int16), codes, toy_model(), m2=0, d4=1024)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_on_two_bases_and_four_samples():
    """A sample on its base's level costs the bias alone, -43; 2000 away it costs the cap, 1024 - 43; in the background at 0, 0; at +-1000
    16 * 10^6 / 144400 = 110."""
    assert ref.quant(-1000, 0, 1024) == -1000 and ref.cost(-1000, (-1000, W100, -43)) == -43 and ref.cost(1000, (-1000, W100, -43)) == 981
    assert ref.cost(0, (0, W_BG, 0)) == 0 and ref.cost(1000, (0, W_BG, 0)) == 110
    for x, first, last, score in (([-1000, -1000, 1000, 1000], [0, 2], [1, 3], -172),
                                  ([-1000, 1000, 1000, 1000], [0, 1], [0, 3], -172),
                                  ([-1000, -1000, -1000, 1000], [0, 3], [2, 3], -172),
                                  ([0, -1000, 1000, 1000], [1, 2], [1, 3], -129),        # the lead takes the sample at the background's level
                                  ([-1000, -1000, 1000, 0], [0, 2], [1, 2], -129)):      # ... and the trail
        o = toy(x, [0, 1])
        assert (o["status"], o["first"], o["last"], o["score"]) == (ref.OK, first, last, score), (x, o)
        assert o["start"] == first and o["end"] == first[1:] + [last[1] + 1]
        n = [e - s for s, e in zip(o["start"], o["end"])]
        assert o["sums"] == [sum(n), -1000 * n[0] + 1000 * n[1], 10 ** 6 * sum(n), sum(x[first[0]:last[1] + 1]),
                             -1000 * sum(x[o["start"][0]:o["end"][0]]) + 1000 * sum(x[o["start"][1]:o["end"][1]])]
    assert toy([5, 5, 5], [0, 1, 0, 1])["status"] == ref.NO_PATH and toy([], [0])["status"] == ref.EMPTY


def test_restatement_tie_break_on_a_constant_signal():
    """Six samples on C's level and three C: every cell of a base state costs -43, so every advance after the first possible one ties
    with staying and is NOT taken: every base but the last takes exactly one sample, at the start."""
    o = toy([1000] * 6, [1, 1, 1])
    assert (o["first"], o["last"], o["score"]) == ([0, 1, 2], [0, 1, 5], -258)
    assert o["sums"] == [6, 6000, 6 * 10 ** 6, 6000, 6 * 10 ** 6]
    # the end: the trail only if STRICTLY smaller.  With the background as cheap as the base (bias 0 and w 0 everywhere) everything ties:
    flat = ref.Model(1, [0] * 4, [0] * 4, [0] * 4, (0, 0, 0))
    o = ref.align_plain(np.zeros(5, dtype=np.int16), [2, 2], flat, m2=0, d4=1024)
    assert (o["first"], o["last"], o["score"]) == ([0, 1], [0, 4], 0)


def test_restatement_scale_and_rounding():
    assert ref.window_scale([10, 20, 30, 40]) == (50, 40)          # m2 = 20 + 30; |2x - 50| = 30 10 10 30 -> 10 + 30
    assert ref.window_scale([7]) == (14, 0)
    # rounded half up: (2u + d4) / (2 d4) = u / d4 + 1/2, floored; u = 512 (2x - m2)
    assert ref.quant(1, 0, 2048) == 1 and ref.quant(-1, 0, 2048) == 0 and ref.quant(-3, 0, 2048) == -1 and ref.quant(0, 1, 1024) == 0
    assert ref.quant(32767, 0, 1) == 1 << 14 and ref.quant(-32768, 0, 1) == -(1 << 14)
    assert ref.kmer([0, 1, 2, 3], 0, 3) == 0b000001 and ref.kmer([0, 1, 2, 3], 3, 3) == 0b101111 and ref.kmer([2], 0, 5) == 0b1010101010


# ---------------------------------------------------------------------------------------------- the cases
def test_twin_equals_plain():
    small = ec.small_cases()
    assert len(small) >= 30
    for c in small:
        plain = ref.align_plain(c["raw"], c["codes"], ec.MODEL, c["t_lo"], c["t_hi"], c["m2"], c["d4"])
        assert plain == ec.reference(c), c["name"]


def test_every_case_meets_its_condition():
    cases = ec.all_cases()
    states = {len(c["codes"]) + 2 for c in cases}
    assert set(ec.STATE_COUNTS) <= states
    for c in cases:
        assert c["cond"](ec.reference(c)), c["name"]
    seen = {ec.reference(c)["status"] for c in cases}
    assert seen == {ref.OK, ref.EMPTY, ref.TOO_LONG, ref.MAD_ZERO, ref.NO_PATH}
    a, b = (ec.reference(c) for c in cases if c["name"] in ("win_inner", "scale_given"))
    assert a == b                                                    # d4 given == d4 computed
    # empty and non-empty lead and trail both occur among the OK cases
    lead = {ec.reference(c)["first"][0] > c["t_lo"] for c in cases if ec.reference(c)["status"] == ref.OK and len(c["codes"])}
    trail = {ec.reference(c)["last"][-1] < c["t_hi"] - 1 for c in cases if ec.reference(c)["status"] == ref.OK and len(c["codes"])}
    assert lead == {False, True} and trail == {False, True}


def test_host_equals_restatement_on_every_case():
    from radian_amd.backend import eventalign_host
    cases = ec.all_cases()
    res = eventalign_host(model=ec.backend_model(), **ec.call_args(cases))
    for r, c in enumerate(cases):
        ref.assert_read_equal(res, r, ec.reference(c), c["name"])
    # one read per call and the reverse order give the same
    few = [c for c in ec.small_cases()][::-1]
    res = eventalign_host(model=ec.backend_model(), **ec.call_args(few))
    for r, c in enumerate(few):
        ref.assert_read_equal(res, r, ec.reference(c), c["name"])
        ref.assert_read_equal(eventalign_host(model=ec.backend_model(), **ec.call_args([c])), 0, ec.reference(c), c["name"])


def test_host_refusals():
    from radian_amd.backend import EvalModel, RadianHipError, eventalign_host, eventalign_workspace_bytes
    m = ec.backend_model()
    raw, codes = [np.arange(50, dtype=np.int16)], [np.array([0, 1, 2], dtype=np.uint8)]
    assert eventalign_host(raw, codes, m).status[0] == ref.OK
    assert eventalign_host([], [], m).status.shape == (0,)
    bad = [dict(seqs=[np.array([0, 4], dtype=np.uint8)]), dict(t_lo=[-1]), dict(t_lo=[10], t_hi=[9]), dict(t_hi=[51]), dict(d4=[-1]),
           dict(d4=[(1 << 20) + 1]), dict(m2=[(1 << 17) + 1], d4=[5])]
    for kw in bad:
        with pytest.raises(RadianHipError):
            eventalign_host(**{**dict(raws=raw, seqs=codes, model=m), **kw})
    for field, value in (("lvl", 1 << 14), ("lvl", -(1 << 14)), ("bias", 257), ("bias", -257)):
        t = dict(lvl=m.lvl.copy(), w=m.w.copy(), bias=m.bias.copy())
        t[field][9] = value
        with pytest.raises(RadianHipError):
            eventalign_host(raw, codes, EvalModel(m.k, t["lvl"], t["w"], t["bias"], m.bg))
    with pytest.raises(RadianHipError):
        eventalign_host(raw, codes, EvalModel(m.k, m.lvl, m.w, m.bias, (1 << 14, 0, 0)))
    # the workspace formula: 4 T + 4 T ceil((L + 2) / 32) + (8 T when L + 2 > 4096), each term rounded up to 256
    up = lambda v: (v + 255) // 256 * 256
    for T, L in ((1, 0), (1000, 30), (1000, 31), (30000, 1000), (777, 4094), (777, 4095), (1 << 19, 4000)):
        assert eventalign_workspace_bytes(T, L) == up(4 * T) + up(4 * T * ((L + 2 + 31) // 32)) + (up(8 * T) if L + 2 > 4096 else 0)
    assert eventalign_workspace_bytes(-1, 0) == -1


# ---------------------------------------------------------------------------------------------- the host formulas of the command
def test_model_tables_on_known_rows():
    from radian_amd.eventalign import model_tables
    level = np.zeros(4, dtype=np.int32)
    sd = np.zeros(4, dtype=np.int32)
    level[:] = (1024, -1536, 32768, 0)
    sd[:] = (307, 41, 0, 32768)
    m, sd_m = model_tables(1, level, sd, bg_sd=1.0)
    assert m.lvl.tolist() == [380, -569, 12145, 0]                       # rint(level 1.4826 / 4): 379.5 -> 380, -569.3, 12145.5 -> 12145 (even), 0
    assert sd_m.tolist() == [114, 15, 8, 12145]                          # 113.8; 15.2; 0 -> the floor of 8; 12145.5 -> 12145
    assert m.w.tolist() == [round(16 * 2 ** 32 / 114 ** 2), round(16 * 2 ** 32 / 225), 2 ** 30, round(16 * 2 ** 32 / 12145 ** 2)]
    bg = 1.4826 * 256
    assert m.bias.tolist() == [round(32 * np.log(114 / bg)), round(32 * np.log(15 / bg)), round(32 * np.log(8 / bg)), round(32 * np.log(12145 / bg))]
    assert m.bias.tolist() == [-38, -103, -124, 111] and m.bg == (0, round(16 * 2 ** 32 / bg ** 2), 0)
    # the clamps: the sd floor of 8 gives w = 2^30, far from 2^32 - 1; a background of 0.01 z is 3.8 units: ITS w, 16 2^32 / 3.8^2 > 2^32,
    # is clamped, and 32 ln(12145 / 3.8) = 258 is clipped to 256.  Against a background of 1280 z every bias is clipped to -256
    m, _ = model_tables(1, level, sd, bg_sd=0.01)
    assert m.bg[1] == 2 ** 32 - 1 and m.bias.tolist() == [109, 44, 24, 256]
    m, _ = model_tables(1, level, sd, bg_sd=32.0)
    assert m.bias.tolist() == [-149, -214, -234, 0]
    m, _ = model_tables(1, level, sd, bg_sd=1280.0)
    assert m.bias.tolist() == [-256, -256, -256, -118] and m.bg[1] == 0


def test_refit_against_lstsq_and_on_degenerate_reads():
    from radian_amd.eventalign import refit
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(2, 400))
        l = rng.integers(-1500, 1500, n)
        alpha, beta = float(rng.uniform(300, 900)), float(rng.uniform(0.05, 0.6))
        x = np.rint(alpha + beta * l + rng.normal(0, 5, n)).astype(np.int64)
        sums = [n, int(l.sum()), int((l * l).sum()), int(x.sum()), int((x * l).sum())]
        if len(set(l.tolist())) < 2:
            continue
        (b, a), *_ = np.linalg.lstsq(np.stack([l, np.ones(n)], axis=1).astype(np.float64), x.astype(np.float64), rcond=None)
        m2, d4 = refit(sums, 0, 1)
        assert abs(m2 - 2 * a) <= 0.5 + 1e-6 and abs(d4 - 1024 * b) <= 0.5 + 1e-6
    # exact: x = 600 + l / 4 on l = 0, 4, 8 -> alpha 600, beta 1/4
    assert refit([3, 12, 80, 1803, 7220], 7, 9) == (1200, 256)
    assert refit([2, 1, 1, 1, 1], 7, 9) == (0, 1024)                     # l = 0, 1; x = 0, 1: alpha 0, beta 1
    assert refit([2, 0, 2, 1, 1], 7, 9) == (1, 512)                      # l = -1, 1; x = 0, 1: alpha 1/2, beta 1/2
    # halves round up: l = -1, -1, 1, 1 and x = 0, 0, 0, 1: beta 1/4, alpha 1/4 -> rnd(1/2) = 1; with x = 0, 0, 0, -1: rnd(-1/2) = 0, and a
    # slope that is not positive leaves d4 = max(1, rnd(-256)) = 1
    assert refit([4, 0, 4, 1, 1], 7, 9) == (1, 256) and refit([4, 0, 4, -1, -1], 7, 9) == (0, 1)
    # degenerate: one base, or every base on one level -> the denominator is 0: the scale stays
    assert refit([5, 500, 50000, 3000, 300000], 1190, 238) == (1190, 238)
    assert refit([0, 0, 0, 0, 0], 1190, 238) == (1190, 238)
    # a fit the library would refuse keeps the scale as well
    assert refit([2, 1, 1, 10 ** 6, 10 ** 6], 1190, 238) == (1190, 238)


def test_bounds_of_a_polya_and_a_truth_table(tmp_path):
    from radian_amd.eventalign import read_bounds, window_start
    from radian_amd.polya import COLUMNS
    row = {c: "0" for c in COLUMNS}
    p = tmp_path / "polya.tsv"
    with open(p, "w") as f:
        f.write("\t".join(COLUMNS) + "\n")
        for rid, end in (("a", 4000), ("b", -1), ("c", 10)):
            f.write("\t".join({**row, "read_id": rid, "tail_end": str(end)}[c] for c in COLUMNS) + "\n")
    b = read_bounds(str(p))
    assert b == {"a": 4000, "b": -1, "c": 10}
    assert window_start("a", 9000, b, 32) == (3968, True) and window_start("c", 9000, b, 32) == (0, True)
    assert window_start("b", 9000, b, 32) == (0, False) and window_start("zz", 9000, b, 32) == (0, False) and window_start("a", 9000, None, 32) == (0, False)
    assert window_start("a", 3000, b, 32) == (3000, True)                # a bound past the read leaves an empty window
    t = tmp_path / "truth.tsv"
    t.write_text("read_id\tref_name\tref_start\tref_end\tn_samples\tlead\ttail_nt\ttail_start\ttail_end\nr1\tT1\t0\t200\t9000\t400\t60\t1290\t3011\nr2\tT1\t0\t200\t9000\t400\t0\t-1\t-1\n")
    assert read_bounds(str(t)) == {"r1": 3011, "r2": -1}
    bad = tmp_path / "bad.tsv"
    bad.write_text("read_id\tsomething\nr1\t5\n")
    with pytest.raises(SystemExit):
        read_bounds(str(bad))


# ---------------------------------------------------------------------------------------------- accuracy on simulated reads
def _sim_model():
    from radian_amd.eventalign import model_tables
    from radian_amd.simulate import standin_tables
    level, sd, _ = standin_tables(ec.SIM_K, ec.SIM_MODEL_SEED)
    return model_tables(ec.SIM_K, level, sd, 1.0)[0]


def test_accuracy_of_the_restatement_on_simulated_reads():
    """16 reads of sim_signal_host: 30 adapter bases, 60 A, a fragment of 200 or 300 bases; the stand-in table, k = 5; the window starts 32
    samples before the fragment's true first sample.  Two refits.  The floors leave out the stand-in's own ambiguity (neighbouring k-mers
    whose levels lie within the noise), not slack for a kernel: the GPU is held to this restatement bit for bit."""
    from radian_amd.eventalign import refit
    model = ref.as_ref_model(_sim_model())
    tot = {0: np.zeros(4, dtype=np.int64), 2: np.zeros(4, dtype=np.int64)}
    worst10, worst_err = 1.0, 0
    for seed in ec.SIM_SEEDS:
        raw, codes, t_lo, truth = ec.sim_read(seed)
        assert len(codes) in (200, 300) and t_lo > ec.SIM_LEAD
        m2 = d4 = 0
        for rnd in range(3):
            o = ref.align_numpy(raw, codes, model, t_lo, len(raw), m2, d4)
            assert o["status"] == ref.OK
            if rnd in tot:
                acc = ec.accuracy(o["first"], truth)
                tot[rnd] += acc[:4]
            m2, d4 = refit(o["sums"], o["m2"], o["d4"])
        worst10, worst_err = min(worst10, acc[0] / acc[3]), max(worst_err, acc[4])
        print(f"seed {seed}: L {len(codes)} m2 {o['m2']} d4 {o['d4']} within10 {acc[0] / acc[3]:.3f} within30 {acc[1] / acc[3]:.3f} exact {acc[2] / acc[3]:.3f} max {acc[4]}")
        assert abs(o["m2"] - 1200) <= 8 and abs(o["d4"] - 240) <= 6, (seed, o["m2"], o["d4"])
        assert acc[0] / acc[3] >= 0.85, (seed, acc)
    r0, r2 = tot[0] / tot[0][3], tot[2] / tot[2][3]
    print(f"pooled: round 0 within10 {r0[0]:.3f} within30 {r0[1]:.3f}; round 2 within10 {r2[0]:.3f} within30 {r2[1]:.3f} exact {r2[2]:.3f}; worst read {worst10:.3f}, max error {worst_err}")
    assert r2[0] >= 0.90 and r2[1] >= 0.96
    assert r2[0] >= r0[0] and r2[1] >= r0[1]
