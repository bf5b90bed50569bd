"""The argument sets of the score-arithmetic tests are what they claim to be (tests/_score_math_cases.py: each group's defining condition);
glibc_math.h compiled for the host inside the library (rd_diag_score_math_host) equals the running libm bit for bit on the full sets -- the
host twin is what test_gpu_score_math.py holds the device build against --; its refusals; and the error figures of libm alone against
mpmath, which check the error measure on a library whose accuracy is published."""
import math

import numpy as np
import pytest

import _score_math_cases as c


@pytest.fixture(scope="module")
def bk():
    from radian_amd import backend, build
    build.build()
    return backend


def word20(u):
    return (c.hi_word(u) & 0xFFFFF).astype(np.int64)


def holds(a, points):
    b = set(c.bits(a).tolist())
    return all(int(c.bits(p)[0]) in b for p in points)


# ------------------------------------------------------------------------------------------------------------- the sets
def test_exp_set_conditions():
    g = c.exp_groups()
    for name, a in g.items():
        if c.is_nonpos_group(name):
            assert np.all(a <= 0.0), name                                   # d <= 0 (-0.0 included; no NaN)
    a = g["zero_and_tiny"]
    assert holds(a, [0.0, -0.0, -c.TINY, -2.0 ** -29]) and np.signbit(a).sum() == a.size - 1
    for p in (-2.0 ** -60, -2.0 ** -54, -2.0 ** -53):
        assert holds(a, [c.step1(p, -1), p, c.step1(p, 1)])
    # k ln2 / 128 for k = 0, -3, -6, ..: five neighbours each (clamped at 0), down to below -745.2, every table index among them
    a = g["gm_exp_cuts"].reshape(-1, 5)
    ks = -c.GM_EXP_STRIDE * np.arange(a.shape[0])
    assert math.gcd(c.GM_EXP_STRIDE, 128) == 1 and a.shape[0] > 128 and a[-1, 2] < -745.2 and a[0, 2] == 0.0
    assert np.all(np.abs(a[:, 2] - ks * (c.LN2 / 128)) <= 4e-16 * np.abs(a[:, 2]))
    assert np.all(np.diff(a[1:], axis=1) > 0) and np.all(c.bits(a[1:, 4]) + 4 == c.bits(a[1:, 0]))       # (negative: the bit pattern falls as d rises)
    # -(k + 1/2) ln2 for k = 0 .. 1075, five neighbours each
    a = g["exp_nonpos_cuts"].reshape(-1, 5)
    assert a.shape[0] == 1076 and np.all(np.abs(a[:, 2] + (np.arange(1076) + 0.5) * c.LN2) <= 4e-16 * np.abs(a[:, 2]))
    assert np.all(c.bits(a[:, 4]) + 4 == c.bits(a[:, 0]))
    # the thresholds: nine neighbours each; the two that are defined by the result straddle it
    a = g["thresholds"].reshape(-1, 9)
    assert a.shape[0] == 5 and np.all(c.bits(a[:, 8]) + 8 == c.bits(a[:, 0]))
    assert abs(a[0, 4] + 708.3964185322641) < 1e-12 and abs(a[1, 4] + 745.1332191019412) < 1e-12
    assert list(a[2:, 4]) == [-746.0, -512.0, -1024.0]
    with c.mpmath.workprec(c.MP_PREC):
        assert c.mpmath.exp(c._mpf(a[0, 0])) < c.DBL_MIN < c.mpmath.exp(c._mpf(a[0, 8]))
        assert c.mpmath.exp(c._mpf(a[1, 0])) < c.mpmath.ldexp(1, -1075) < c.mpmath.exp(c._mpf(a[1, 8]))
    assert list(g["far"]) == [-1e308, -c.INF]
    a = g["random"]
    assert a.size == 100000 and a.max() <= -2.0 ** -60 and a.min() >= -746.0
    assert np.histogram(np.log2(-a), bins=7, range=(-60, 10))[0].min() > 10000         # log-uniform: every ten binades hold their share
    assert tuple(g["scan_worst"]) == c.EXP_SCAN_WORST
    a = g["gm_exp_only"]
    assert holds(a, [c.INF, 512.0, 1024.0, c.CUT["overflow"], c.step1(c.CUT["overflow"], 1)]) and np.isnan(a).sum() == 1
    assert np.nanmin(a) > 0 and math.exp(c.CUT["overflow"]) < c.INF
    assert sum(v.size for v in g.values()) <= 2000000 and c.mp_subset(g, c.is_nonpos_group).size <= 100000


def test_log1p_set_conditions():
    g = c.log1p_groups()
    for name, a in g.items():
        if c.is_unit_group(name):
            assert np.all((a >= 0.0) & (a <= 1.0)) and not np.signbit(a).any(), name
    a = g["zero_one_and_tiny"]
    assert holds(a, [0.0, c.TINY, 1.0])
    for p in (2.0 ** -60, 2.0 ** -54, 2.0 ** -29):
        assert holds(a, [c.step1(p, -1), p, c.step1(p, 1)])
    a = g["branch_word"]
    w = c.hi_word(a)
    first = c.from_bits([c.LOG1P_BRANCH_WORD << 32])[0]
    assert holds(a, [c.step1(first, j) for j in range(-4, 5)])
    assert (w == c.LOG1P_BRANCH_WORD - 1).any() and (w == c.LOG1P_BRANCH_WORD + 1).any()
    assert holds(a, c.from_bits([(c.LOG1P_BRANCH_WORD << 32) | 0xFFFFFFFF])) and abs(first - (math.sqrt(2) - 1)) < 1e-6
    a = g["sqrt2_cut"]
    u = 1.0 + a
    assert np.all(np.abs(word20(u) - c.SQRT2_WORD) <= 1) and np.all((u >= 1.0) & (u < 2.0))
    for wd in (c.SQRT2_WORD - 1, c.SQRT2_WORD, c.SQRT2_WORD + 1):           # each word: its two ends and thousands of points inside
        lo = c.bits(u[word20(u) == wd]) & np.uint64(0xFFFFFFFF)
        assert lo.min() == 0 and lo.max() == 0xFFFFFFFF and np.unique(lo).size > 3000, hex(wd)
    assert np.any(c.bits(a) & np.uint64(3))                                   # ... and t that are no u - 1: 1 + t rounds
    a = g["hu_zero"]
    assert holds(a, 1.0 - np.arange(65) * 2.0 ** -53)
    hu = word20(1.0 + a)                                                      # gm_log1p_unit: hu = (0x100000 - word) >> 2 after the halving; u = 2: word 0
    is0 = np.where(1.0 + a == 2.0, True, ((0x100000 - hu) >> 2) == 0)
    assert is0[:65].all() and is0[65:].any() and not is0[65:].all()           # the last nine straddle the range's lower end
    a = g["exp_of_random"]
    assert a.size == 100000 and (a == 1.0).any() and (a < 1e-300).any() and ((a > 0.01) & (a < 0.99)).sum() > 10000
    a = g["random"]
    assert a.size == 100000 and a.min() >= 2.0 ** -60 and np.histogram(np.log2(a), bins=6, range=(-60, 0))[0].min() > 10000
    a = g["near_one"]
    assert a.size == 8000 and a.min() >= 0.99 and np.histogram(a, bins=10, range=(0.99, 1.0))[0].min() > 600
    assert tuple(g["scan_worst"]) == c.LOG1P_SCAN_WORST and g["scan_worst"].min() > 0.99
    a = g["gm_log1p_only"]
    assert holds(a, [-1.0, c.step1(-1.0, 1), c.step1(-1.0, -1), -2.0, -c.INF, c.INF, 2.0 ** 53, c.step1(2.0 ** 53, -1), c.DBL_MAX]) and np.isnan(a).sum() == 1
    neg_cut = c.from_bits([(c.LOG1P_NEG_CUT_WORD << 32) | 0xFFFFFFFF])[0]      # the last double of the word: below it (more negative) the reduction
    assert holds(a, [c.step1(neg_cut, j) for j in range(-4, 5)]) and abs(neg_cut + (1 - math.sqrt(0.5))) < 1e-6
    assert ((a > -1.0) & (a < 0)).sum() >= 20000 and (a > 1.0).sum() >= 20000
    assert sum(v.size for v in g.values()) <= 2000000 and c.mp_subset(g, c.is_unit_group).size <= 100000


def test_log_set_conditions():
    g = c.log_groups()
    a = g["f16_positive"]
    assert a.size == c.N_F16_POSITIVE == 31743 and np.all(np.diff(a) > 0) and a[0] == 2.0 ** -24 and a[-1] == 65504.0
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a)
    assert list(g["f32_edges"]) == [2.0 ** -149, 2.0 ** -126, 1.0 - 2.0 ** -24, 1.0]
    a = g["f32_softmax"]
    assert 80000 < a.size <= 100000 and np.array_equal(a.astype(np.float32).astype(np.float64), a) and a.min() > 0 and a.max() <= 1.0
    assert (a < 2.0 ** -126).any() and (a > 0.999).any()
    a = g["near1_ends"].reshape(2, 9)
    assert list(a[:, 4]) == [0.9375, 1.0 + 0x109 / 4096] and np.all(c.bits(a[:, 0]) + 8 == c.bits(a[:, 8]))
    in_near1 = (c.bits(a) - np.uint64(0x3FEE000000000000)) < np.uint64(0x3090000000000)         # gm_log's own test (unsigned wrap-around)
    assert in_near1.tolist() == [[False] * 4 + [True] * 5, [True] * 4 + [False] * 5]
    a = g["table_boundaries"].reshape(len(c.LOG_BINADES), 128, 3)
    for b, rows in zip(c.LOG_BINADES, a):
        assert np.all(np.floor(np.log2(rows[:, 1])) == b), b
        tmp = c.bits(rows) - np.uint64(c.LOG_OFF)
        i = ((tmp >> np.uint64(45)) & np.uint64(127)).astype(np.int64)
        assert np.array_equal(i[:, 1], np.arange(128)) and np.array_equal(i[:, 2], np.arange(128)) and np.array_equal(i[:, 0], (np.arange(128) - 1) % 128)
        assert np.all(c.bits(rows[:, 1]) & np.uint64((1 << 45) - 1) == 0)
    a = g["subnormal_and_extremes"]
    assert holds(a, [c.TINY, c.DBL_MIN, c.DBL_MAX]) and ((a > 0) & (a < c.DBL_MIN)).sum() > 10000 and np.isfinite(a).all()
    a = g["any_positive_double"]
    assert np.all((a >= c.DBL_MIN) & (a <= c.DBL_MAX)) and np.unique(np.floor(np.log2(a))).size > 1500
    a = g["no_probability"]
    assert holds(a, [0.0, -0.0, -c.INF, c.INF]) and np.isnan(a).sum() == 1 and not np.any((a > 0) & (a < c.INF))
    assert sum(v.size for v in g.values()) <= 2000000


def test_lae_and_count4_set_conditions():
    hi, lo, ns = c.lae_pairs()
    assert np.all(hi >= lo) and np.all(hi <= 0.0) and hi[0] == lo[0] == -c.INF and np.all(np.isfinite(hi[1:]))
    assert (hi[:ns] == lo[:ns]).sum() >= 5 and (np.isinf(lo[:ns]) & np.isfinite(hi[:ns])).sum() == len(c.LAE_HI)
    assert set(c.LAE_HI) == {0.0, -2.0 ** -30, -1.0, c.step1(-c.LN2, -1), -c.LN2, c.step1(-c.LN2, 1), -700.0, -7000.0}
    d = set(c.bits(c.flat(c.exp_groups())).tolist())
    for h in c.LAE_HI:
        m = (hi == h)
        m[:ns] = False
        assert m.sum() >= 1000, h
        if h == 0.0:
            assert set(c.bits(lo[m]).tolist()) <= d | {0}                     # hi = 0: lo IS the exp argument (+0 for -0)
    tail = hi[-10000:]
    assert tail.min() >= -8000.0 and np.unique(tail).size == 10000
    x, y = c.both_orders(hi, lo)
    assert x.size == 2 * hi.size <= 2000000 and hi.size <= 100000 and np.array_equal(x[: hi.size], y[hi.size:])
    keys, key = c.count4_cases()
    ref = c.count4_reference(keys, key)
    assert keys.shape == (key.size, 4) and set(ref.tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert np.isnan(key).any() and np.isnan(keys).any() and np.all(ref[np.isnan(key)] == 0)
    assert (keys == key[:, None]).any(axis=1).sum() > 100                     # ties
    z = (keys == 0) & (key[:, None] == 0) & (np.signbit(keys) != np.signbit(key[:, None]))
    assert z.any()                                                            # -0 against +0: equal, not greater


# ------------------------------------------------------------------------------------------------------------- host twin == libm
def check_bits(args, got, want):
    assert c.same_bits(got, want).all(), c.first_mismatches(args, got, want)


def test_host_twin_equals_libm_bit_for_bit(bk, host_libm_is_glibc235_fma):
    if not host_libm_is_glibc235_fma:
        pytest.skip("this host's libm is not glibc 2.35's x86-64 FMA build")
    d = c.flat(c.exp_groups())
    check_bits(d, bk.score_math_host(bk.SM_GM_EXP, d), c.libm_map(math.exp, d))
    t = c.flat(c.log1p_groups())
    check_bits(t, bk.score_math_host(bk.SM_GM_LOG1P, t), c.libm_map(math.log1p, t))
    tu = np.concatenate([v for k, v in c.log1p_groups().items() if c.is_unit_group(k)])
    check_bits(tu, bk.score_math_host(bk.SM_GM_LOG1P_UNIT, tu), c.libm_map(math.log1p, tu))
    x = c.flat(c.log_groups())
    want = c.libm_map(math.log, x)
    check_bits(x, bk.score_math_host(bk.SM_GM_LOG, x), want)
    ok = (x > 0) & (x <= c.DBL_MAX)
    check_bits(x, bk.score_math_host(bk.SM_SAFE_LOG_GX, x), np.where(ok, want, -c.INF))
    a, b = c.both_orders(*c.lae_pairs()[:2])
    check_bits(np.stack([a, b], axis=1), bk.score_math_host(bk.SM_LAE_GX, a, b), c.libm_lae(a, b))


def test_host_twin_refusals(bk):
    from radian_amd import _lib
    L = _lib.load()
    x, y = np.array([-1.0, -2.0]), np.array([-3.0, -0.5])
    sentinel = 12345.0

    def call(which, x_, y_, n, with_out=True):
        out = np.full(2, sentinel)
        rc = L.rd_diag_score_math_host(which, bk._p(x_), bk._p(y_), n, bk._p(out) if with_out else None)
        assert np.all(out == sentinel) or rc == 0
        return rc
    assert call(bk.SM_GM_EXP, x, None, 2) == 0 and call(bk.SM_LAE_GX, x, y, 2) == 0 and call(bk.SM_GM_EXP, x, None, 0) == 0
    for which in (bk.SM_EXP_NONPOS, bk.SM_LOG1P_UNIT, bk.SM_LAE, bk.SM_SAFE_LOG, bk.SM_COUNT4_GT, -1, 11, 1 << 20):
        assert call(which, x, y, 2) == -1, which                              # RD_ERR_ARG: device-only, or unknown
    assert call(bk.SM_GM_EXP, None, None, 2) == -1 and call(bk.SM_LAE_GX, x, None, 2) == -1 and call(bk.SM_GM_LOG, x, None, 2, with_out=False) == -1
    assert call(bk.SM_GM_EXP, x, None, -1) == -1 and call(bk.SM_GM_EXP, x, None, (1 << 24) + 1) == -1
    assert b"2^24" in L.rd_last_error()
    with pytest.raises(bk.RadianHipError):
        bk.score_math_host(bk.SM_LAE, x, y)


# ------------------------------------------------------------------------------------------------------------- libm alone against mpmath
def test_libm_error_against_mpmath():
    """The error measure on a library of published accuracy: glibc states at most 1 ulp for exp, log and log1p in double precision on x86-64
    (manual, "Known Maximum Errors in Math Functions"); any libm that rounds faithfully passes.  The composition's figure is what
    test_gpu_score_math.py prints beside the device's: a record, no limit."""
    d = c.mp_subset(c.exp_groups(), c.is_nonpos_group)
    ref = c.ref_exp(d)
    err = ref.error(c.libm_map(math.exp, d))
    print("libm exp: max %.4f ulp at d = %r; subnormal results %.4f" % (*c.worst(err, d), err[ref.subnormal()].max()))
    assert err.max() < 1.0 and ref.subnormal().sum() > 500
    assert np.all(ref.nearest[d < -745.14] == 0.0) and (d < -745.14).sum() > 20 and ref.nearest[d == 0].tolist()[:2] == [1.0, 1.0]
    t = c.mp_subset(c.log1p_groups(), c.is_unit_group)
    err = c.ref_log1p(t).error(c.libm_map(math.log1p, t))
    print("libm log1p: max %.4f ulp at t = %r" % c.worst(err, t))
    assert err.max() < 1.0
    x = c.mp_subset(c.log_groups(), c.is_positive_group, cap=3000)
    err = c.ref_log(x).error(c.libm_map(math.log, x))
    print("libm log: max %.4f ulp at x = %r" % c.worst(err, x))
    assert err.max() < 1.0
    hi, lo, _ = c.lae_pairs()
    err = c.ref_lae(hi[1:], lo[1:]).error(c.libm_lae(hi[1:], lo[1:]))
    print("libm hi + log1p(exp(lo - hi)): max %.4f ulp at (hi, lo) = %r" % c.worst(err, hi[1:], lo[1:]))
    assert err.max() < 0.5 + 1.0 + 1.0                                        # one rounding and two routines of at most 1 ulp each


def test_error_measure_on_known_values():
    """the unit and the measure themselves, on values worked out by hand"""
    with c.mpmath.workprec(c.MP_PREC):
        one_third = c.mpmath.mpf(1) / 3                                       # 0x1.5555..p-2: the nearest double is 1/3 (1 - 2^-54): error 1/3 ulp
        vals = [one_third, c.mpmath.mpf(1), c.mpmath.ldexp(c.mpmath.mpf(3), -1076), c.mpmath.mpf(0), -one_third]
        ref = c.Reference(vals)
    assert ref.ulp_exp.tolist() == [-54, -52, -1074, -1074, -54]
    got = np.array([1 / 3, 1.0 + 2.0 ** -52, c.TINY, c.TINY, -1 / 3])
    assert np.allclose(ref.error(got), [1 / 3, 1.0, 0.25, 1.0, 1 / 3], rtol=1e-12, atol=0)
    assert np.isnan(ref.error(np.full(5, c.NAN))).all() and np.isinf(ref.error(np.full(5, c.INF))).all()
    with c.mpmath.workprec(c.MP_PREC):
        ref = c.Reference([one_third - 1], unit_of=[-1.0])                    # lae's unit: the larger of |hi| and |e|
    assert ref.ulp_exp.tolist() == [-52] and abs(ref.error(np.array([-2 / 3]))[0] - 1 / 6) < 1e-12
