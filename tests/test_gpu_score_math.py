"""The beam search's scalar score arithmetic on the device, routine by routine (rd_diag_score_math: a kernel that calls the routines of
csrc/decode_common.h and csrc/glibc_math.h themselves), on the argument sets of tests/_score_math_cases.py:

* the glibc arithmetic (gm_exp, gm_log, gm_log1p, gm_log1p_unit, lae_gx, safe_log<true>) equals the same header compiled for the host bit
  for bit on every element -- and the running libm, where that is glibc 2.35's FMA build (test_score_math_cpu.py holds the host twin
  against libm on the same sets);
* the fast arithmetic (exp_nonpos, log1p_unit, lae) stays within its stated error against mpmath; the device library's log is recorded;
* safe_log's guard, count4_gt, and the entry point's refusals."""
import math

import numpy as np
import pytest

import _score_math_cases as c

pytestmark = pytest.mark.gpu

# the project's stated figures (csrc/decode_common.h), in ulps
LIM_EXP = 0.68
LIM_EXP_SUBNORMAL = 0.68 + 0.5      # in units of 2^-1074: ldexp rounds the 0.68-ulp result a second time
# log1p_unit: the stated 0.63 was an overstated claim.  Next to t = 1 the routine reaches 0.7103 ulp against mpmath (t = 0.9945960893620833):
# the s^3 / 3 term of its series takes the rounded quotient -- no defect, the result stays faithfully rounded.  The claim is
# corrected in decode_common.h, DESIGN.md 4.4 and DESIGN_LOG.md, and the limit is that figure rounded up at the second decimal; lae's limit
# keeps the sum as first stated.
LIM_LOG1P = 0.72
# lae = hi + log1p_unit(exp_nonpos(lo - hi)): the final addition rounds once (0.5); d log1p(e) / de * e / log1p(e) <= 1, so exp's relative
# error reaches log1p's result at most at full size (0.68, counted in the unit's ulps: log1p(e) <= |hi| or <= |result|); log1p's own (0.63)
LIM_LAE = 0.5 + 0.68 + 0.63


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def bk():
    from radian_amd import backend
    return backend


def check_bits(what, args, got, want):
    assert c.same_bits(got, want).all(), what + ": " + c.first_mismatches(args, got, want)


def test_glibc_routines_equal_the_host_twin_bit_for_bit(be, bk, host_libm_is_glibc235_fma):
    """every element of every set; a failure lists the first five arguments with both bit patterns"""
    libm = host_libm_is_glibc235_fma
    print("the running libm is glibc 2.35's FMA build:", libm)
    d = c.flat(c.exp_groups())
    t = c.flat(c.log1p_groups())
    tu = np.concatenate([v for k, v in c.log1p_groups().items() if c.is_unit_group(k)])
    x = c.flat(c.log_groups())
    for name, which, a, fn in (("gm_exp", bk.SM_GM_EXP, d, math.exp), ("gm_log", bk.SM_GM_LOG, x, math.log), ("gm_log1p", bk.SM_GM_LOG1P, t, math.log1p),
                               ("gm_log1p_unit", bk.SM_GM_LOG1P_UNIT, tu, math.log1p), ("safe_log<true>", bk.SM_SAFE_LOG_GX, x, None)):
        got = be.score_math(which, a)
        assert got.size == a.size
        check_bits(name + " device / host", a, got, bk.score_math_host(which, a))
        if libm and fn is not None:
            check_bits(name + " device / libm", a, got, c.libm_map(fn, a))
    p, q = c.both_orders(*c.lae_pairs()[:2])
    got = be.score_math(bk.SM_LAE_GX, p, q)
    check_bits("lae_gx device / host", np.stack([p, q], axis=1), got, bk.score_math_host(bk.SM_LAE_GX, p, q))
    if libm:
        check_bits("lae_gx device / libm", np.stack([p, q], axis=1), got, c.libm_lae(p, q))


@pytest.mark.parametrize("variant", ["fast", "glibc"])
def test_safe_log_guard_and_order(be, bk, variant):
    which = bk.SM_SAFE_LOG if variant == "fast" else bk.SM_SAFE_LOG_GX
    g = c.log_groups()
    bad = g["no_probability"]
    got = be.score_math(which, bad)
    assert np.all(got == -c.INF), list(zip(bad.tolist(), got.tolist()))       # 0, -0.0, negatives, NaN, +inf: probability 0
    for name, a in (("f16", g["f16_positive"]), ("f32", np.concatenate([g["f32_edges"], g["f32_softmax"]]))):
        a = np.unique(a)                                                      # sorted
        got = be.score_math(which, a)
        down = np.flatnonzero(~(np.diff(got) >= 0))
        assert down.size == 0, (name, [(a[i], a[i + 1], got[i], got[i + 1]) for i in down[:5]])
        assert np.isfinite(got).all() and got[a == 1.0].tolist() == [0.0] and not np.signbit(got[a == 1.0]).any()      # log 1 = +0


@pytest.fixture(scope="module")
def refs():
    """the mpmath references of the accuracy legs, once"""
    d = c.mp_subset(c.exp_groups(), c.is_nonpos_group)
    t = c.mp_subset(c.log1p_groups(), c.is_unit_group)
    x = c.mp_subset(c.log_groups(), c.is_positive_group, cap=3000)
    hi, lo, _ = c.lae_pairs()
    hi, lo = hi[1:], lo[1:]                                                   # (pair 0 is -inf, -inf: exact, below)
    return {"exp": (d, c.ref_exp(d)), "log1p": (t, c.ref_log1p(t)), "log": (x, c.ref_log(x)), "lae": (hi, lo, c.ref_lae(hi, lo))}


def test_fast_routines_against_mpmath(be, bk, refs):
    """Every figure is printed before anything is asserted (run with -s for the record of DESIGN.md 4.4).

    Measured on an MI355X on these sets (ulp): exp_nonpos 0.6441 at d = -555.5492400300294, on subnormal results 0.7487 at d = -709.0433661168122;
    log1p_unit 0.7103 at t = 0.9945960893620833; lae 0.9376 at (0, -18.227604763787305), libm's composition the same; the device library's
    log 0.6192 at x = 1.0625."""
    fails = []

    def limit(what, err, lim, *args):
        w, at = c.worst(err, *args)
        print(f"{what}: max {w:.4f} ulp at {at!r} (limit {lim})")
        if not np.all(err <= lim):                                            # (a NaN error fails)
            fails.append(f"{what}: {w:.4f} ulp at {at!r} > {lim}")

    d, ref = refs["exp"]
    got = be.score_math(bk.SM_EXP_NONPOS, d)
    err = ref.error(got)
    sub = ref.subnormal()
    limit("exp_nonpos, normal results", err[~sub], LIM_EXP, d[~sub])
    limit("exp_nonpos, subnormal results (units of 2^-1074)", err[sub], LIM_EXP_SUBNORMAL, d[sub])
    full = np.concatenate([v for k, v in c.exp_groups().items() if c.is_nonpos_group(k)])
    got = be.score_math(bk.SM_EXP_NONPOS, full)
    zero = full < -745.14                                                     # (-inf among them)
    assert zero.sum() > 20 and np.isinf(full[zero]).any()
    if not (np.all(got[zero] == 0.0) and not np.signbit(got[zero]).any()):
        fails.append(f"exp_nonpos: not 0 at d = {full[zero][got[zero] != 0.0][:5].tolist()}")
    if not (np.all(got[full == 0.0] == 1.0) and (full == 0.0).sum() >= 2):
        fails.append("exp_nonpos(+-0) != 1")
    if not np.all((got >= 0.0) & (got <= 1.0)):
        fails.append(f"exp_nonpos outside [0, 1] at d = {full[~((got >= 0.0) & (got <= 1.0))][:5].tolist()}")

    t, ref = refs["log1p"]
    limit("log1p_unit", ref.error(be.score_math(bk.SM_LOG1P_UNIT, t)), LIM_LOG1P, t)

    hi, lo, ref = refs["lae"]
    p, q = c.both_orders(hi, lo)
    got = be.score_math(bk.SM_LAE, p, q)
    err = np.concatenate([ref.error(got[: hi.size]), ref.error(got[hi.size:])])
    limit("lae (hi + log1p_unit(exp_nonpos(lo - hi)), both orders)", err, LIM_LAE, p, q)
    w, at = c.worst(ref.error(c.libm_lae(hi, lo)), hi, lo)
    print(f"    libm's hi + log1p(exp(lo - hi)) on the same pairs: max {w:.4f} ulp at {at!r} (a record, no limit)")
    if not np.array_equal(c.bits(got[: hi.size]), c.bits(got[hi.size:])):
        fails.append("lae(x, y) != lae(y, x)")
    ninf = np.array([-c.INF])
    if not be.score_math(bk.SM_LAE, ninf, ninf)[0] == -c.INF:
        fails.append("lae(-inf, -inf) != -inf")

    # safe_log<false> is the device library's log.  The documentation that ROCm installs (/opt/rocm/share: doc/, html/) holds no accuracy
    # statement for double-precision log -- no text file under it names an ulp figure --, so the figure is recorded and no bound asserted.
    x, ref = refs["log"]
    err = ref.error(be.score_math(bk.SM_SAFE_LOG, x))
    w, at = c.worst(err, x)
    print(f"safe_log<false> (the device library's log): max {w:.4f} ulp at {at!r} (recorded, no documented bound)")
    assert not fails, "\n".join(fails)


def test_count4_gt_equals_the_numpy_count(be, bk):
    keys, key = c.count4_cases()
    got = be.score_math(bk.SM_COUNT4_GT, keys.reshape(-1), key)
    want = c.count4_reference(keys, key)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(keys[i].tolist(), key[i], got[i], want[i]) for i in bad[:5]]


def test_refusals_leave_out_untouched(be, bk):
    L, h = be._L, be._h
    x, y = np.array([-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0]), np.array([-3.0, -0.5])
    sentinel = 12345.0

    def call(which, x_, y_, n, with_out=True, ctx=h):
        out = np.full(2, sentinel)
        rc = L.rd_diag_score_math(ctx, which, bk._p(x_), bk._p(y_), n, bk._p(out) if with_out else None)
        assert rc == 0 or np.all(out == sentinel)
        return rc, out
    for which in (-1, 11, 1 << 20):
        assert call(which, x, y, 2)[0] == -1, which
    assert call(bk.SM_GM_EXP, None, None, 2)[0] == -1 and call(bk.SM_LAE, x, None, 2)[0] == -1 and call(bk.SM_COUNT4_GT, x, None, 2)[0] == -1
    assert call(bk.SM_GM_LOG, x, None, 2, with_out=False)[0] == -1 and call(bk.SM_GM_EXP, x, None, 2, ctx=None)[0] == -1
    assert call(bk.SM_GM_EXP, x, None, -1)[0] == -1 and call(bk.SM_GM_EXP, x, None, (1 << 24) + 1)[0] == -1
    assert b"2^24" in L.rd_last_error()
    rc, out = call(bk.SM_GM_EXP, x, None, 0)
    assert rc == 0 and np.all(out == sentinel)                                # n = 0: nothing to do
    rc, out = call(bk.SM_EXP_NONPOS, x, None, 2)                              # y may be null for a one-argument routine
    assert rc == 0 and np.allclose(out, np.exp(x[:2]), rtol=1e-15)
    rc, out = call(bk.SM_COUNT4_GT, x, y, 2)
    assert rc == 0 and out.tolist() == [2.0, 0.0]
    # more than one workgroup, a last one that is not full, and no element past n written
    n = 256 * 3 + 5
    a = -np.arange(n + 256, dtype=np.float64)
    out = np.full(n + 256, sentinel)
    assert L.rd_diag_score_math(h, bk.SM_GM_EXP, bk._p(a), None, n, bk._p(out)) == 0
    assert np.all(out[n:] == sentinel) and np.array_equal(out[:n], bk.score_math_host(bk.SM_GM_EXP, a[:n]))
