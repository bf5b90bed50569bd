"""Argument sets and references for the score-arithmetic tests (test_score_math_cpu.py, test_gpu_score_math.py): the scalar routines of
radian_amd/csrc/decode_common.h and glibc_math.h, probed through rd_diag_score_math.  Plain numpy and mpmath, fixed seeds.

A set is an ordered dict  group name -> float64 array.  A group is named after the condition that defines it; test_score_math_cpu.py
asserts that condition group by group (and imports the constants below for it).  `flat(groups)` is the whole set -- what the bit-exact legs
run on, every element --, `mp_subset(groups)` the part the mpmath legs run on: every edge group whole, the large groups thinned by a fixed
stride to at most MP_GROUP_CAP elements each.

The error unit: ulp(e) = 2^(floor(log2 |e|) - 52), at least 2^-1074; error = |got - e| / ulp(e) with e from mpmath at MP_PREC bits.
`Reference` keeps e in units of that ulp as an integer part (< 2^53, exact in a double) and a fraction, so the error of any result array is
three exact numpy operations and no second mpmath pass."""
import functools
import math
from collections import OrderedDict

import mpmath
import numpy as np

MP_PREC = 240
MP_GROUP_CAP = 8000
INF = float("inf")
NAN = float("nan")
DBL_MIN = 2.0 ** -1022
DBL_MAX = float(np.finfo(np.float64).max)
TINY = 2.0 ** -1074
LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------------------- bit helpers
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def hi_word(x):
    return (bits(x) >> np.uint64(32)).astype(np.uint32)


def step(x, k):
    """x moved by k units in the last place (k < 0: towards -inf); +-0 are one point.  Finite x, and no step past +-DBL_MAX."""
    i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    o = np.where(i >= 0, i, np.int64(-(2 ** 63)) - i) + np.int64(k)        # ordered: monotone in x
    return np.where(o >= 0, o, np.int64(-(2 ** 63)) - o).view(np.float64)


def step1(x, k):
    return float(step(np.array([x], dtype=np.float64), k)[0])


def around(points, k):
    """every point with its neighbours up to k units in the last place on both sides, in ascending order per point"""
    p = np.atleast_1d(np.asarray(points, dtype=np.float64))
    return np.stack([step(p, j) for j in range(-k, k + 1)], axis=1).reshape(-1)


def log_uniform(rng, n, lo, hi):
    return np.exp2(rng.uniform(math.log2(lo), math.log2(hi), n))


def flat(groups):
    return np.concatenate([np.asarray(v, dtype=np.float64) for v in groups.values()])


def thin(a, cap=MP_GROUP_CAP):
    a = np.asarray(a, dtype=np.float64)
    return a if a.size <= cap else a[:: -(-a.size // cap)]


def mp_subset(groups, only=None, cap=MP_GROUP_CAP):
    return np.concatenate([thin(v, cap) for k, v in groups.items() if only is None or only(k)])


def same_bits(a, b):
    """elementwise: equal bit patterns, or both NaN (a NaN's payload and sign are not part of any routine's contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def first_mismatches(args, a, b, limit=5):
    """the report of a bit-exact leg: the first `limit` arguments whose results differ, with both bit patterns"""
    bad = np.flatnonzero(~same_bits(a, b))
    rows = []
    for i in bad[:limit]:
        arg = ", ".join(f"{float(v)!r} ({int(bits(v)[0]):#018x})" for v in np.atleast_1d(args[i]))
        rows.append(f"  [{i}] {arg}: {int(bits(a[i])[0]):#018x} ({float(a[i])!r}) != {int(bits(b[i])[0]):#018x} ({float(b[i])!r})")
    return f"{bad.size} of {len(a)} differ\n" + "\n".join(rows)


def _mpf(x):
    return mpmath.mpf(float(x))


def _with_prec(fn):
    def run(*a, **k):
        with mpmath.workprec(MP_PREC):
            return fn(*a, **k)
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


# ------------------------------------------------------------------------------------------------------------- the cuts
@_with_prec
def _cuts():
    ln2 = +mpmath.ln2
    c = {
        "subnormal": float(-1022 * ln2),      # -708.396...: e^d < 2^-1022 below it
        "last_nonzero": float(-1075 * ln2),   # -745.133...: e^d rounds to 0 below it
        "overflow": float(1024 * ln2),        # 709.782...: e^d overflows above it
    }
    c["gm_exp"] = _with_prec(lambda k: float(k * ln2 / 128))                            # k ln2 / 128: where gm_exp's k changes (nearly: its own product is rounded)
    c["exp_nonpos"] = _with_prec(lambda k: float(-(k + mpmath.mpf(0.5)) * ln2))         # -(k + 1/2) ln2: where exp_nonpos's k changes
    c["neg_ln2"] = float(-ln2)
    return c


CUT = _cuts()
EXP_CLAMP = -746.0                       # exp_nonpos: fmax(d, -746)
GM_EXP_BRANCHES = (-512.0, -1024.0)      # gm_exp: |x| >= 512 -> gm_exp_special, |x| >= 1024 -> underflow / overflow
GM_EXP_STRIDE = 3                        # k of the gm_exp cuts k ln2 / 128: every third k (coprime to 128: every table entry is a cut)
GM_EXP_KMIN = -int(math.ceil(745.2 * 128 / LN2))
LOG1P_BRANCH_WORD = 0x3FDA827A           # gm_log1p(_unit): hx >= this word takes the u = 1 + t reduction
SQRT2_WORD = 0x6A09E                     # ... which halves u when the high mantissa word of u reaches this
LOG1P_NEG_CUT_WORD = 0xBFD2BEC3          # gm_log1p: -0.2929 < x takes the reduction-free path (hx <= this word, as a signed int)
LOG_NEAR1 = (1.0 - 2.0 ** -4, 1.0 + float.fromhex("0x1.09p-4"))   # gm_log: [lo, hi) goes through log1p(x - 1) directly
LOG_OFF = 0x3FE6000000000000             # gm_log: z in [OFF, 2 OFF), table interval i = bits 45..51 above OFF
LOG_BINADES = (-1022, -600, -1, 0, 1, 1023)
# the worst arguments of the fast routines that a scan of 4e5 random arguments each found on an MI355X (log1p_unit: t in [0.4, 1], dense next to
# 1; exp_nonpos: d in [-745.2, 0]): kept as fixed points of the sets
LOG1P_SCAN_WORST = (0.9945960893620833, 0.9969707672739021, 0.9923313782417666, 0.9999996096958366, 0.993828754682555)
EXP_SCAN_WORST = (-555.5492400300294, -709.0433661168122)
N_F16_POSITIVE = 0x7C00 - 1              # every positive finite f16: bit patterns 1 .. 0x7BFF


# ------------------------------------------------------------------------------------------------------------- exp
@functools.lru_cache(maxsize=None)
def exp_groups():
    """arguments of exp: d <= 0 in every group but gm_exp_only"""
    rng = np.random.default_rng(20240601)
    g = OrderedDict()
    g["zero_and_tiny"] = np.concatenate([[0.0, -0.0, -TINY, -2 * TINY], around([-2.0 ** -60, -2.0 ** -54, -2.0 ** -53], 1), [-2.0 ** -29]])
    ks = np.arange(0, GM_EXP_KMIN - 1, -GM_EXP_STRIDE)
    g["gm_exp_cuts"] = np.minimum(around([CUT["gm_exp"](int(k)) for k in ks], 2), 0.0)
    g["exp_nonpos_cuts"] = around([CUT["exp_nonpos"](k) for k in range(1076)], 2)
    g["thresholds"] = around([CUT["subnormal"], CUT["last_nonzero"], EXP_CLAMP, *GM_EXP_BRANCHES], 4)
    g["far"] = np.array([-1e308, -INF])
    g["random"] = -log_uniform(rng, 100000, 2.0 ** -60, 746.0)
    g["scan_worst"] = np.array(EXP_SCAN_WORST)
    g["gm_exp_only"] = np.concatenate([around([512.0, CUT["overflow"], 1024.0], 4), [TINY, 2.0 ** -54, 1.0, 709.0, 1e308, INF, NAN],
                                       log_uniform(rng, 20000, 2.0 ** -60, CUT["overflow"])])
    return g


def is_nonpos_group(name):
    return name != "gm_exp_only"


# ------------------------------------------------------------------------------------------------------------- log1p
def _u_with_word(word20, low):
    """u in [1, 2) whose high mantissa word is word20 and whose low word is `low`"""
    return from_bits((np.uint64(0x3FF00000 | word20) << np.uint64(32)) | np.asarray(low, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def log1p_groups():
    """arguments of log1p: t in [0, 1] in every group but gm_log1p_only"""
    rng = np.random.default_rng(20240602)
    g = OrderedDict()
    g["zero_one_and_tiny"] = np.concatenate([[0.0, TINY, 1.0], around([2.0 ** -60, 2.0 ** -54, 2.0 ** -29], 1)])
    w = np.uint64(LOG1P_BRANCH_WORD) << np.uint64(32)
    g["branch_word"] = np.concatenate([around(from_bits([w]), 4), from_bits([w - np.uint64(1), w, w | np.uint64(0xFFFFFFFF), w + np.uint64(1 << 32)])])
    # the sqrt 2 cut: u = 1 + t with high mantissa word SQRT2_WORD - 1, SQRT2_WORD, SQRT2_WORD + 1.  There are 3 * 2^32 such u (and four
    # t for each, t's last place being finer): both ends of every word, every t that rounds onto an end, and a sample of the inside
    ends, inside = [], []
    for word in (SQRT2_WORD - 1, SQRT2_WORD, SQRT2_WORD + 1):
        ends.append(_u_with_word(word, [0, 1, 0xFFFFFFFE, 0xFFFFFFFF]) - 1.0)           # exact: u - 1 for u in [1, 2)
        inside.append(_u_with_word(word, rng.integers(0, 1 << 32, 3500, dtype=np.uint64)) - 1.0)
    t = around(np.concatenate(ends), 4)          # t's last place is a quarter of u's: +-4 covers every t that rounds onto the end and its neighbour
    g["sqrt2_cut"] = np.concatenate([t[in_sqrt2_words(t)], *inside])
    g["hu_zero"] = np.concatenate([1.0 - np.arange(65) * 2.0 ** -53, around([1.0 - 3 * 2.0 ** -20], 4)])
    d = np.concatenate([-log_uniform(rng, 50000, 2.0 ** -60, 746.0), rng.uniform(-50.0, 0.0, 50000)])
    g["exp_of_random"] = np.minimum(np.exp(d), 1.0)
    g["random"] = log_uniform(rng, 100000, 2.0 ** -60, 1.0)
    g["near_one"] = np.random.default_rng(20240606).uniform(0.99, 1.0, 8000)      # s = t / (2 + t) and with it log1p_unit's correction term are largest
    g["scan_worst"] = np.array(LOG1P_SCAN_WORST)
    wn = np.uint64(LOG1P_NEG_CUT_WORD) << np.uint64(32)
    g["gm_log1p_only"] = np.concatenate([
        -log_uniform(rng, 20000, 2.0 ** -60, 1.0), [-1.0, step1(-1.0, 1), step1(-1.0, 2), -0.0],
        around([-2.0 ** -54, -2.0 ** -29], 1),
        [step1(-1.0, -1), -2.0, -1e300, -DBL_MAX, -INF],
        around(from_bits([wn | np.uint64(0xFFFFFFFF)]), 4), from_bits([wn, wn + np.uint64(1 << 32)]),
        around([2.0 ** 53], 2), [2.0 ** 54, 1e300, DBL_MAX],
        log_uniform(rng, 20000, 1.0, 2.0 ** 60), [INF, NAN]])
    return g


def in_sqrt2_words(t):
    return np.abs(((hi_word(1.0 + np.asarray(t)) & 0xFFFFF).astype(np.int64)) - SQRT2_WORD) <= 1


def is_unit_group(name):
    return name != "gm_log1p_only"


# ------------------------------------------------------------------------------------------------------------- log
def softmax_f32(rng, rows, scale):
    z = (rng.standard_normal((rows, 5)) * scale).astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def log_table_boundaries():
    """the 128 interval boundaries of gm_log's table in each of LOG_BINADES, as bit patterns"""
    base = np.uint64(LOG_OFF) + (np.arange(128, dtype=np.uint64) << np.uint64(45))        # in [0.6875, 1.375): binade -1 or 0
    e = (base >> np.uint64(52)).astype(np.int64) - 1023
    return np.concatenate([(base.astype(np.int64) + ((b - e) << 52)).astype(np.uint64) for b in LOG_BINADES])


@functools.lru_cache(maxsize=None)
def log_groups():
    """arguments of log: probabilities as the three row types hold them, the cuts of gm_log, and what is no probability"""
    rng = np.random.default_rng(20240603)
    g = OrderedDict()
    g["f16_positive"] = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    p = np.concatenate([softmax_f32(rng, 10000, 4.0), softmax_f32(rng, 10000, 30.0)]).reshape(-1)      # (peaked rows: down to f32 subnormals)
    g["f32_edges"] = np.array([2.0 ** -149, 2.0 ** -126, 1.0 - 2.0 ** -24, 1.0])
    g["f32_softmax"] = p[p > 0].astype(np.float64)
    g["near1_ends"] = around(LOG_NEAR1, 4)
    g["table_boundaries"] = around(from_bits(log_table_boundaries()), 1)
    g["subnormal_and_extremes"] = np.concatenate([[TINY, 2 * TINY, DBL_MIN - TINY, DBL_MIN, DBL_MIN + TINY, DBL_MAX, step1(DBL_MAX, -1)],
                                                  from_bits(rng.integers(1, 1 << 52, 10000, dtype=np.uint64))])
    g["any_positive_double"] = from_bits(rng.integers(1 << 52, 0x7FF << 52, 50000, dtype=np.uint64))
    g["no_probability"] = np.array([0.0, -0.0, -TINY, -2.0 ** -149, -0.5, -1.0, -DBL_MAX, -INF, INF, NAN])
    return g


def is_positive_group(name):
    return name != "no_probability"


def is_probability_group(name):
    return name in ("f16_positive", "f32_edges", "f32_softmax")


# ------------------------------------------------------------------------------------------------------------- log-add-exp
LAE_HI = (0.0, -2.0 ** -30, -1.0, step1(CUT["neg_ln2"], -1), CUT["neg_ln2"], step1(CUT["neg_ln2"], 1), -700.0, -7000.0)
LAE_PER_HI = 1250


@functools.lru_cache(maxsize=None)
def lae_pairs():
    """(hi, lo, n_special): pairs with hi >= lo, the first n_special of which are x = y or hold a -inf.  hi - lo is drawn from the exp set
    (its d <= 0 groups, thinned to LAE_PER_HI per fixed hi; lo = hi + d rounded).  The tests run both orders of every pair."""
    rng = np.random.default_rng(20240604)
    d = flat(OrderedDict((k, v) for k, v in exp_groups().items() if is_nonpos_group(k)))
    fixed = np.array(LAE_HI)
    eq = np.array([-INF, 0.0, -2.0 ** -30, -1.0, -700.0, -7000.0, -TINY])
    his, los = [eq, fixed], [eq, np.full(fixed.size, -INF)]
    n_special = eq.size + fixed.size
    dd = thin(d, LAE_PER_HI)
    for h in fixed:
        his.append(np.full(dd.size, h))
        los.append(h + dd)
    rh = rng.uniform(-8000.0, 0.0, 10000)
    his.append(rh)
    los.append(rh + d[rng.integers(0, d.size, rh.size)])
    return np.concatenate(his), np.concatenate(los), n_special


def both_orders(hi, lo):
    return np.concatenate([hi, lo]), np.concatenate([lo, hi])


# ------------------------------------------------------------------------------------------------------------- count4_gt
@functools.lru_cache(maxsize=None)
def count4_cases():
    """(keys [n, 4], key [n]): few distinct values so that ties are the rule, with +-0, +-inf and NaN among them"""
    rng = np.random.default_rng(20240605)
    pool = np.array([0.0, -0.0, INF, -INF, NAN, -1.5, -1.5, 2.25, -TINY, TINY, -700.0, 1e300, -1e300, -3.0, step1(-3.0, 1), step1(-3.0, -1)])
    n = 1000
    return pool[rng.integers(0, pool.size, (n, 4))], pool[rng.integers(0, pool.size, n)]


def count4_reference(keys, key):
    with np.errstate(invalid="ignore"):
        return (keys > key[:, None]).sum(axis=1).astype(np.float64)      # NaN compares false


# ------------------------------------------------------------------------------------------------------------- references
class Reference:
    """the exact values e of one leg in units of their own ulp: e = (m_int + m_frac) 2^ulp_exp, m_int an integer below 2^53"""

    def __init__(self, values, unit_of=None):
        n = len(values)
        self.m_int, self.m_frac, self.ulp_exp, self.nearest = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
        with mpmath.workprec(MP_PREC):
            for i, e in enumerate(values):
                u = e if unit_of is None else max(abs(e), abs(_mpf(unit_of[i])))
                ue = max(u.man.bit_length() + u.exp - 1 - 52, -1074) if u != 0 else -1074      # floor(log2 |u|) - 52
                m = mpmath.ldexp(abs(e), -ue)
                mi = mpmath.floor(m)
                s = -1.0 if e < 0 else 1.0
                self.m_int[i], self.m_frac[i], self.ulp_exp[i], self.nearest[i] = s * float(mi), s * float(m - mi), ue, float(e)

    def error(self, got):
        """|got - e| / ulp, elementwise (exact up to the rounding of the result itself; inf or NaN for a non-finite got)"""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.abs((np.ldexp(got, -self.ulp_exp) - self.m_int) - self.m_frac)

    def subnormal(self):
        return np.abs(self.nearest) < DBL_MIN


def worst(err, *args):
    """(max error, its arguments) for the printed record"""
    i = int(np.nanargmax(np.where(np.isnan(err), INF, err)))
    return float(err[i]), tuple(float(a[i]) for a in args)


@_with_prec
def ref_exp(d):
    return Reference([mpmath.exp(_mpf(v)) if v > -1e6 else mpmath.mpf(0) for v in d])      # (e^-1e6 is 10^-434294: 0 to any number of ulps)


@_with_prec
def ref_log1p(t):
    return Reference([mpmath.log1p(_mpf(v)) for v in t])


@_with_prec
def ref_log(x):
    return Reference([mpmath.log(_mpf(v)) for v in x])


@_with_prec
def ref_lae(hi, lo):
    """log(e^hi + e^lo) = hi + log1p(e^(lo - hi)) for FINITE hi >= lo (lo may be -inf), in ulps of the larger of |hi| and |result|"""
    out = []
    for h, l in zip(hi, lo):
        h_, dm = _mpf(h), (_mpf(l) - _mpf(h) if l > -INF else None)
        out.append(h_ + (mpmath.log1p(mpmath.exp(dm)) if dm is not None and dm > -1e6 else 0))
    return Reference(out, unit_of=hi)


def libm_lae(x, y):
    """numpy's npy_logaddexp through the running libm, element by element (numpy's own vector loops are not libm)"""
    out = np.empty(len(x))
    for i, (a, b) in enumerate(zip(x, y)):
        a, b = float(a), float(b)
        if a == b:
            out[i] = a + LN2
        else:
            h, l = max(a, b), min(a, b)
            out[i] = h + math.log1p(math.exp(l - h))
    return out


def libm_map(fn, x):
    """fn of math (exp, log, log1p) element by element; a ValueError (log of a negative, log1p below -1) is NaN, a pole -inf, an
    OverflowError +inf, as the C function returns them"""
    out = np.empty(len(x))
    for i, v in enumerate(x):
        v = float(v)
        try:
            out[i] = fn(v)
        except ValueError:
            out[i] = -INF if (fn is math.log and v == 0.0) or (fn is math.log1p and v == -1.0) else NAN
        except OverflowError:
            out[i] = INF
    return out
