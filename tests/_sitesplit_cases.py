"""TEST INFRASTRUCTURE: seeded inputs of the two-cluster split.  Every group is a dict: name, site (uint32), cond
(uint8), value (int16), n_sites, min_frac_q16 (one per call) and cond_of: {site: predicate over (that site's entry of the restatement
tests/_sitesplit_ref.py, its values a, b)} -- the group's defining condition, asserted without a GPU by tests/test_sitesplit_cpu.py.
Sizes follow the kernels' constants: 64 lanes and the chunk of C = 256 sorted elements of a site one wave takes (a site's sorted
elements are sample 0 ascending, then sample 1 ascending)."""
import functools
import math
import random
from bisect import bisect_right

import numpy as np

import _sitesplit_ref as ref

LANES, C = 64, 256
DEPTHS = (1, 2, 3, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5)


def _group(name, per_site, n_sites, cond, min_frac_q16=0, rng=None):
    """per_site: {site: (values of sample 0, values of sample 1)}; the events site by site unless rng shuffles them"""
    site, cnd, value = [], [], []
    for s, (a, b) in per_site.items():
        site += [s] * (len(a) + len(b))
        cnd += [0] * len(a) + [1] * len(b)
        value += list(a) + list(b)
    site, cnd, value = np.array(site, dtype=np.uint32), np.array(cnd, dtype=np.uint8), np.array(value, dtype=np.int16)
    if rng is not None:
        p = rng.permutation(len(site))
        site, cnd, value = site[p], cnd[p], value[p]
    return dict(name=name, site=site, cond=cnd, value=value, n_sites=n_sites, min_frac_q16=min_frac_q16, cond_of=cond)


def _draw(rng, n, spread=30, centre=0):
    """n values with many ties: a rounded Gaussian"""
    return np.clip(np.rint(centre + spread * rng.standard_normal(n)), -32768, 32767).astype(np.int64).tolist()


def _mix(rng, n, frac=0.5, shift=150):
    """n values of two overlapping clusters"""
    k = int(round(frac * n))
    return _draw(rng, n - k) + _draw(rng, k, centre=shift)


def score_cmp(c1, c2):
    """the sign of J(c1) - J(c2) for two candidates (cut, D, n_lo, n_hi), in Python integers"""
    l, r = c1[1] ** 2 * (c2[2] * c2[3]), c2[1] ** 2 * (c1[2] * c1[3])
    return (l > r) - (l < r)


def ranked(a, b, min_frac_q16=0):
    """the admissible cuts, the best first (the order rd_site_split picks by: J, then the smaller cut)"""
    return sorted(ref.cuts(list(a), list(b), min_frac_q16), key=functools.cmp_to_key(lambda x, y: -score_cmp(x, y) or (x[0] > y[0]) - (x[0] < y[0])))


def depths_group():
    """total depths 1 .. 3C + 5 split at random between the samples (sites 0 ..), and the same depths as n0 against a short sample 1"""
    rng = np.random.default_rng(2601)
    per, cond = {}, {}
    for i, d in enumerate(DEPTHS):
        n0 = min(max(int(rng.integers(0, d + 1)), 1), d - 1) if d > 1 else 1
        per[i] = (_mix(rng, n0), _draw(rng, d - n0, centre=8))
        cond[i] = (lambda d: lambda e, a, b: sum(e["n"]) == d and e["status"] == (ref.OK if d > 1 else ref.ONE_SIDED))(d)
        per[100 + i] = (_mix(rng, d), _draw(rng, int(rng.integers(1, 70)), centre=-5))
        cond[100 + i] = (lambda d: lambda e, a, b: e["n"][0] == d and e["status"] == ref.OK and e["n_cuts"] >= 1)(d)
    return _group("depths", per, 200, cond, rng=rng)


def sided_group():
    rng = np.random.default_rng(2602)
    per = {3: ([], _mix(rng, 70)), 4: (_mix(rng, 70), []), 9: (_draw(rng, 1), _mix(rng, C + 1)), 10: (_mix(rng, C + 1), _draw(rng, 1))}
    zero = lambda e: (e["cut"], e["n_cuts"], e["n_lo"], e["sum_lo"], e["sumsq_lo"]) == (0, 0, (0, 0), (0, 0), (0, 0))
    cond = {3: lambda e, a, b: e["status"] == ref.ONE_SIDED and e["n"] == (0, 70) and zero(e) and e["sumsq"][1] > 0,
            4: lambda e, a, b: e["status"] == ref.ONE_SIDED and e["n"] == (70, 0) and zero(e) and e["sumsq"][0] > 0,
            9: lambda e, a, b: e["status"] == ref.OK and e["n"] == (1, C + 1),
            10: lambda e, a, b: e["status"] == ref.OK and e["n"] == (C + 1, 1)}
    return _group("sided", per, 11, cond, rng=rng)


def degenerate_group():
    """every value of a site equal: no cut (NONE), inside one chunk and over two; exactly two distinct values: one cut"""
    per = {0: ([7] * 40, [7] * 90), 1: ([-300] * (C + 3), [-300] * 2), 2: ([5] * 30 + [9] * 10, [9] * 25 + [5] * 5), 3: ([-1], [1])}
    none = lambda e, a, b: e["status"] == ref.NONE and (e["cut"], e["n_cuts"], e["n_lo"]) == (0, 0, (0, 0)) and e["sumsq"][0] > 0
    cond = {0: none, 1: none,
            2: lambda e, a, b: (e["status"], e["cut"], e["n_cuts"], e["n_lo"], e["sum_lo"]) == (ref.OK, 5, 1, (30, 5), (150, 25)),
            3: lambda e, a, b: (e["status"], e["cut"], e["n_cuts"], e["n_lo"], e["sumsq_lo"]) == (ref.OK, -1, 1, (1, 0), (1, 0))}
    return _group("degenerate", per, 4, cond)


def tie_group():
    """values 0, 1, 2 with equal multiplicities in both samples: J(0) = J(1) as integers, the smaller cut wins; with multiplicity 100 the
    two cuts are evaluated by different waves (sorted elements 99 / 199 of sample 0) and met by the pick"""
    per = {0: ([0, 1, 2] * 2, [0, 1, 2] * 2), 1: ([0, 1, 2] * 100, [2, 1, 0] * 100), 2: ([-2, 0, 2], [-2, 0, 2])}

    def tied(e, a, b):
        c = ref.cuts(a, b, 0)
        return len(c) == 2 and score_cmp(c[0], c[1]) == 0 and c[0][1] != 0 and e["cut"] == c[0][0] == min(a) and e["n_cuts"] == 2
    return _group("tie", per, 3, {0: tied, 1: tied, 2: tied})


FRAC_N, FRAC_Q16 = 128, 5120          # 5120 * 128 == 65536 * 10: a cluster of 10 events of 128 is admissible, one of 9 is not


def min_frac_group():
    """min_frac_q16 = 5120 at N = 128: the unconstrained best cut leaves 9 events on the low side (site 0), on the high side (site 1);
    10 events on the low side is admissible and chosen (site 2)"""
    rng = np.random.default_rng(2605)
    bulk = lambda n: _draw(rng, n, spread=40)
    per = {0: ([-3000] * 5 + bulk(59), [-3000] * 4 + bulk(60)), 1: ([3000] * 4 + bulk(60), [3000] * 5 + bulk(59)),
           2: ([-3000] * 5 + bulk(59), [-3000] * 5 + bulk(59))}

    def short(side):
        def pred(e, a, b):
            free = ranked(a, b, 0)[0]
            return (len(a) + len(b) == FRAC_N and free[2 + side] == 9 and 65536 * 9 < FRAC_Q16 * FRAC_N == 65536 * 10 and e["status"] == ref.OK
                    and e["cut"] != free[0] and min(sum(e["n_lo"]), FRAC_N - sum(e["n_lo"])) >= 10 and e["n_cuts"] < len(ref.cuts(a, b, 0)))
        return pred
    cond = {0: short(0), 1: short(1), 2: lambda e, a, b: sum(e["n_lo"]) == 10 and e["cut"] == -3000 and ranked(a, b, 0)[0][0] == -3000}
    assert FRAC_Q16 * FRAC_N == 65536 * 10
    return _group("min_frac", per, 3, cond, min_frac_q16=FRAC_Q16, rng=rng)


def half_group():
    """min_frac_q16 = 32768: both clusters must hold exactly half of the events"""
    per = {0: ([1, 2, 3, 4], [5, 6, 7, 8]), 1: ([1, 2, 3], [5, 6, 7, 8]), 2: ([1, 2, 4, 4], [4, 4, 7, 8]), 3: ([10] * 100 + [50] * 28, [50] * 100 + [10] * 28)}
    cond = {0: lambda e, a, b: (e["status"], e["cut"], e["n_cuts"], e["n_lo"]) == (ref.OK, 4, 1, (4, 0)),
            1: lambda e, a, b: e["status"] == ref.NONE and len(a) + len(b) == 7,
            2: lambda e, a, b: e["status"] == ref.NONE and len(ref.cuts(a, b, 0)) == 4,
            3: lambda e, a, b: (e["status"], e["cut"], e["n_cuts"], e["n_lo"]) == (ref.OK, 10, 1, (100, 28))}
    return _group("half", per, 4, cond, min_frac_q16=32768)


def locations_group():
    """where the chosen cut is evaluated: a value of sample 1 alone; sorted element C - 1 (the last of a chunk) and C (the first of the
    next) of sample 0; an element of the site's third chunk"""
    rng = np.random.default_rng(2607)
    low = lambda n, top: sorted(_draw(rng, n - 1, spread=20, centre=top - 80))[::-1] + [top]
    per, cond = {}, {}
    per[0] = ([v for v in low(40, -500) if v != -500] + _draw(rng, 30, centre=600), low(40, -470) + _draw(rng, 30, centre=600))
    cond[0] = lambda e, a, b: e["cut"] == -470 and -470 not in a and -470 in b and max(v for v in a + b if v < 0) == -470
    for s, n_low in ((1, C), (2, C + 1), (3, 2 * C + 40)):
        vals = [min(v, -601) for v in low(n_low, -600)[:-1]] + [-600]           # -600 once, the largest low value of sample 0
        per[s] = (vals + _draw(rng, 100, centre=700), [min(v, -601) for v in _draw(rng, 50, spread=20, centre=-700)] + _draw(rng, 60, centre=700))
        cond[s] = (lambda n_low: lambda e, a, b: e["cut"] == -600 and a.count(-600) == 1 and -600 not in b
                   and bisect_right(sorted(a), -600) - 1 == n_low - 1)(n_low)
    assert 2 * C <= 2 * C + 40 - 1 < 3 * C
    return _group("locations", per, 4, cond, rng=rng)


def wide_sites_group():
    """site ids 0 and 2^32 - 2 with n_sites = 2^32 - 1"""
    rng = np.random.default_rng(2608)
    top = (1 << 32) - 2
    per = {top: (_mix(rng, 66), _draw(rng, 65)), 0: (_mix(rng, 10), _draw(rng, 12)), 1 << 31: (_mix(rng, 3), _draw(rng, 3))}
    cond = {top: lambda e, a, b: e["out_site"] == top and e["status"] == ref.OK, 0: lambda e, a, b: e["out_site"] == 0 and e["status"] == ref.OK}
    return _group("wide_sites", per, (1 << 32) - 1, cond, rng=rng)


def interleaved_group():
    """no site is contiguous in the input: event i belongs to site i mod 7"""
    rng = np.random.default_rng(2609)
    n = 7 * 90
    site = (np.arange(n) % 7).astype(np.uint32) * 11
    cond = rng.integers(0, 2, n).astype(np.uint8)
    value = np.array(_draw(rng, n), dtype=np.int16) + (200 * (rng.random(n) < 0.3) * (cond == 0)).astype(np.int16)
    return dict(name="interleaved", site=site, cond=cond, value=value, n_sites=100, min_frac_q16=0,
                cond_of={0: lambda e, a, b: sum(e["n"]) == 90 and e["status"] == ref.OK})


# ---------------------------------------------------------------------------------------------- the near-tie
def _convergents(P, Q, limit):
    """the convergents X / Y of sqrt(Q / P) with X, Y <= limit: P X^2 - Q Y^2 is small against either term"""
    D = P * Q
    r = math.isqrt(D)
    if r * r == D:
        return
    m, d, h0, h1, k0, k1 = 0, P, 0, 1, 1, 0
    while d:
        a = (m + r) // d
        h0, h1, k0, k1 = h1, a * h1 + h0, k1, a * k1 + k0
        if h1 > limit or k1 > limit:
            return
        yield h1, k1
        m = a * d - m
        if (D - m * m) % d:
            return
        d = (D - m * m) // d


NEAR_TIE_BOXES = ((-32768, -12000), (-4000, 4000), (12000, 32767))     # the values of the low, middle and high cluster


def find_near_tie(seed):
    """A seeded search for three tight clusters of n1, t, n3 values with sums S1, T, H whose two cluster-boundary cuts have scores
    D1^2 / (n1 (t + n3)) and D2^2 / ((n1 + t) n3) that differ by less than one part in 2^55: (n1 + t) n3 D1^2 - n1 (t + n3) D2^2 = k
    small and not zero, D1 / D2 a convergent of the square root of the ratio of the two products (a Pell-like equation), D1 above 2^27;
    then D1 = S1 (t + n3) - n1 (T + H), D2 = (S1 + T) n3 - (n1 + t) H solved for integer sums inside the clusters' boxes.  About a minute;
    the tests use its recorded result NEAR_TIE (seed 26) and assert the property itself."""
    rng = random.Random(seed)
    LO, MID, HI = NEAR_TIE_BOXES
    while True:
        n1, t, n3 = rng.randint(20, 120), rng.randint(20, 120), rng.randint(20, 120)
        N, Q, P = n1 + t + n3, n1 * (t + n3), (n1 + t) * n3
        for X, Y in _convergents(P, Q, 1 << 40):
            if X < (1 << 27) or P * X * X == Q * Y * Y:
                continue
            d1_lo = LO[0] * n1 * (t + n3) - n1 * (MID[1] * t + HI[1] * n3)
            d1_hi = LO[1] * n1 * (t + n3) - n1 * (MID[0] * t + HI[0] * n3)
            for g in list(range(max(1, -d1_hi // X), -d1_lo // X + 1))[:8]:
                D1, D2, det = -g * X, -g * Y, n1 * N
                S1 = np.arange(LO[0] * n1, LO[1] * n1 + 1, dtype=np.int64)
                r1, r2 = D1 - (t + n3) * S1, D2 - n3 * S1
                Tn, Hn = -(n1 + t) * r1 + n1 * r2, -n3 * r1 - n1 * r2
                T, H = Tn // det, Hn // det
                ok = (Tn % det == 0) & (Hn % det == 0) & (T >= MID[0] * t) & (T <= MID[1] * t) & (H >= HI[0] * n3) & (H <= HI[1] * n3)
                if ok.any():
                    i = int(np.flatnonzero(ok)[0])
                    return (n1, t, n3), (int(S1[i]), int(T[i]), int(H[i]))


NEAR_TIE = ((114, 44, 73), (-3667667, -175985, 1919638))               # find_near_tie(26)


def near_tie_values(found=NEAR_TIE):
    """the three clusters: n values of sum S are S mod n times floor(S / n) + 1 and the rest floor(S / n)"""
    out = []
    for n, S in zip(*found):
        q, r = divmod(S, n)
        out.append([q + 1] * r + [q] * (n - r))
    return out


def fp64_scores(c):
    """a candidate's score as a kernel would form it in fp64: from the exact square, and from the product of two doubles"""
    return float(c[1] ** 2) / float(c[2] * c[3]), float(c[1]) * float(c[1]) / (float(c[2]) * float(c[3]))


def near_tie_group():
    """the two best cuts' scores differ as integers, yet their fp64 quotients compare equal or in the wrong order: a kernel that compares
    in floating point, or in 64 bits, picks the other cut.  Site 0 as found; site 1 the same values negated (the order of the two cuts
    reversed); the elements of every cluster alternate between the samples"""
    lo, mid, hi = near_tie_values()
    vals = lo + mid + hi
    per = {0: (vals[0::2], vals[1::2]), 1: ([-v for v in vals[1::2]], [-v for v in vals[0::2]])}

    def pred(e, a, b):
        first, second = ranked(a, b, 0)[:2]
        if score_cmp(first, second) != 1 or e["cut"] != first[0]:
            return False
        return all(f <= s for f, s in zip(fp64_scores(first), fp64_scores(second)))
    return _group("near_tie", per, 2, {0: pred, 1: pred})


def all_groups():
    return [depths_group(), sided_group(), degenerate_group(), tie_group(), min_frac_group(), half_group(), locations_group(), wide_sites_group(),
            interleaved_group(), near_tie_group()]


@functools.lru_cache(maxsize=None)
def deep_group():
    """N = 2^16 at the int16 extremes (site 5: two cuts, -32768 and 0, whose cross products take 122 bits), N = 2^16 of drawn values (site
    6: the deepest site that is split) and N = 2^16 + 1 (site 2: DEEP), interleaved"""
    rng = np.random.default_rng(2610)
    q = 1 << 14
    a5, b5 = [-32768] * q + [32767] * q, [-32768] * (q - 1) + [0] + [32767] * q
    n6, n2 = 1 << 16, (1 << 16) + 1
    c6, c2 = rng.integers(0, 2, n6), rng.integers(0, 2, n2)
    v6 = np.clip(np.rint(400 * rng.standard_normal(n6) + 900 * (rng.random(n6) < 0.4) * (c6 == 0)), -32768, 32767)
    v2 = np.clip(np.rint(400 * rng.standard_normal(n2)), -32768, 32767)
    site = np.concatenate([np.full(2 * q + 2 * q, 5), np.full(n6, 6), np.full(n2, 2)]).astype(np.uint32)
    cond = np.concatenate([np.zeros(2 * q), np.ones(2 * q), c6, c2]).astype(np.uint8)
    value = np.concatenate([a5, b5, v6, v2]).astype(np.int16)
    p = rng.permutation(len(site))

    def extreme(e, a, b):
        c = ref.cuts(a, b, 0)
        bits = max(x[1] ** 2 * (y[2] * y[3]) for x in c for y in c).bit_length()
        return sum(e["n"]) == 1 << 16 and [x[0] for x in c] == [-32768, 0] and 121 <= bits <= 122 and max(abs(x[1]) for x in c) <= 1 << 46
    return dict(name="deep", site=site[p], cond=cond[p], value=value[p], n_sites=8, min_frac_q16=0,
                cond_of={5: extreme, 6: lambda e, a, b: sum(e["n"]) == 1 << 16 and e["status"] == ref.OK and e["n_cuts"] > 1000,
                         2: lambda e, a, b: sum(e["n"]) == (1 << 16) + 1 and e["status"] == ref.DEEP and (e["cut"], e["n_cuts"], e["n_lo"]) == (0, 0, (0, 0))
                         and e["sumsq"][0] > 0})


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's entries of a group, computed once and shared by the tests (never modified)"""
    if name == "deep":
        g = deep_group()
        return ref.split_deep(g["site"], g["cond"], g["value"], g["min_frac_q16"])
    g = next(g for g in all_groups() if g["name"] == name)
    return ref.split(g["site"], g["cond"], g["value"], g["min_frac_q16"])
