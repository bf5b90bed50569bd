"""TEST INFRASTRUCTURE: seeded inputs of the two-sample site comparison.  Every group is a dict: name, site (uint32),
cond (uint8), value (int16), n_sites, and cond: {site: predicate over that site's entry of the restatement (tests/_sitecmp_ref.py)} -- the
group's defining condition, asserted without a GPU by tests/test_sitecmp_cpu.py.  Sizes follow the kernels' constants: 64 lanes and the
chunk of C = 256 elements one wave of the site kernel takes."""
import functools

import numpy as np

import _sitecmp_ref as ref

LANES, C = 64, 256
DEPTHS = (1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5)


def _group(name, per_site, n_sites, cond, rng=None):
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
    return dict(name=name, site=site, cond=cnd, value=value, n_sites=n_sites, cond_of=cond)


def _draw(rng, n, spread=30, centre=0):
    """n values with many ties: a rounded Gaussian"""
    return np.clip(np.rint(centre + spread * rng.standard_normal(n)), -32768, 32767).astype(np.int64).tolist()


def depths_group():
    """total depths 1 .. 3C + 5 split at random between the samples (sites 0 ..), and the same depths as n0 against a short sample 1"""
    rng = np.random.default_rng(2001)
    per, cond = {}, {}
    for i, d in enumerate(DEPTHS):
        n0 = int(rng.integers(0, d + 1)) if d > 1 else 1
        n0 = min(max(n0, 1), d - 1) if d > 1 else 1
        per[i] = (_draw(rng, n0), _draw(rng, d - n0, centre=8))
        cond[i] = (lambda d: lambda e: sum(e["n"]) == d)(d)
        per[100 + i] = (_draw(rng, d), _draw(rng, int(rng.integers(1, 70)), centre=-5))
        cond[100 + i] = (lambda d: lambda e: e["n"][0] == d and e["status"] == ref.OK)(d)
    return _group("depths", per, 200, cond, rng)


def one_sided_group():
    rng = np.random.default_rng(2002)
    per = {3: ([], _draw(rng, 70)), 4: (_draw(rng, 70), []), 9: (_draw(rng, 5), _draw(rng, 5))}
    zero = lambda e: (e["u2"], e["ks_num"], e["ks_x"], e["tie"]) == (0, 0, 0, 0)
    cond = {3: lambda e: e["status"] == ref.ONE_SIDED and e["n"] == (0, 70) and zero(e) and (e["sum"][0], e["vmin"][0], e["med2"][0]) == (0, 0, 0),
            4: lambda e: e["status"] == ref.ONE_SIDED and e["n"] == (70, 0) and zero(e) and (e["sum"][1], e["vmax"][1], e["med2"][1]) == (0, 0, 0),
            9: lambda e: e["status"] == ref.OK}
    return _group("one_sided", per, 10, cond)


def one_vs_chunk_group():
    rng = np.random.default_rng(2003)
    per = {0: (_draw(rng, 1), _draw(rng, C + 1)), 1: (_draw(rng, C + 1), _draw(rng, 1))}
    return _group("one_vs_chunk", per, 2, {0: lambda e: e["n"] == (1, C + 1), 1: lambda e: e["n"] == (C + 1, 1)}, rng)


def all_equal_group():
    """every value of a site equal: tie = N^3 - N (its maximum), ks_num 0, ks_x that value"""
    per = {0: ([7] * 40, [7] * 90), 1: ([-300] * (C + 3), [-300] * 2)}
    cond = {0: lambda e: (e["tie"], e["ks_num"], e["ks_x"], e["u2"]) == (130 ** 3 - 130, 0, 7, 40 * 90),
            1: lambda e: (e["tie"], e["ks_num"], e["ks_x"]) == ((C + 5) ** 3 - (C + 5), 0, -300)}
    return _group("all_equal", per, 2, cond)


def disjoint_group():
    """disjoint ranges: ks_num = n0 n1 and u2 is 0 (a below b) or 2 n0 n1 (a above b)"""
    rng = np.random.default_rng(2005)
    lo, hi = _draw(rng, 90, 10, -500), _draw(rng, 70, 10, 500)
    per = {0: (lo, hi), 1: (hi, lo)}
    cond = {0: lambda e: (e["ks_num"], e["u2"]) == (90 * 70, 0) and e["ks_x"] == max(lo),
            1: lambda e: (e["ks_num"], e["u2"]) == (90 * 70, 2 * 90 * 70) and e["ks_x"] == max(lo)}
    return _group("disjoint", per, 2, cond, rng)


def ks_tie_group():
    """the maximum attained at two values: ks_x is the smaller.  a = 1 3, b = 2 4: |#{a <= x} 2 - #{b <= x} 2| = 2 0 2 0 at x = 1 2 3 4;
    and a site where the maximum is attained at a value of sample 1 only, before a value of sample 0"""
    per = {0: ([1, 3], [2, 4]), 1: ([5, 5, 9, 9], [2, 2, 7, 7])}
    # site 1: x = 2: |0 - 2 * 4| = 8; x = 5: |2 * 4 - 2 * 4| = 0; x = 7: |8 - 16| = 8; x = 9: 0 -> maximum 8 at x = 2 and x = 7
    cond = {0: lambda e: (e["ks_num"], e["ks_x"]) == (2, 1), 1: lambda e: (e["ks_num"], e["ks_x"]) == (8, 2)}
    return _group("ks_tie", per, 2, cond)


def extremes_group():
    per = {0: ([-32768, 32767, -32768, 0], [32767, -32768, 32767]), 1: ([-32768] * 3, [32767] * 5), 2: ([32767] * 3, [-32768] * 5)}
    cond = {0: lambda e: e["vmin"] == (-32768, -32768) and e["vmax"] == (32767, 32767) and e["sumsq"][0] == 2 * 32768 ** 2 + 32767 ** 2,
            1: lambda e: (e["ks_num"], e["ks_x"], e["u2"]) == (15, -32768, 0),
            2: lambda e: (e["ks_num"], e["ks_x"], e["u2"]) == (15, -32768, 30)}
    return _group("extremes", per, 3, cond)


def wide_sites_group():
    """site ids 0 and 2^32 - 2 with n_sites = 2^32 - 1: the key takes all of its 49 bits"""
    rng = np.random.default_rng(2008)
    top = (1 << 32) - 2
    per = {top: (_draw(rng, 66), _draw(rng, 65)), 0: (_draw(rng, 10), _draw(rng, 12)), 1 << 31: (_draw(rng, 3), _draw(rng, 3))}
    cond = {top: lambda e: e["out_site"] == top and e["status"] == ref.OK, 0: lambda e: e["out_site"] == 0}
    return _group("wide_sites", per, (1 << 32) - 1, cond, rng)


def interleaved_group():
    """no site is contiguous in the input: event i belongs to site i mod 7"""
    rng = np.random.default_rng(2009)
    n = 7 * 90
    site = (np.arange(n) % 7).astype(np.uint32) * 11
    g = dict(name="interleaved", site=site, cond=rng.integers(0, 2, n).astype(np.uint8), value=np.array(_draw(rng, n), dtype=np.int16), n_sites=100)
    g["cond_of"] = {0: lambda e: sum(e["n"]) == 90}
    return g


def all_groups():
    return [depths_group(), one_sided_group(), one_vs_chunk_group(), all_equal_group(), disjoint_group(), ks_tie_group(), extremes_group(),
            wide_sites_group(), interleaved_group()]


@functools.lru_cache(maxsize=None)
def deep_group():
    """one site of exactly 2^20 events (OK: the deepest site that gets rank statistics) and one of 2^20 + 1 (DEEP), interleaved"""
    rng = np.random.default_rng(2010)
    n_ok, n_deep = 1 << 20, (1 << 20) + 1
    site = np.concatenate([np.full(n_ok, 5, np.uint32), np.full(n_deep, 2, np.uint32)])
    cond = rng.integers(0, 2, n_ok + n_deep).astype(np.uint8)
    value = np.clip(np.rint(400 * rng.standard_normal(n_ok + n_deep) + 60 * cond), -32768, 32767).astype(np.int16)
    p = rng.permutation(n_ok + n_deep)
    return dict(name="deep", site=site[p], cond=cond[p], value=value[p], n_sites=8,
                cond_of={5: lambda e: sum(e["n"]) == 1 << 20 and e["status"] == ref.OK and e["tie"] > 0 and e["ks_num"] > 0,
                         2: lambda e: sum(e["n"]) == (1 << 20) + 1 and e["status"] == ref.DEEP and (e["u2"], e["ks_num"], e["ks_x"], e["tie"]) == (0, 0, 0, 0)
                         and e["sumsq"][0] > 0 and e["med2"] != (0, 0)})


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's entries of a group, computed once and shared by the tests (never modified)"""
    if name == "deep":
        g = deep_group()
        return ref.compare_deep(g["site"], g["cond"], g["value"])
    g = next(g for g in all_groups() if g["name"] == name)
    return ref.compare(g["site"], g["cond"], g["value"])
