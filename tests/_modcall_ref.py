"""The modcall contract (include/radian_hip.h, rd_modcall) restated from its text: a plain-Python version (Python ints and lists) and a
NumPy int64 twin for the large cases.  Neither shares code with the library or with radian_amd.eventalign; the sample and cell rules are
_eventalign_ref's restatements of rd_eventalign's."""
import math

import numpy as np

from _eventalign_ref import CAP, INF, ZMAX, cost, kmer, quant

OK, NO_ANCHOR, NO_PATH, TOO_LONG, TOO_LARGE = 0, 1, 2, 3, 4
STATUS_NAMES = ("ok", "no-anchor", "no-path", "too-long", "too-large")
MAX_R = 1 << 15
MAX_FLANK, MAX_ALT, MAX_S = 27, 9, 63
# floor(32 ln(1 + e^(-d/32)) + 1/2), d = 0 .. 133 (test_modcall_cpu.py holds this and the library's literal to mpmath at 50 digits: no entry
# is nearer than 1e-3 to a rounding tie, so float64 decides every one)
LSE = [int(math.floor(32.0 * math.log1p(math.exp(-d / 32.0)) + 0.5)) for d in range(134)]
FIELDS = ("status", "n_rows", "n_states", "vit_ref", "vit_alt", "fwd_ref", "fwd_alt")


def softmin(a, b):
    return min(a, b) - LSE[min(abs(a - b), 133)]


def window(first, last, L, n, alt_first, n_alt, F):
    """-> (status, a0, S, r0, R)"""
    a0, a1 = max(0, alt_first - F), min(L - 1, alt_first + n_alt - 1 + F)
    S = a1 - a0 + 1
    r0, r1 = int(first[a0]), int(last[a1])
    if r0 == -1 or r1 == -1:
        return NO_ANCHOR, a0, S, 0, 0
    R = r1 - r0 + 1
    if R < S or r0 < 0 or r1 >= n:
        return NO_PATH, a0, S, 0, 0
    if R > MAX_R:
        return TOO_LONG, a0, S, 0, 0
    return OK, a0, S, r0, R


def _blank(status):
    return dict(status=status, n_rows=0, n_states=0, vit_ref=0, vit_alt=0, fwd_ref=0, fwd_alt=0)


def states(codes, model, a0, S, alt_first, alts):
    """-> the S (lvl, w, bias) of the window under ref and under alt"""
    ref = [(model.lvl[i], model.w[i], model.bias[i]) for i in (kmer(codes, a0 + s, model.k) for s in range(S))]
    alt = list(ref)
    for j, e in enumerate(alts):
        if 0 <= alt_first + j - a0 < S:
            alt[alt_first + j - a0] = tuple(int(v) for v in e)
    return ref, alt


def job_plain(raw, codes, m2, d4, first, last, model, alt_first, alts, F):
    """one job, Python ints and lists only; alts: [(lvl, w, bias)] -> dict of every output field"""
    L = len(codes)
    assert 1 <= len(alts) <= MAX_ALT and alt_first >= 0 and alt_first + len(alts) <= L and 0 <= F <= MAX_FLANK and d4 >= 1
    status, a0, S, r0, R = window(first, last, L, len(raw), alt_first, len(alts), F)
    if status != OK:
        return _blank(status)
    ref, alt = states(codes, model, a0, S, alt_first, alts)
    out = dict(status=OK, n_rows=R, n_states=S)
    for name, st in (("ref", ref), ("alt", alt)):
        z = quant(raw[r0], m2, d4)
        vit, fwd = [INF] * S, [INF] * S
        vit[0] = fwd[0] = cost(z, st[0])
        for t in range(1, R):
            z = quant(raw[r0 + t], m2, d4)
            c = [cost(z, s) for s in st]
            vit = [c[i] + min(vit[i], vit[i - 1] if i else INF) for i in range(S)]
            fwd = [c[i] + softmin(fwd[i], fwd[i - 1] if i else INF) for i in range(S)]
            assert all(-(1 << 31) <= v < (1 << 31) for v in vit + fwd)
        out["vit_" + name], out["fwd_" + name] = vit[S - 1], fwd[S - 1]
    return out


def job_numpy(raw, codes, m2, d4, first, last, model, alt_first, alts, F):
    """the int64 twin: a row at a time, the four values of every state in one array"""
    L = len(codes)
    status, a0, S, r0, R = window(first, last, L, len(raw), alt_first, len(alts), F)
    if status != OK:
        return _blank(status)
    ref, alt = states(codes, model, a0, S, alt_first, alts)
    lvl, w, bias = (np.array([[s[i] for s in ref], [s[i] for s in alt]], dtype=np.int64) for i in range(3))
    x = np.asarray(raw[r0:r0 + R], dtype=np.int64)
    zq = np.clip(np.floor_divide(2 * 512 * (2 * x - m2) + d4, 2 * d4), -ZMAX, ZMAX)
    lse = np.asarray(LSE, dtype=np.int64)

    def costs(z):
        d = z - lvl
        return np.minimum((d * d * w) >> 32, CAP) + bias

    V = np.full((4, S), INF, dtype=np.int64)    # vit_ref, vit_alt, fwd_ref, fwd_alt
    V[:, 0] = np.tile(costs(zq[0])[:, 0], 2)
    adv = np.full((4, S), INF, dtype=np.int64)
    for t in range(1, R):
        c = costs(zq[t])
        adv[:, 1:] = V[:, :-1]
        m = np.minimum(V, adv)
        m[2:] -= lse[np.minimum(np.abs(V[2:] - adv[2:]), 133)]
        V = m + np.tile(c, (2, 1))
    return dict(status=OK, n_rows=R, n_states=S, vit_ref=int(V[0, -1]), vit_alt=int(V[1, -1]), fwd_ref=int(V[2, -1]), fwd_alt=int(V[3, -1]))


def path_cost(raw, codes, m2, d4, first, last, model, a0, a1):
    """the summed cell cost of the path that the steps describe, over the rows first[a0] .. last[a1] and the bases a0 .. a1"""
    total = 0
    for b in range(a0, a1 + 1):
        i = kmer(codes, b, model.k)
        st = (model.lvl[i], model.w[i], model.bias[i])
        total += sum(cost(quant(raw[t], m2, d4), st) for t in range(int(first[b]), int(last[b]) + 1))
    return total


def assert_job_equal(res, j, want, what=""):
    """job j of a backend ModcallResult against a restatement dict, every field"""
    got = {f: int(getattr(res, f)[j]) for f in FIELDS}
    assert got == {f: want[f] for f in FIELDS}, (what, j, got, want)
