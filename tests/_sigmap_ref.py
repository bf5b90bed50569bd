"""The sigmap contract (include/radian_hip.h, rd_sigmap) restated from its text: a plain-Python version (Python ints, lists, the strict
tie-breaks) and a NumPy int64 twin for the larger cases.  The sample, the cost, the k-mer and the window's scale are rd_eventalign's and
come from its restatement (_eventalign_ref); nothing here shares code with the library or with radian_amd.sigmap."""
import numpy as np

from _eventalign_ref import CAP, ZMAX, cost, kmer, quant, window_scale

OK, EMPTY, TOO_LONG, MAD_ZERO, NO_TARGET, TOO_LARGE = 0, 1, 2, 3, 4, 5
MAX_T = 1 << 14
MAX_BEST = 8


class Panel:
    """targets: lists of codes 0..3.  off[j]: the first global state of target j; per global state its (lvl, w, bias), whether it is the
    first of its target, and its target"""

    def __init__(self, targets, model):
        self.targets = [[int(c) for c in t] for t in targets]
        self.model = model
        self.off = [0]
        for t in self.targets:
            self.off.append(self.off[-1] + len(t))
        self.R = self.off[-1]
        self.tgt = [j for j, t in enumerate(self.targets) for _ in t]
        self.first = [b == 0 for t in self.targets for b in range(len(t))]
        self._st = None
        self._np = None

    def states(self):
        if self._st is None:
            m = self.model
            self._st = [(m.lvl[i], m.w[i], m.bias[i]) for t in self.targets for i in (kmer(t, b, m.k) for b in range(len(t)))]
        return self._st

    def arrays(self):
        """lvl, w, bias, first as NumPy arrays over the global states"""
        if self._np is None:
            m, idx = self.model, []
            for t in self.targets:
                c, L = np.asarray(t, dtype=np.int64), len(t)
                i = np.zeros(L, dtype=np.int64)
                for j in range(-(m.k // 2), m.k // 2 + 1):
                    i = i * 4 + (c[np.clip(np.arange(L) + j, 0, L - 1)] if L else c)
                idx.append(i)
            idx = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
            self._np = tuple(np.asarray(a, dtype=np.int64)[idx] for a in (m.lvl, m.w, m.bias)) + (np.asarray(self.first, dtype=bool),)
        return self._np


def _blank(status, n_best, m2=0, d4=0):
    return dict(status=status, m2=m2, d4=d4, tgt=[-1] * n_best, score=[-1] * n_best, end=[-1] * n_best, org=[-1] * n_best)


def _before(raw, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best):
    """the statuses in their order -> (a finished dict or None, m2, d4)"""
    T = q_hi - q_lo
    if T == 0:
        return _blank(EMPTY, n_best), 0, 0
    if T > MAX_T:
        return _blank(TOO_LONG, n_best), 0, 0
    if d4 == 0:
        m2, d4 = window_scale(raw[sc_lo:sc_hi]) if sc_hi > sc_lo else (0, 0)
        if d4 == 0:
            return _blank(MAD_ZERO, n_best, m2, d4), m2, d4
    if s_hi == s_lo:
        return _blank(NO_TARGET, n_best, m2, d4), m2, d4
    return None, m2, d4


def _result(panel, V, O, s_lo, s_hi, n_best, m2, d4, keep_final):
    """V, O: sequences over the states s_lo .. s_hi - 1 at the last row"""
    per = {}
    for i in range(s_hi - s_lo):          # ascending s: a later equal value does not replace the earlier
        j, v = panel.tgt[s_lo + i], int(V[i])
        if j not in per or v < per[j][0]:
            per[j] = (v, s_lo + i, int(O[i]))
    ranked = sorted((v, j, e, o) for j, (v, e, o) in per.items())[:n_best]
    out = _blank(OK, n_best, m2, d4)
    for r, (v, j, e, o) in enumerate(ranked):
        out["tgt"][r], out["score"][r], out["end"][r], out["org"][r] = j, v, e - panel.off[j], o - panel.off[j]
    if keep_final:
        out["final"], out["final_org"] = [int(v) for v in V], [int(v) for v in O]
    return out


def map_plain(raw, panel, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best, join=False, keep_final=False):
    """one query, Python ints and lists only.  join: the targets' first states are no heads (what the contract forbids: the cases use it to
    show that a path across two targets would have scored better)"""
    done, m2, d4 = _before(raw, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best)
    if done:
        return done
    st = panel.states()[s_lo:s_hi]
    head = [(not join and panel.first[s]) or s == s_lo for s in range(s_lo, s_hi)]
    zq = [quant(v, m2, d4) for v in raw[q_lo:q_hi]]
    n = s_hi - s_lo
    V = [cost(zq[0], st[i]) for i in range(n)]
    O = list(range(s_lo, s_hi))
    for t in range(1, len(zq)):
        W, P = [0] * n, [0] * n
        for i in range(n):
            adv = (not head[i]) and V[i - 1] < V[i]        # the advance only if STRICTLY smaller
            W[i] = cost(zq[t], st[i]) + (V[i - 1] if adv else V[i])
            P[i] = O[i - 1] if adv else O[i]
            assert abs(W[i]) < 1 << 25
        V, O = W, P
    return _result(panel, V, O, s_lo, s_hi, n_best, m2, d4, keep_final)


def map_numpy(raw, panel, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best, join=False, keep_final=False):
    """the int64 twin: a row at a time"""
    T = q_hi - q_lo
    x = np.asarray(raw, dtype=np.int64)
    if 0 < T <= MAX_T and d4 == 0 and sc_hi > sc_lo:       # the scale with NumPy's sort
        w = x[sc_lo:sc_hi]
        s = np.sort(w)
        m2 = int(s[(len(w) - 1) // 2] + s[len(w) // 2])
        d = np.sort(np.abs(2 * w - m2))
        d4 = int(d[(len(w) - 1) // 2] + d[len(w) // 2])
        if d4 == 0:
            return _blank(MAD_ZERO, n_best, m2, 0)
    done, m2, d4 = _before(raw, q_lo, q_hi, sc_lo, sc_hi, m2, d4, s_lo, s_hi, n_best)
    if done:
        return done
    lvl, w, bias, first = (a[s_lo:s_hi] for a in panel.arrays())
    head = np.zeros(s_hi - s_lo, dtype=bool) if join else first.copy()
    head[0] = True
    zq = np.clip(np.floor_divide(2 * 512 * (2 * x[q_lo:q_hi] - m2) + d4, 2 * d4), -ZMAX, ZMAX)

    def costs(z):
        d = z - lvl
        return np.minimum((d * d * w) >> 32, CAP) + bias       # d^2 < 2^30, w < 2^32: below 2^62

    V = costs(zq[0])
    O = np.arange(s_lo, s_hi, dtype=np.int64)
    av, ao = np.zeros_like(V), np.zeros_like(O)
    B = max(1, min(256, (1 << 22) // max(len(V), 1)))          # rows whose costs are worked out at once
    for t0 in range(1, T, B):
        C = costs(zq[t0:t0 + B, None])
        for i in range(len(C)):
            av[1:], ao[1:] = V[:-1], O[:-1]
            take = ~head & (av < V)
            V = C[i] + np.where(take, av, V)
            O = np.where(take, ao, O)
    assert np.abs(V).max() < 1 << 25
    return _result(panel, V, O, s_lo, s_hi, n_best, m2, d4, keep_final)


FIELDS = ("tgt", "score", "end", "org")


def assert_query_equal(res, q, want, what=""):
    """query q of a backend SigmapResult against a restatement dict, every field"""
    assert int(res.status[q]) == want["status"], (what, q, "status", int(res.status[q]), want["status"])
    assert (int(res.m2[q]), int(res.d4[q])) == (want["m2"], want["d4"]), (what, q, "scale", int(res.m2[q]), int(res.d4[q]), want["m2"], want["d4"])
    for f in FIELDS:
        got = [int(v) for v in getattr(res, f)[q]]
        assert got == want[f], (what, q, f, got, want[f])
