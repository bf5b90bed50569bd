"""CPU restatement (numpy, fp64) of the model-evaluation contract of rd_ctc_* (radian_amd/csrc/ctc.hip):
Keras ctc_batch_cost's per-window loss, the feasibility rule, the greedy decode and its edit distance.  Test infrastructure."""
import numpy as np

EPS = 1e-7      # Keras backend epsilon()
BLANK = 4


def log_probs(y):
    """log p[t][k], p = (y + eps) / sum_j (y + eps): Keras log(y + epsilon), then TF's log-softmax -- in fp64"""
    q = np.asarray(y, dtype=np.float64) + EPS
    return np.log(q) - np.log(q.sum(axis=-1, keepdims=True))


def infeasible(label, n):
    label = list(label)
    return len(label) + sum(1 for a, b in zip(label, label[1:]) if a == b) > n


def ctc_loss(y, n, label):
    """-log sum over paths of the first n rows that collapse to label of prod p; +inf when there is none"""
    lp = log_probs(np.asarray(y)[:n])
    label = [int(c) for c in label]
    ext = [BLANK]
    for c in label:
        ext += [c, BLANK]
    S = len(ext)
    ext = np.array(ext)
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = ext[s] != ext[s - 2]
    a = np.full(S, -np.inf)
    a[0] = lp[0, BLANK]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, n):
        p1 = np.concatenate(([-np.inf], a[:-1]))
        p2 = np.concatenate(([-np.inf, -np.inf], a[:-2]))[:S]
        p2 = np.where(skip, p2, -np.inf)
        m = np.maximum(np.maximum(a, p1), p2)
        fin = np.isfinite(m)
        mm = np.where(fin, m, 0.0)
        with np.errstate(invalid="ignore"):
            s = np.exp(a - mm) + np.exp(p1 - mm) + np.exp(p2 - mm)
        a = np.where(fin, mm + np.log(np.where(fin, s, 1.0)), -np.inf) + lp[t, ext]
    tail = a[-2:] if S > 1 else a[-1:]
    m = tail.max()
    if m == -np.inf:
        return np.inf
    return -(m + np.log(np.exp(tail - m).sum()))


def greedy(y, n):
    """argmax of each of the first n rows (lowest class on a tie: np.argmax), repeats collapsed, blanks dropped"""
    best = np.argmax(np.asarray(y)[:n], axis=1)
    out, prev = [], None
    for c in best:
        if c != BLANK and c != prev:
            out.append(int(c))
        prev = c
    return out


def levenshtein(a, b):
    a, b = list(a), list(b)
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, z in enumerate(b, 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (x != z))
            prev, d[j] = d[j], cur
    return d[len(b)]


def evaluate(y, n, label):
    """(loss, status, greedy_len, edit_distance) of one window, as rd_ctc_probs reports them"""
    g = greedy(y, n)
    return ctc_loss(y, n, label), int(infeasible(label, n)), len(g), levenshtein(g, label)
