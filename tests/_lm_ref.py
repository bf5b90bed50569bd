"""CPU restatement of the RNA-model builder's contract (radian_amd.lm_build; include/radian_hip.h), in plain Python / numpy, written from
the contract and not from the kernels.  TESTS ONLY.

  read_fasta   the scanner's rules, byte by byte
  counts       C_k: one per window of k + 1 labels over ACGT, in decode order (the record reversed) unless as_written
  marginals    C_j[s][b] = sum over the (k - j)-label prefixes p of C_k[p s][b]
  table        row c from the largest order j <= k whose row of c's last j labels has a positive sum: (C + a) / (s + 4 a) in float64
  score        held-out windows against a table
"""
import gzip
import math

import numpy as np

_CODE = {c: i for i, c in enumerate("ACGT")}
_CODE.update({c.lower(): i for c, i in list(_CODE.items())})
_CODE["U"] = _CODE["u"] = 3


def read_fasta(data, field=None, value=None):
    """bytes (gzip or plain) -> (codes uint8, offsets int64, info).  Errors: ValueError('record R, line L: ...')"""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    codes, offsets = [], []
    rec, keep = 0, False
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln, line in enumerate(lines, 1):
        if line[:1] == b">":
            rec += 1
            head = line[1:]
            if head.endswith(b"\r"):
                head = head[:-1]
            if field is None:
                keep = True
            else:
                parts = head.split(b"|")
                keep = field < len(parts) and parts[field] == value.encode()
            if keep:
                offsets.append(len(codes))
            continue
        for byte in line:
            ch = chr(byte)
            if ch in " \t\r\v\f":
                continue
            if not (("A" <= ch <= "Z") or ("a" <= ch <= "z") or ch in "*-"):
                raise ValueError(f"record {rec}, line {ln}: byte 0x{byte:02x}")
            if rec == 0:
                raise ValueError(f"record 0, line {ln}: sequence before the first header")
            if keep:
                codes.append(_CODE.get(ch, 255))
    kept = len(offsets)
    offsets.append(len(codes))
    return np.array(codes, dtype=np.uint8), np.array(offsets, dtype=np.int64), {"records": rec, "kept": kept, "bases": len(codes)}


def window_codes(codes, offsets, k, as_written=False):
    """(context << 2 | next) of every counted window, vectorised: int64 array"""
    out = []
    for r in range(len(offsets) - 1):
        d = np.asarray(codes[offsets[r]:offsets[r + 1]], dtype=np.int64)
        if not as_written:
            d = d[::-1]
        n = len(d)
        if n < k + 1:
            continue
        # window ending at j (k <= j < n): labels d[j-k .. j], oldest first
        code = np.zeros(n - k, dtype=np.int64)
        ok = np.ones(n - k, dtype=bool)
        for q in range(k + 1):
            lab = d[q: n - k + q]
            ok &= lab < 4
            code = code * 4 + (lab & 3)
        out.append(code[ok])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def counts(codes, offsets, k, as_written=False):
    """C_k as int64 [4^k, 4]"""
    wc = window_codes(codes, offsets, k, as_written)
    return np.bincount(wc, minlength=4 ** (k + 1)).astype(np.int64).reshape(4 ** k, 4)


def counts_loop(codes, offsets, k, as_written=False):
    """the same, as the contract's loop over windows (small inputs)"""
    C = np.zeros((4 ** k, 4), dtype=np.int64)
    for r in range(len(offsets) - 1):
        t = [int(x) for x in codes[offsets[r]:offsets[r + 1]]]
        d = t if as_written else t[::-1]
        for j in range(k, len(d)):
            w = d[j - k: j + 1]
            if all(x < 4 for x in w):
                ctx = 0
                for x in w[:-1]:
                    ctx = ctx * 4 + x
                C[ctx, w[-1]] += 1
    return C


def marginals(Ck, k):
    """[C_0, ..., C_k]: C_j int64 [4^j, 4]"""
    out = [None] * (k + 1)
    out[k] = Ck
    for j in range(k - 1, -1, -1):
        out[j] = Ck.reshape(4 ** (k - j), 4 ** j, 4).sum(0)
    return out


def table(Ck, k, unseen="backoff", alpha=0.0):
    """-> (table float64 [4^k, 4] with NaN rows where absent, order int [4^k]: the order each row was filled from, -1 uniform / absent)"""
    C = marginals(Ck, k)
    n = 4 ** k
    tab = np.full((n, 4), np.nan, dtype=np.float64)
    order = np.full(n, -1, dtype=np.int64)
    todo = np.ones(n, dtype=bool)
    ctx = np.arange(n, dtype=np.int64)
    for j in range(k, -1, -1):
        rows = C[j][ctx % (4 ** j)]                         # the row of each context's last j labels
        s = rows.sum(1)
        hit = todo & (s > 0)
        num = rows[hit].astype(np.float64) + np.float64(alpha)
        den = s[hit].astype(np.float64) + np.float64(4.0 * alpha)
        tab[hit] = num / den[:, None]
        order[hit] = j
        todo &= ~hit
        if unseen != "backoff":
            break
    if unseen == "uniform":
        tab[todo] = 0.25
    return tab, order


def entropy(tab):
    """decode.py:73-76,85-90: -sum p ln p over p > 0, Python floats left to right; inf for absent rows"""
    out = np.empty(len(tab), dtype=np.float64)
    for c, row in enumerate(tab):
        if row[0] != row[0]:
            out[c] = math.inf
            continue
        terms = [float(p) * math.log(float(p)) for p in row if p > 0]
        out[c] = -sum(terms[1:], terms[0]) if terms else 0.0
    return out


def score(tab, k, codes, offsets, r_threshold, as_written=False):
    wc = window_codes(codes, offsets, k, as_written)
    ctx, nxt = wc >> 2, wc & 3
    ent = entropy(tab)
    absent = np.isnan(tab[ctx, 0]) if len(wc) else np.zeros(0, dtype=bool)
    p = tab[ctx, nxt] if len(wc) else np.zeros(0)
    pos = ~absent & (p > 0)
    terms = [-math.log(float(x)) for x in p[pos]]
    total = math.fsum(terms)
    return {"windows": int(len(wc)), "scored": int(pos.sum()), "zero": int((~absent & ~pos).sum()), "absent": int(absent.sum()),
            "gate_windows": int((ent[ctx] < r_threshold).sum()) if len(wc) else 0, "nll_sum": total,
            "mean_nll": total / len(terms) if terms else float("nan")}


def markov_transcripts(seed, n_records, length, order=3, conc=0.3, floor=0.02):
    """transcripts from a seeded order-`order` Markov chain -> list of str over ACGT.  The chain's rows are Dirichlet(conc) draws with the
    entries below `floor` set to zero (renormalised), so that some short contexts never occur and the back-off reaches low orders.  All
    records advance together, one vectorised step per position."""
    rng = np.random.default_rng(seed)
    rows = rng.dirichlet([conc] * 4, size=4 ** order)
    rows[rows < floor] = 0.0
    rows /= rows.sum(1, keepdims=True)
    cum = np.cumsum(rows, axis=1)
    cum[:, 3] = 2.0
    lab = np.empty((n_records, length), dtype=np.uint8)
    state = rng.integers(0, 4 ** order, size=n_records)
    for i in range(length):
        u = rng.random(n_records)
        b = (u[:, None] >= cum[state]).sum(1)
        lab[:, i] = b
        state = (state * 4 + b) % (4 ** order)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [alphabet[r].tobytes().decode() for r in lab]


def encode(seqs):
    """list of str -> (codes, offsets) by the alphabet rule (no file)"""
    codes = np.array([_CODE.get(ch, 255) for s in seqs for ch in s], dtype=np.uint8)
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return codes, off
