"""TEST INFRASTRUCTURE: the signal-simulation contract (include/radian_hip.h, rd_sim_signal) restated in Python / numpy integers, written
from the contract's text.  Philox runs vectorised over the counters in uint64 arithmetic masked to 32 bits; everything after it is int64."""
import numpy as np

OK, EMPTY, TOO_LARGE = 0, 1, 2
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (arrays or scalars) under one key -> four uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def philox_scalar(counter, key):
    """plain Python integers, for the known answers"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def kmers(codes, k):
    """the k-mer index of every base: centred, first base most significant, positions outside the read take the nearest end base"""
    codes = np.asarray(codes, dtype=np.int64)
    L, h = len(codes), k // 2
    idx = np.zeros(L, dtype=np.int64)
    for j in range(-h, h + 1):
        idx = idx * 4 + codes[np.clip(np.arange(L) + j, 0, L - 1)]
    return idx


def noise_z(n, key):
    """z of samples 0 .. n - 1"""
    w = philox(np.arange(n, dtype=np.uint64), 1, 0, 0, key[0], key[1])
    Z = np.zeros(n, dtype=np.int64)
    for x in w:
        x = x.astype(np.int64)
        Z += (x & 1023) + ((x >> 10) & 1023) + ((x >> 20) & 1023)
    return Z - 6138


def dwells(codes, model, key, dwell_scale=None):
    L = len(codes)
    if L == 0:
        return np.zeros(0, dtype=np.int64)
    w0 = philox(np.arange(L, dtype=np.uint64), 0, 0, 0, key[0], key[1])[0].astype(np.int64)
    scale = np.full(L, 256, dtype=np.int64) if dwell_scale is None else np.asarray(dwell_scale, dtype=np.int64)
    m = (np.asarray(model["dwell_q8"], dtype=np.int64)[kmers(codes, model["k"])] * scale) >> 8
    t = np.asarray(model["dwell_cdf"], dtype=np.int64)[w0 >> 22]
    return np.clip((m * t + (1 << 23)) >> 24, 1, 32767)


def simulate(codes, model, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, level_shift=None, dwell_scale=None):
    """one read -> (n_samples, base_first int64 [L], raw int64 [n_samples], status)"""
    L = len(codes)
    d = dwells(codes, model, key, dwell_scale)
    base_first = lead + np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64) if L else np.zeros(0, dtype=np.int64)
    n = int(lead + d.sum())
    if n == 0:
        return 0, base_first, np.zeros(0, dtype=np.int64), EMPTY
    s = np.arange(n, dtype=np.int64)
    base = np.searchsorted(base_first, s, side="right") - 1          # -1: the lead
    level = np.full(n, lead_level_q10, dtype=np.int64)
    sd = np.full(n, lead_sd_q10, dtype=np.int64)
    if L:
        km = kmers(codes, model["k"])
        lv = np.asarray(model["level_q10"], dtype=np.int64)[km] + (0 if level_shift is None else np.asarray(level_shift, dtype=np.int64))
        sv = np.asarray(model["sd_q10"], dtype=np.int64)[km]
        on = base >= 0
        level[on], sd[on] = lv[base[on]], sv[base[on]]
    v = level + ((sd * noise_z(n, key)) >> 10)                       # >> on int64 is floor
    raw = np.clip(median + ((v * scale_q10 + (1 << 19)) >> 20), -32768, 32767)
    return n, base_first, raw, OK
