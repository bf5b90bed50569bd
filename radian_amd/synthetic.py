"""Seeded synthetic inputs of BASELINE.json's configs: Gaussian int16 reads; and the read-accuracy workload (alignment_pairs)."""
import numpy as np

from .preprocess import mad_normalise, get_windows


def synthetic_reads(n_reads, n_samples=4096, seed=0):
    """int16 = round(N(mu=500, sigma=80))."""
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(500.0, 80.0, size=(n_reads, n_samples))).astype(np.int16)


def reads_to_windows(reads, chunk_len=1024, step=512, clip=4):
    """MAD-normalise + window every read (basecall.py:78,83).  Returns
    (windows float32 [nW_total, chunk], valid_len int32 [nW_total], read_win_off int32 [n_reads+1], pads int32 [n_reads])."""
    wins, valid, offs, pads = [], [], [0], []
    for r in reads:
        norm = mad_normalise(r, clip)
        w, pad = get_windows(norm, chunk_len, step)
        v = np.full(w.shape[0], chunk_len, dtype=np.int32)
        v[-1] = chunk_len - pad
        wins.append(w.astype(np.float32))
        valid.append(v)
        offs.append(offs[-1] + w.shape[0])
        pads.append(pad)
    return (np.concatenate(wins, axis=0), np.concatenate(valid), np.asarray(offs, dtype=np.int32),
            np.asarray(pads, dtype=np.int32))


def peaky_probs(n_windows, chunk_len=1024, seed=0, gain=4.0, blank_bias=2.0):
    """SURVEY.md section 8d's decode-only benchmark rows: softmax(gain * N(0,1) + blank_bias on the blank class), float32
    [n_windows, chunk_len, 5] -- peaked rows with the blank favoured, as a trained CTC model emits them (a base every few rows), unlike
    the random-weight model's saturated rows (~5 bases per window) or the soft head's (~200)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_windows, chunk_len, 5), dtype=np.float32) * np.float32(gain)
    z[..., 4] += np.float32(blank_bias)
    z -= z.max(axis=-1, keepdims=True)
    np.exp(z, out=z)
    z /= z.sum(axis=-1, keepdims=True)
    return z


def alignment_pairs(n_pairs, seed=0, median_len=1500, sigma=0.35, p_sub=0.08, p_ins=0.04, p_del=0.04, max_junk=40, p_u=0.25, p_n=0.25,
                    min_len=1):
    """Seeded read-accuracy workload (radian_amd.align): (ids, refs, reads) as str.  Reference lengths are log-normal around
    median_len; each read is its reference with ~p_sub substitutions, p_ins insertions and p_del deletions per base, and 0..max_junk
    random bases of junk at each end (so the soft clip engages).  A fraction p_u of the reads is written with U for T (the basecaller's
    alphabet), a fraction p_n of the references carries a few N."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = np.maximum(np.round(median_len * np.exp(sigma * rng.standard_normal(n_pairs))).astype(np.int64), min_len)
    ids, refs, reads = [], [], []
    for k in range(n_pairs):
        n = int(lens[k])
        ref = alpha[rng.integers(0, 4, n)]
        if rng.random() < p_n:
            ref = ref.copy()
            ref[rng.integers(0, n, max(1, n // 200))] = ord("N")
        # per reference base: deleted, substituted or kept, then maybe one inserted base after it
        ev = rng.random(n)
        sub = alpha[(np.searchsorted(alpha, ref) % 4 + rng.integers(1, 4, n)) % 4]   # a different base (any base at an N)
        cols = np.zeros((n, 2), dtype=np.uint8)
        cols[:, 0] = np.where(ev < p_del, 0, np.where(ev < p_del + p_sub, sub, ref))
        cols[:, 1] = np.where(rng.random(n) < p_ins, alpha[rng.integers(0, 4, n)], 0)
        out = cols.reshape(-1)
        out = out[out != 0]
        nn = out == ord("N")   # a kept N: the basecaller emits a base
        out[nn] = alpha[rng.integers(0, 4, int(nn.sum()))]
        head = alpha[rng.integers(0, 4, int(rng.integers(0, max_junk + 1)))]
        tail = alpha[rng.integers(0, 4, int(rng.integers(0, max_junk + 1)))]
        read = bytes(head) + bytes(out) + bytes(tail)
        if rng.random() < p_u:
            read = read.replace(b"T", b"U")
        ids.append(f"read_{seed}_{k}")
        refs.append(ref.tobytes().decode("ascii"))
        reads.append(read.decode("ascii"))
    return ids, refs, reads


def write_alignment_inputs(path_fasta, path_tsv, ids, refs, reads, line_width=60):
    """the FASTA of the reads (wrapped lines) and the reference TSV (header, then id <tab> text <tab> sequence) radian_amd.align reads"""
    with open(path_fasta, "w") as f:
        for rid, s in zip(ids, reads):
            f.write(f">{rid} synthetic\n")
            for o in range(0, len(s), line_width):
                f.write(s[o: o + line_width] + "\n")
    with open(path_tsv, "w") as f:
        f.write("read_id\ttranscript\tsequence\n")
        for rid, s in zip(ids, refs):
            f.write(f"{rid}\tsynthetic\t{s}\n")


def tail_read(rng, leader=400, adapter=600, tail=1500, body=4000, leader_level=800.0, adapter_level=450.0, tail_level=620.0,
              body_levels=(300.0, 700.0), noise=45.0, tail_noise=2.0):
    """One synthetic direct-RNA read with a poly(A) tail, in the order the pore sees it (3' first): a leader and an adapter at their own
    levels with moderate noise, a TAIL of constant level with small noise, then a body of piecewise-constant levels (uniform over
    body_levels, dwell 8..60 samples, Gaussian noise: the jumps are large against it, and the noise is large against what counts as flat).
    rng: a numpy Generator.  -> (int16 samples, (tail_start, tail_end)): the tail is samples [tail_start, tail_end)."""
    parts = [leader_level + noise * rng.standard_normal(leader), adapter_level + noise * rng.standard_normal(adapter),
             tail_level + tail_noise * rng.standard_normal(tail)]
    levels = np.empty(body)
    i = 0
    while i < body:
        d = int(rng.integers(8, 61))
        levels[i:i + d] = rng.uniform(*body_levels)
        i += d
    parts.append(levels + noise * rng.standard_normal(body))
    x = np.clip(np.round(np.concatenate(parts)), -32768, 32767).astype(np.int16)
    return x, (leader + adapter, leader + adapter + tail)


def site_events(rng, n_sites=300, median_depth=40.0, sigma=0.8, min_depth=1, shifted=(), level_shift=0.5, dwell_stretch=1.6, level_sd=0.3,
                mean_dwell=12.0):
    """Two samples' events over n_sites transcript positions, as `resquiggle` would tabulate them.  Every site has a level of its own (uniform
    over -1.5 .. 1.5 z) and, per sample, a depth drawn from a log-normal (median median_depth, shape sigma, at least min_depth); an
    event's level is the site's plus Gaussian noise of level_sd, its dwell 1 + a geometric number of samples (mean mean_dwell).  At the
    sites in `shifted`, sample 1's levels are moved by level_shift and its mean dwell is stretched by dwell_stretch.  rng: a numpy Generator.
    -> {site int64, cond uint8, level float64 (z units), dwell int64} arrays, one entry per event (sample 0's events first, each sample
    site by site), and depth int64 [n_sites, 2]."""
    shifted = set(int(s) for s in shifted)
    base = rng.uniform(-1.5, 1.5, n_sites)
    depth = np.maximum(np.rint(median_depth * np.exp(sigma * rng.standard_normal((n_sites, 2)))).astype(np.int64), int(min_depth))
    site, cond, level, dwell = [], [], [], []
    for c in (0, 1):
        for s in range(n_sites):
            n = int(depth[s, c])
            moved = c == 1 and s in shifted
            site.append(np.full(n, s, dtype=np.int64))
            cond.append(np.full(n, c, dtype=np.uint8))
            level.append(base[s] + (level_shift if moved else 0.0) + level_sd * rng.standard_normal(n))
            dwell.append(rng.geometric(1.0 / (mean_dwell * (dwell_stretch if moved else 1.0)), n).astype(np.int64))
    return {"site": np.concatenate(site), "cond": np.concatenate(cond), "level": np.concatenate(level), "dwell": np.concatenate(dwell),
            "depth": depth}
