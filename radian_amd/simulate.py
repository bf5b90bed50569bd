"""Simulate direct-RNA reads from transcripts: raw signal whose sequence, base boundaries, tail and modified sites are known.

    python -m radian_amd.simulate transcripts.fa[.gz] -o out_dir --reads N [--seed 0]
           [--kmer-table T.tsv [--fill-missing] | --model-seed S --kmer 5] [--protein-coding | --field N --value S]
           [--length-median 1200 --length-sigma 0.5 --min-length 200] [--tail-median 80 --tail-sigma 0.5 | --tail N] [--adapter SEQ]
           [--lead-samples 400 --lead-level 2.0 --lead-sd 0.3] [--dwell-min-frac 0.2] [--median 600 --mad 60] [--noise-scale 1.0]
           [--modify sites.tsv [--mods-out mods.tsv]] [--reads-per-file 4000]
           [--shards DIR --chunk-len 1024 --step-size 128 --outlier-clip 4 --val-fraction 0.05 --windows-per-shard 50000 --max-label-len 255]
           [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour.  The host draws, with numpy.random.Generator(PCG64(seed)) and read by read, a transcript, the length of a fragment
anchored at its 3' end (log-normal, at least --min-length, at most the transcript), a tail length (log-normal, or --tail) and a 64-bit
key; a fragment with a letter outside ACGTU is drawn again.  The read is composed in the order the pore sees it: the adapter (--adapter,
written in that order), the tail as A, then the fragment reversed (U = T).  The GPU turns it into samples (rd_sim_signal, DESIGN.md section
21; the contract is in include/radian_hip.h): every base dwells for its k-mer's mean dwell times an exponential quantile (with a floor of
--dwell-min-frac), every sample is the k-mer's level plus noise of its sd, mapped to DAQ units by --median and --mad
(z = (x - median) / (1.4826 mad), as mad_normalise reads it back).  --lead-samples of open-pore-like signal come first.

The pore model is a `resquiggle --kmer-table` file (k-mers written 5'->3'; a k-mer the table lacks is an error naming it, or with
--fill-missing takes the table's count-weighted means), or a STAND-IN derived from --model-seed: levels uniform over +-1.5 z by a hash of
the k-mer, sd 0.3 z, mean dwell 30 samples, the all-A k-mer at sd 0.04 z.  The stand-in is no pore.

--modify takes rows `ref_name pos level_shift dwell_scale fraction` (pos 0-based on the transcript, level_shift in z, no header): a read
that covers the site is modified there with probability `fraction` (drawn on the host): that base's level moves and its dwell stretches.
--mods-out writes that draw: rows `read_id ref_name pos modified` (0 / 1, with a header), one for every read and --modify site the read
covers, in read order; no other output changes with it.

Outputs under out_dir: sim_{k:04d}.fast5 (--reads-per-file each); truth.tsv (read_id ref_name ref_start ref_end n_samples lead tail_nt
tail_start tail_end -- the tail is the samples of the bases whose whole k-mer is A, -1 -1 without one); read_ref.tsv (what `align`,
`label_build` and `resquiggle` read); truth.paf (the twelve columns `compare` reads); truth_moves.tsv (`fastq --moves`' format: the
fragment's bases in written order).  --shards writes {train,val}/shard-NNNNN.tfrecords as label_build does, labelled by the truth: a
window's label is the fragment bases whose first sample lies in it; a window is dropped and counted when that is empty, longer than
--max-label-len or not CTC-feasible, or when the window starts before the fragment's first sample (lead, adapter or tail in it).
Every file is bit-identical across --batch-reads, --budget-bytes and runs.  One GPU; there is no CPU path."""
import argparse
import math
import os
import sys

import numpy as np

from . import fast5
from .backend import Backend, SimModel
from .label_build import ShardWriter, ctc_rows, is_val
from .map import TSV_HEADER, Transcripts
from .preprocess import get_windows
from .tfrecord import WINDOW

DEFAULT_ADAPTER = "GGCTTCTTCTTGCTCTTAGGTAGTAGGTTC"      # a fixed 30-mer without a run of A; it stands for an adapter, it is none
KMER_COLUMNS = ("kmer", "n_events", "level_mean", "level_sd", "dwell_mean")
DROP_REASONS = ("edge", "empty", "too-long", "infeasible")
_CODE = {c: i for i, letters in enumerate(("Aa", "Cc", "Gg", "TtUu")) for c in letters}
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def encode(seq, what):
    try:
        return np.array([_CODE[c] for c in seq], dtype=np.uint8)
    except KeyError as e:
        raise SystemExit(f"simulate: {what} holds {e.args[0]!r}, not one of ACGTU")


# ------------------------------------------------------------------------------------------------ the pore model
def _philox_w0(i, stream, key0, key1):
    """word 0 of Philox4x32-10 of counters (i, stream, 0, 0), i a uint64 array below 2^32"""
    m = np.uint64(0xFFFFFFFF)
    c = [i.astype(np.uint64), np.full(i.shape, stream, np.uint64), np.zeros(i.shape, np.uint64), np.zeros(i.shape, np.uint64)]
    k0, k1 = key0 & 0xFFFFFFFF, key1 & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c[0]


def dwell_cdf(min_frac):
    """1024 quantiles of the dwell in Q16 multiples of its mean: a floor of min_frac plus an exponential of mean 1 - min_frac"""
    q = (np.arange(1024) + 0.5) / 1024
    return np.rint(65536 * (min_frac + (1 - min_frac) * -np.log(1 - q))).astype(np.uint32)


def standin_tables(k, seed):
    """the stand-in: (level_q10, sd_q10, dwell_q8) int32 [4^k] from a seed.  No pore."""
    n = 4 ** k
    w0 = _philox_w0(np.arange(n, dtype=np.uint64), 2, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    level = (-1536 + ((w0 * np.uint64(3073)) >> np.uint64(32)).astype(np.int64)).astype(np.int32)        # uniform over -1536 .. 1536
    sd = np.full(n, 307, dtype=np.int32)
    sd[0] = 41
    return level, sd, np.full(n, 30 * 256, dtype=np.int32)


def read_kmer_table(path, fill_missing=False):
    """a `resquiggle --kmer-table` file -> (k, level_q10, sd_q10, dwell_q8), indexed by the k-mer in PORE order: the file's k-mers are
    written 5'->3' and the pore sees them reversed"""
    rows = []
    with open(path, "r") as f:
        for i, line in enumerate(f):
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if i == 0 or not line.strip():
                continue
            if len(cols) != len(KMER_COLUMNS):
                raise SystemExit(f"simulate: {path}, line {i + 1}: {len(cols)} columns, not {', '.join(KMER_COLUMNS)}")
            try:
                rows.append((cols[0], int(cols[1]), float(cols[2]), float(cols[3]), float(cols[4])))
            except ValueError:
                raise SystemExit(f"simulate: {path}, line {i + 1}: a number does not parse")
    if not rows:
        raise SystemExit(f"simulate: {path} holds no k-mer")
    k = len(rows[0][0])
    if k % 2 == 0 or k > 9:
        raise SystemExit(f"simulate: {path}: k = {k}; the simulator takes odd k up to 9")
    n = 4 ** k
    level, sd, dwell, seen = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for kmer, cnt, lm, ls, dm in rows:
        if len(kmer) != k:
            raise SystemExit(f"simulate: {path}: k-mers of {k} and of {len(kmer)} letters")
        idx = 0
        for c in encode(kmer, f"{path}: k-mer {kmer}")[::-1]:
            idx = idx * 4 + int(c)
        level[idx], sd[idx], dwell[idx], seen[idx] = lm, ls, dm, True
    if not seen.all():
        missing = int(np.argmin(seen))
        name = "".join("ACGT"[(missing >> (2 * j)) & 3] for j in range(k))      # back to 5'->3': the last pore base first
        if not fill_missing:
            raise SystemExit(f"simulate: {path} has no row for {name} ({int((~seen).sum())} of {n} k-mers are missing); --fill-missing gives "
                             "them the table's means")
        w = np.array([r[1] for r in rows], dtype=np.float64)
        w = w if w.sum() > 0 else np.ones_like(w)
        for arr, col in ((level, 2), (sd, 3), (dwell, 4)):
            arr[~seen] = float(np.sum(w * np.array([r[col] for r in rows])) / w.sum())
    return (k, np.clip(np.rint(level * 1024), -(1 << 15), 1 << 15).astype(np.int32), np.clip(np.rint(sd * 1024), 0, 1 << 15).astype(np.int32),
            np.clip(np.rint(dwell * 256), 256, 1 << 23).astype(np.int32))


def build_model(args):
    if args.kmer_table:
        k, level, sd, dwell = read_kmer_table(args.kmer_table, args.fill_missing)
    else:
        k = args.kmer
        level, sd, dwell = standin_tables(k, args.model_seed)
    sd = np.clip(np.rint(sd * args.noise_scale), 0, 1 << 15).astype(np.int32)
    return SimModel(k, level, sd, dwell, dwell_cdf(args.dwell_min_frac))


# ------------------------------------------------------------------------------------------------ the reads
class ReadPlan:
    """what the host decides about one read: transcript t, the fragment [ref_start, ref_end) of it, the tail's length, the key and the
    modified sites [(transcript position, level_shift_q10, dwell_scale_q8)]; covered: [(transcript position, 0 / 1)] of every --modify
    site the fragment covers, in the file's order (--mods-out)"""
    __slots__ = ("read_id", "t", "ref_start", "ref_end", "tail", "key", "mods", "covered")

    def __init__(self, read_id, t, ref_start, ref_end, tail, key, mods=(), covered=()):
        self.read_id, self.t, self.ref_start, self.ref_end, self.tail, self.key, self.mods = read_id, t, ref_start, ref_end, tail, key, list(mods)
        self.covered = list(covered)


def read_sites(path, tr):
    """--modify's rows -> {transcript index: [(pos, level_shift_q10, dwell_scale_q8, fraction)]} in file order"""
    index = {n: t for t, n in reversed(list(enumerate(tr.names)))}
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            cols = line.split()
            if not cols or cols[0].startswith("#"):
                continue
            try:
                name, pos, shift, scale, frac = cols[0], int(cols[1]), float(cols[2]), float(cols[3]), float(cols[4])
            except (IndexError, ValueError):
                raise SystemExit(f"simulate: {path}, line {i + 1}: not ref_name pos level_shift dwell_scale fraction")
            if name not in index or not 0 <= pos < tr.length(index[name]):
                raise SystemExit(f"simulate: {path}, line {i + 1}: {name}:{pos} is not a position of the transcripts")
            if not (abs(shift) <= 31.99 and 1 / 256 <= scale <= 16 and 0 <= frac <= 1):
                raise SystemExit(f"simulate: {path}, line {i + 1}: level_shift within +-31.99, dwell_scale 1/256..16 and fraction 0..1")
            out.setdefault(index[name], []).append((pos, int(round(shift * 1024)), int(round(scale * 256)), frac))
    return out


def draw_reads(args, tr, rng, sites=None):
    """the ReadPlans of the run, drawn read by read"""
    n_tr = len(tr.names)
    plans = []
    for i in range(args.reads):
        for _ in range(1000):
            t = int(rng.integers(0, n_tr))
            n = tr.length(t)
            want = int(round(args.length_median * math.exp(args.length_sigma * rng.standard_normal())))
            F = min(max(want, args.min_length), n)
            if F > 0 and not (tr.codes[tr.offsets[t] + n - F: tr.offsets[t] + n] > 3).any():
                break
        else:
            raise SystemExit("simulate: a thousand draws in a row gave no fragment of ACGTU alone")
        tail = args.tail if args.tail is not None else int(round(args.tail_median * math.exp(args.tail_sigma * rng.standard_normal())))
        key = rng.integers(0, 1 << 32, 2, dtype=np.uint64).astype(np.uint32)
        mods, covered = [], []
        for pos, shift, scale, frac in (sites or {}).get(t, ()):
            if n - F <= pos < n:
                hit = rng.random() < frac
                covered.append((pos, int(hit)))
                if hit:
                    mods.append((pos, shift, scale))
        plans.append(ReadPlan(f"sim{args.seed}_{i:08d}", t, n - F, n, max(tail, 0), key, mods, covered))
    return plans


def write_mods(path, plans, tr):
    """--mods-out: read_id ref_name pos modified for every (read, --modify site it covers), from the draw of draw_reads"""
    with open(path, "w") as f:
        f.write("read_id\tref_name\tpos\tmodified\n")
        for p in plans:
            for pos, hit in p.covered:
                f.write(f"{p.read_id}\t{tr.names[p.t]}\t{pos}\t{hit}\n")


def compose(plan, tr, adapter):
    """-> (codes in pore order: adapter, tail, the fragment reversed; level_shift int16; dwell_scale uint16)"""
    o = int(tr.offsets[plan.t])
    frag = tr.codes[o + plan.ref_start: o + plan.ref_end][::-1]
    codes = np.concatenate([adapter, np.zeros(plan.tail, dtype=np.uint8), frag]).astype(np.uint8)
    shift, scale = np.zeros(len(codes), dtype=np.int16), np.full(len(codes), 256, dtype=np.uint16)
    for pos, s, d in plan.mods:
        b = len(adapter) + plan.tail + (plan.ref_end - 1 - pos)
        shift[b], scale[b] = s, d
    return codes, shift, scale


def tail_span(codes, base_first, n_samples, n_adapter, tail, k):
    """the samples of the tail bases whose whole k-mer (with the edge rule) is A: (start, end), or (-1, -1)"""
    L, h = len(codes), k // 2
    if tail == 0:
        return -1, -1
    is_a = codes == 0
    whole = np.ones(L, dtype=bool)
    for j in range(-h, h + 1):
        whole &= is_a[np.clip(np.arange(L) + j, 0, L - 1)]
    idx = np.flatnonzero(whole[n_adapter: n_adapter + tail]) + n_adapter
    if idx.size == 0:
        return -1, -1
    lo, hi = int(idx[0]), int(idx[-1]) + 1
    return int(base_first[lo]), int(base_first[hi]) if hi < L else int(n_samples)


def per_read_params(args, n):
    return dict(lead=np.full(n, args.lead_samples, np.int32), lead_level_q10=np.full(n, int(round(args.lead_level * 1024)), np.int32),
                lead_sd_q10=np.full(n, int(round(args.lead_sd * args.noise_scale * 1024)), np.int32), median=np.full(n, args.median, np.int32),
                scale_q10=np.full(n, int(round(args.mad * 1.4826 * 1024)), np.int32))


def simulate_batch(be, model, plans, tr, adapter, args):
    """-> (SimResult, [codes per read])"""
    parts = [compose(p, tr, adapter) for p in plans]
    seqs = [c for c, _, _ in parts]
    any_mod = any(p.mods for p in plans)
    kw = dict(per_read_params(args, len(plans)), keys=np.stack([p.key for p in plans]),
              level_shift=[s for _, s, _ in parts] if any_mod else None, dwell_scale=[d for _, _, d in parts] if any_mod else None)
    n_samples = be.sim_lengths(seqs, model, **kw)
    res = be.sim_signal(seqs, model, n_samples=n_samples, budget_bytes=args.budget_bytes, **kw)
    return res, seqs


def window_labels(norm, codes, base_first, first_fragment_base, args):
    """the truth-labelled windows of one read -> ([(window float32, signal_length, label)], {reason: dropped})"""
    windows, pad_end = get_windows(norm, args.chunk_len, args.step_size)
    sig_len = [args.chunk_len] * (len(windows) - 1) + [args.chunk_len - pad_end]
    dropped = {r: 0 for r in DROP_REASONS}
    kept = []
    frag_first = base_first[first_fragment_base:]
    frag_codes = codes[first_fragment_base:]
    for w, win in enumerate(windows):
        lo = w * args.step_size
        hi = lo + sig_len[w]
        a, e = np.searchsorted(frag_first, [lo, hi], side="left")
        label = frag_codes[a:e]
        if frag_first.size == 0 or lo < frag_first[0]:
            dropped["edge"] += 1
        elif label.size == 0:
            dropped["empty"] += 1
        elif label.size > args.max_label_len:
            dropped["too-long"] += 1
        elif ctc_rows(label) > sig_len[w]:
            dropped["infeasible"] += 1
        else:
            kept.append((win, sig_len[w], label))
    return kept, dropped


def run(args, be, tr, model, plans):
    """simulate the plans batch by batch and write every output.  Returns the counters."""
    os.makedirs(args.output, exist_ok=True)
    adapter = encode(args.adapter, "--adapter")
    st = {"reads": 0, "bases": 0, "samples": 0, "dwell_hist": np.zeros(32768, dtype=np.int64), "tails": [], "windows_kept": 0, "bad_signal": 0,
          "dropped": {r: 0 for r in DROP_REASONS}, "written": {"train": 0, "val": 0}}
    writers = {s: ShardWriter(os.path.join(args.shards, s), args.windows_per_shard) for s in ("train", "val")} if args.shards else None
    files = {name: open(os.path.join(args.output, name), "w") for name in ("truth.tsv", "read_ref.tsv", "truth.paf", "truth_moves.tsv")}
    files["truth.tsv"].write("read_id\tref_name\tref_start\tref_end\tn_samples\tlead\ttail_nt\ttail_start\ttail_end\n")
    files["read_ref.tsv"].write(TSV_HEADER)
    files["truth_moves.tsv"].write("read_id\tn_samples\tfirst_step\tlast_step\n")
    pending, n_files = {}, 0

    def flush_fast5():
        nonlocal pending, n_files
        if pending:
            fast5.write_multi_fast5(os.path.join(args.output, f"sim_{n_files:04d}.fast5"), pending, track_times=False)
            pending, n_files = {}, n_files + 1

    try:
        for at in range(0, len(plans), args.batch_reads):
            batch = plans[at: at + args.batch_reads]
            res, seqs = simulate_batch(be, model, batch, tr, adapter, args)
            norm = be.normalise_reads(res.raw, args.outlier_clip) if writers else None
            out = {s: ([], [], []) for s in ("train", "val")}
            for r, p in enumerate(batch):
                raw, bf, codes = res.raw[r], res.base_first[r], seqs[r]
                n, L, first = len(raw), len(codes), len(adapter) + p.tail
                name, tlen = tr.names[p.t], tr.length(p.t)
                a, e = tail_span(codes, bf, n, len(adapter), p.tail, model.k)
                files["truth.tsv"].write(f"{p.read_id}\t{name}\t{p.ref_start}\t{p.ref_end}\t{n}\t{args.lead_samples}\t{p.tail}\t{a}\t{e}\n")
                files["read_ref.tsv"].write(f"{p.read_id}\t{name}\t{tr.letters(p.t, p.ref_start, p.ref_end)}\n")
                F = p.ref_end - p.ref_start
                files["truth.paf"].write("\t".join(str(c) for c in (p.read_id, F, 0, F, "+", name, tlen, p.ref_start, p.ref_end, F, F, 255)) + "\n")
                ends = np.concatenate([bf[1:], [n]]).astype(np.int64) - 1
                fs, ls = bf[first:][::-1], ends[first:][::-1]            # written order: 5'->3', the last base the pore saw first
                files["truth_moves.tsv"].write(f"{p.read_id}\t{n}\t{','.join(str(int(v)) for v in fs)}\t{','.join(str(int(v)) for v in ls)}\n")
                st["reads"] += 1
                st["bases"] += L
                st["samples"] += n
                if L:
                    st["dwell_hist"] += np.bincount(ends - bf + 1, minlength=32768)
                st["tails"].append(p.tail)
                pending[p.read_id] = raw
                if len(pending) >= args.reads_per_file:
                    flush_fast5()
                if writers:
                    if norm[1][r] != 0:
                        st["bad_signal"] += 1
                        continue
                    kept, dropped = window_labels(norm[0][r], codes, bf, first, args)
                    for reason, c in dropped.items():
                        st["dropped"][reason] += c
                    split = "val" if is_val(p.read_id, args.val_fraction) else "train"
                    for win, sl, label in kept:
                        out[split][0].append(win), out[split][1].append(sl), out[split][2].append(label)
                    st["windows_kept"] += len(kept)
            if writers:
                for s, (sig, il, lab) in out.items():
                    if il:
                        writers[s].write(np.ascontiguousarray(np.stack(sig), dtype=np.float32), il, lab)
        flush_fast5()
    finally:
        for f in files.values():
            f.close()
    if writers:
        st["written"] = {s: w.n for s, w in writers.items()}
    st["files"] = n_files
    return st


def summary(st):
    h = st["dwell_hist"]
    nb = int(h.sum())
    md = "-"
    if nb:
        c = np.cumsum(h)
        lo, hi = int(np.searchsorted(c, (nb - 1) // 2 + 1)), int(np.searchsorted(c, nb // 2 + 1))
        md = f"{(lo + hi) / 2:.1f}"
    lines = [f"reads: {st['reads']}; bases: {st['bases']}; samples: {st['samples']}; fast5 files: {st['files']}",
             f"median dwell: {md}; median tail_nt: {float(np.median(st['tails'])):.1f}" if st["tails"] else f"median dwell: {md}; median tail_nt: -",
             f"windows: {st['windows_kept']} kept (train {st['written']['train']}, val {st['written']['val']}); dropped "
             + "; ".join(f"{r}: {st['dropped'][r]}" for r in DROP_REASONS) + f"; reads with a flat signal: {st['bad_signal']}"]
    return "\n".join(lines) + "\n"


def build_parser():
    ap = argparse.ArgumentParser(prog="simulate", description="Simulate direct-RNA reads with known truth from transcripts, on one GPU.  "
                                 "Without --kmer-table the pore model is a stand-in and NO pore.")
    ap.add_argument("fasta", help="transcripts, FASTA or FASTA.gz, written 5'->3'")
    ap.add_argument("-o", "--output", required=True, help="directory for the fast5 files and the truth files")
    ap.add_argument("--reads", required=True, type=int, help="reads to simulate")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--kmer-table", default=None, help="the pore model: a `resquiggle --kmer-table` TSV")
    ap.add_argument("--fill-missing", action="store_true", help="k-mers the table lacks take its count-weighted means")
    ap.add_argument("--model-seed", default=0, type=int, help="seed of the stand-in pore model (no --kmer-table)")
    ap.add_argument("--kmer", default=5, type=int, help="k of the stand-in (odd, 1..9)")
    ap.add_argument("--field", default=None, type=int, help="keep only records whose header, split on |, has --value in this field (0-based)")
    ap.add_argument("--value", default=None, help="see --field")
    ap.add_argument("--protein-coding", action="store_true", help="--field 7 --value protein_coding (GENCODE headers)")
    ap.add_argument("--length-median", default=1200.0, type=float, help="median fragment length in bases (log-normal)")
    ap.add_argument("--length-sigma", default=0.5, type=float)
    ap.add_argument("--min-length", default=200, type=int)
    ap.add_argument("--tail-median", default=80.0, type=float, help="median tail length in nucleotides (log-normal)")
    ap.add_argument("--tail-sigma", default=0.5, type=float)
    ap.add_argument("--tail", default=None, type=int, help="a fixed tail length")
    ap.add_argument("--adapter", default=DEFAULT_ADAPTER, help="the bases before the tail, in the order the pore sees them")
    ap.add_argument("--lead-samples", default=400, type=int, help="samples before the first base")
    ap.add_argument("--lead-level", default=2.0, type=float, help="their level in z")
    ap.add_argument("--lead-sd", default=0.3, type=float)
    ap.add_argument("--dwell-min-frac", default=0.2, type=float, help="the least dwell as a share of the k-mer's mean")
    ap.add_argument("--median", default=600, type=int, help="DAQ value of z = 0")
    ap.add_argument("--mad", default=60.0, type=float, help="DAQ units of one MAD: z = (x - median) / (1.4826 mad)")
    ap.add_argument("--noise-scale", default=1.0, type=float, help="multiplies every sd")
    ap.add_argument("--modify", default=None, help="sites to modify: ref_name pos level_shift dwell_scale fraction")
    ap.add_argument("--mods-out", default=None, help="with --modify: write which reads were modified at which site (read_id ref_name pos modified)")
    ap.add_argument("--reads-per-file", default=4000, type=int)
    ap.add_argument("--shards", default=None, help="also write truth-labelled training shards under this directory")
    ap.add_argument("--chunk-len", default=WINDOW, type=int)
    ap.add_argument("--step-size", default=128, type=int)
    ap.add_argument("--outlier-clip", default=4, type=int)
    ap.add_argument("--val-fraction", default=0.05, type=float)
    ap.add_argument("--windows-per-shard", default=50000, type=int)
    ap.add_argument("--max-label-len", default=255, type=int)
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device call (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per launch (0: a quarter of free memory)")
    return ap


def check_args(args):
    if args.protein_coding:
        if args.field is not None or args.value is not None:
            raise SystemExit("simulate: --protein-coding is --field 7 --value protein_coding: give one or the other")
        args.field, args.value = 7, "protein_coding"
    if (args.field is None) != (args.value is None) or (args.field is not None and args.field < 0):
        raise SystemExit("simulate: --field (counted from 0) and --value go together")
    if args.reads < 0 or args.batch_reads < 1 or args.reads_per_file < 1 or args.budget_bytes < 0 or args.windows_per_shard < 1:
        raise SystemExit("simulate: --reads and --budget-bytes at least 0; --batch-reads, --reads-per-file and --windows-per-shard at least 1")
    if args.kmer_table is None and (args.kmer < 1 or args.kmer > 9 or args.kmer % 2 == 0):
        raise SystemExit("simulate: --kmer must be odd, 1..9")
    if args.fill_missing and not args.kmer_table:
        raise SystemExit("simulate: --fill-missing goes with --kmer-table")
    if args.min_length < 1 or not args.length_median > 0 or args.length_sigma < 0 or not args.tail_median >= 0 or args.tail_sigma < 0:
        raise SystemExit("simulate: lengths must be positive and sigmas at least 0")
    if args.tail is not None and args.tail < 0:
        raise SystemExit("simulate: --tail must be at least 0")
    if args.lead_samples < 0 or abs(args.lead_level) > 32 or not 0 <= args.lead_sd * args.noise_scale <= 32 or args.noise_scale < 0:
        raise SystemExit("simulate: --lead-samples at least 0, --lead-level within +-32 z, sds 0..32 z")
    if not 0 <= args.dwell_min_frac <= 1:
        raise SystemExit("simulate: --dwell-min-frac must be 0..1")
    if not -32768 <= args.median <= 32767 or not 1 <= round(args.mad * 1.4826 * 1024) <= 1 << 26:
        raise SystemExit("simulate: --median must be an int16 value and --mad positive, at most 44000")
    if args.mods_out is not None and not args.modify:
        raise SystemExit("simulate: --mods-out goes with --modify")
    if args.shards:
        if args.chunk_len != WINDOW:
            raise SystemExit(f"simulate: --chunk-len must be {WINDOW}: a shard's `signal` feature holds {WINDOW} samples")
        if not 1 <= args.step_size <= args.chunk_len or not 0 <= args.val_fraction <= 1 or not 1 <= args.max_label_len <= 255:
            raise SystemExit("simulate: --step-size 1..chunk-len, --val-fraction 0..1, --max-label-len 1..255")


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    try:
        tr = Transcripts.read(args.fasta, args.field, args.value)
    except (OSError, ValueError) as e:
        raise SystemExit(f"simulate: {e}")
    if not tr.names:
        raise SystemExit(f"simulate: {args.fasta} holds no record that is kept")
    model = build_model(args)
    sites = read_sites(args.modify, tr) if args.modify else None
    plans = draw_reads(args, tr, np.random.Generator(np.random.PCG64(args.seed)), sites)
    if args.mods_out is not None:
        write_mods(args.mods_out, plans, tr)
    os.makedirs(args.output, exist_ok=True)
    for f in os.listdir(args.output):   # a rerun into the same directory leaves no file of the run before
        if f.startswith("sim_") and f.endswith(".fast5"):
            os.remove(os.path.join(args.output, f))
    if args.shards:
        for split in ("train", "val"):
            d = os.path.join(args.shards, split)
            if os.path.isdir(d):
                for f in os.listdir(d):
                    if f.startswith("shard-") and f.endswith(".tfrecords"):
                        os.remove(os.path.join(d, f))
    with Backend(args.device) as be:
        st = run(args, be, tr, model, plans)
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
    sys.exit(0)
