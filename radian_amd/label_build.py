"""Build the training shards `train` and `evaluate` read -- labelled signal windows -- from fast5 reads and their reference sequences.

    python -m radian_amd.label_build fast5_dir read_ref.tsv -o shards_dir
           [--sig-model models/sig2seq.h5 --sig-config models/sig2seq.yaml --chunk-len 1024 --step-size 128 --outlier-clip 4 --beam-width 6]
           [--min-identity 0.9] [--min-call 8] [--max-label-len 255] [--val-fraction 0.05] [--windows-per-shard 50000]
           [--manifest windows.tsv] [--device N] [--budget-bytes B] [--batch-reads R]

The reference trains on `{shards_dir}/{train,val}/*.tfrecords` (radian/train.py:48-79, radian/data.py) and ships nothing that writes
them.  What a labelled window is, is therefore this project's definition -- the one other basecallers' "save CTC data" modes use:

  1. every read is normalised and cut into windows as basecall does (mad_normalise, get_windows: float32, the last window's tail
     zero-padded, signal_length = the samples the window really holds) and every window is basecalled alone (chunk decode);
  2. the read's reference sequence -- column 3 of read_ref.tsv, the file `align` takes: first line skipped, `read <tab> text <tab> seq` --
     is turned into decode order (reversed, not complemented: the signal runs 3'->5'); U = T, lower case accepted, any other letter is
     code 4, which matches nothing;
  3. the window's call is FITTED into that sequence on the GPU (rd_fit_batch: the whole call aligned with align's scores 2 / -4 / -4 / -2,
     the reference before and after the span free); the window's label is the reference's span ref_dec[ref_start:ref_end);
  4. a window is kept when its call has >= --min-call labels, the fit's identity n_match / (n_match + n_sub + n_ins + n_del) is
     >= --min-identity, its label is not empty, holds no code 4, is at most --max-label-len long and is CTC-feasible (its length plus
     its adjacent repeats <= signal_length) -- and when it lies on the read's chain: of the windows that pass, the longest subsequence
     whose ref_start does not decrease in window order (of several longest ones, the lexicographically earliest window indices).
     The chain drops short calls that fitted a repeat elsewhere in the transcript.

A read goes to val/ when crc32c(read_id) % 10000 < val_fraction * 10000, else to train/; each split's windows are written in input order
(fast5 files sorted by path, reads in file order) to `{split}/shard-{k:05d}.tfrecords`, --windows-per-shard records each.  The bytes
written depend on the inputs and options only -- not on --batch-reads (reads per device batch) and not on the run.  --manifest writes one
row per window: read id, window, status (kept / short / low-identity / off-chain / too-long / infeasible / has-N / no-reference),
ref_start, ref_end, score, n_match, n_sub, n_ins, n_del.  A read without a row in the TSV, an empty read and one whose signal cannot be
normalised are skipped and counted.  One GPU; there is no CPU path.
"""
import argparse
import bisect
import os
import sys
import time

import numpy as np

from . import fast5
from .backend import ALIGN_SCORES, Backend, tfrecord_write
from .basecall import load_dilations, load_sig_model
from .preprocess import get_windows
from .tfrecord import WINDOW, crc32c

STATUSES = ("kept", "short", "low-identity", "off-chain", "too-long", "infeasible", "has-N", "no-reference")
_CODE = np.full(256, 4, dtype=np.uint8)
for _k, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _letters:
        _CODE[ord(_c)] = _k


def encode_reference(seq):
    """a 5'->3' sequence as written in the TSV -> codes in decode order (reversed; A C G T/U = 0..3 in either case, anything else 4)"""
    return np.ascontiguousarray(_CODE[np.frombuffer(seq.encode("latin-1", "replace"), dtype=np.uint8)][::-1])


def read_ref_tsv(path):
    """{read id: reference sequence} of `read <tab> text <tab> seq` rows after a header line (radian/align.py:68-73; a later id overrides
    an earlier one).  A row of another shape raises ValueError naming its line."""
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            if i == 0:
                continue
            line = line.rstrip("\n").rstrip("\r")
            if not line:
                continue
            cols = line.split("\t")
            if len(cols) != 3:
                raise ValueError(f"{path}: line {i + 1}: {len(cols)} tab-separated fields, not read, text, seq")
            out[cols[0]] = cols[2]
    return out


def is_val(read_id, val_fraction):
    """the split of a read: a function of its id alone"""
    return crc32c(read_id.encode("utf-8")) % 10000 < val_fraction * 10000


def ctc_rows(label):
    """rows a CTC path of the label needs: its length plus its adjacent repeats"""
    label = np.asarray(label)
    return int(label.size + np.count_nonzero(label[1:] == label[:-1]))


def chain(starts):
    """positions of the longest subsequence of starts that does not decrease; of several, the lexicographically earliest positions"""
    n = len(starts)
    tail = [0] * n          # the longest chain that begins at k: a longest non-decreasing run of -starts read from the right
    tops = []
    for k in range(n - 1, -1, -1):
        x = -int(starts[k])
        pos = bisect.bisect_right(tops, x)
        if pos == len(tops):
            tops.append(x)
        else:
            tops[pos] = x
        tail[k] = pos + 1
    out, want, floor = [], len(tops), None
    for k in range(n):
        if want and tail[k] == want and (floor is None or starts[k] >= floor):
            out.append(k)
            floor, want = starts[k], want - 1
    return out


def select_windows(calls, signal_lengths, ref_dec, fit, first, args):
    """statuses of one read's windows.  fit: the batch's FitResult, first: the row of the read's first window with a call in it (windows
    without a call have no row).  Returns [(status, row or -1)] in window order."""
    rows, k = [], first
    for call, sl in zip(calls, signal_lengths):
        if len(call) == 0:
            rows.append(["short", -1])
            continue
        nm, ns, ni, nd = (int(c) for c in fit.counts[k])
        lo, hi = int(fit.ref_start[k]), int(fit.ref_end[k])
        label = ref_dec[lo:hi]
        if len(call) < args.min_call:
            st = "short"
        elif nm / (nm + ns + ni + nd) < args.min_identity or hi == lo:
            st = "low-identity"
        elif (label == 4).any():
            st = "has-N"
        elif hi - lo > args.max_label_len:
            st = "too-long"
        elif ctc_rows(label) > sl:
            st = "infeasible"
        else:
            st = "kept"
        rows.append([st, k])
        k += 1
    cand = [w for w, (st, _) in enumerate(rows) if st == "kept"]
    on = set(cand[c] for c in chain([int(fit.ref_start[rows[w][1]]) for w in cand]))
    for w in cand:
        if w not in on:
            rows[w][0] = "off-chain"
    return rows


class ShardWriter:
    """one split's windows, appended in order to shard-{k:05d}.tfrecords, per_shard records each"""

    def __init__(self, directory, per_shard):
        self.dir, self.per_shard, self.n = directory, per_shard, 0
        os.makedirs(directory, exist_ok=True)

    def write(self, signals, input_len, labels):
        at = 0
        while at < len(input_len):
            k, used = divmod(self.n, self.per_shard)
            take = min(self.per_shard - used, len(input_len) - at)
            tfrecord_write(os.path.join(self.dir, f"shard-{k:05d}.tfrecords"), signals[at: at + take], input_len[at: at + take],
                           labels[at: at + take], append=used > 0)
            self.n += take
            at += take


def _batches(reads, max_reads, max_samples=32 << 20):
    batch, samples = [], 0
    for r in reads:
        batch.append(r)
        samples += len(r[1])
        if len(batch) >= max_reads or samples >= max_samples:
            yield batch
            batch, samples = [], 0
    if batch:
        yield batch


def run(args, be, reads, refs):
    """reads: iterable of (read id, raw int16 samples) in input order; refs: {read id: sequence as in the TSV}.  Returns the counters."""
    st = {"reads": 0, "reads_used": 0, "reads_no_reference": 0, "reads_bad_signal": 0, "windows": 0, "label_lengths": [],
          "t_basecall": 0.0, "t_fit": 0.0, "t_select": 0.0, "t_write": 0.0, "cells": 0, **{s: 0 for s in STATUSES}}
    writers = {s: ShardWriter(os.path.join(args.output, s), args.windows_per_shard) for s in ("train", "val")}
    manifest = open(args.manifest, "w") if args.manifest else None
    if manifest:
        manifest.write("read_id\twindow\tstatus\tref_start\tref_end\tscore\tn_match\tn_sub\tn_ins\tn_del\n")
    try:
        for batch in _batches(reads, args.batch_reads):
            st["reads"] += len(batch)
            todo = []
            for rid, raw in batch:
                raw = np.ascontiguousarray(raw, dtype=np.int16)
                if rid not in refs:
                    nw = be.count_windows(len(raw), args.chunk_len, args.step_size) if len(raw) else 0
                    st["reads_no_reference"] += 1
                    st["windows"] += nw
                    st["no-reference"] += nw
                    if manifest:
                        for w in range(nw):
                            manifest.write(f"{rid}\t{w}\tno-reference\t0\t0\t0\t0\t0\t0\t0\n")
                elif len(raw) == 0:
                    st["reads_bad_signal"] += 1
                else:
                    todo.append((rid, raw))
            if not todo:
                continue
            t0 = time.perf_counter()
            raws = [raw for _, raw in todo]
            calls, status = be.basecall_raw_chunk(raws, args.outlier_clip, args.chunk_len, args.step_size, args.beam_width)
            norm, _ = be.normalise_reads(raws, args.outlier_clip)
            t1 = time.perf_counter()
            good = [r for r in range(len(todo)) if status[r] == 0]
            st["reads_bad_signal"] += len(todo) - len(good)
            ref_dec = [encode_reference(refs[todo[r][0]]) for r in good]
            queries, query_ref, first = [], [], []
            for g, r in enumerate(good):
                first.append(len(queries))
                for c in calls[r]:
                    if len(c):
                        queries.append(c)
                        query_ref.append(g)
                        st["cells"] += len(c) * len(ref_dec[g])
            fit = be.fit_batch(ref_dec, queries, query_ref, ALIGN_SCORES, budget_bytes=args.budget_bytes)
            t2 = time.perf_counter()
            out = {s: ([], [], []) for s in writers}
            for g, r in enumerate(good):
                rid = todo[r][0]
                windows, pad_end = get_windows(norm[r], args.chunk_len, args.step_size)
                sig_len = [args.chunk_len] * (len(windows) - 1) + [args.chunk_len - pad_end]
                rows = select_windows(calls[r], sig_len, ref_dec[g], fit, first[g], args)
                split = "val" if is_val(rid, args.val_fraction) else "train"
                st["reads_used"] += 1
                st["windows"] += len(rows)
                for w, (status_w, k) in enumerate(rows):
                    st[status_w] += 1
                    if status_w == "kept":
                        label = ref_dec[g][int(fit.ref_start[k]): int(fit.ref_end[k])]
                        out[split][0].append(windows[w])
                        out[split][1].append(sig_len[w])
                        out[split][2].append(label)
                        st["label_lengths"].append(len(label))
                    if manifest:
                        f = (int(fit.ref_start[k]), int(fit.ref_end[k]), int(fit.score[k]), *(int(c) for c in fit.counts[k])) if k >= 0 else (0,) * 7
                        manifest.write(f"{rid}\t{w}\t{status_w}\t" + "\t".join(str(v) for v in f) + "\n")
            t3 = time.perf_counter()
            for s, (sig, il, lab) in out.items():
                if il:
                    writers[s].write(np.ascontiguousarray(np.stack(sig), dtype=np.float32), il, lab)
            t4 = time.perf_counter()
            for key, dt in (("t_basecall", t1 - t0), ("t_fit", t2 - t1), ("t_select", t3 - t2), ("t_write", t4 - t3)):
                st[key] += dt
    finally:
        if manifest:
            manifest.close()
    st["written"] = {s: w.n for s, w in writers.items()}
    return st


def summary(st):
    ll = st["label_lengths"]
    lines = [f"reads: {st['reads']} seen, {st['reads_used']} used; no reference: {st['reads_no_reference']}; empty or flat signal: {st['reads_bad_signal']}",
             f"windows: {st['windows']} seen, {st['kept']} kept (train {st['written']['train']}, val {st['written']['val']}); "
             + "; ".join(f"{s}: {st[s]}" for s in STATUSES[1:]),
             f"label length median: {float(np.median(ll)):.1f}" if ll else "label length median: -"]
    return "\n".join(lines) + "\n"


def build_parser():
    ap = argparse.ArgumentParser(prog="label_build", description="Labelled signal windows (TFRecord shards for train / evaluate) from fast5 reads and their reference sequences, on one GPU.")
    ap.add_argument("fast5_dir", help="directory of single/multi fast5 files")
    ap.add_argument("ref_tsv", help="TSV with a header line, then read_id <tab> text <tab> reference sequence (align's file)")
    ap.add_argument("-o", "--output", required=True, help="shards directory: {train,val}/shard-NNNNN.tfrecords are written under it")
    ap.add_argument("--sig-model", default="models/sig2seq.h5")
    ap.add_argument("--sig-config", default="models/sig2seq.yaml")
    ap.add_argument("--chunk-len", default=WINDOW, type=int, help="window length; the shards' format fixes it at 1024")
    ap.add_argument("--step-size", default=128, type=int)
    ap.add_argument("--outlier-clip", default=4, type=int)
    ap.add_argument("--beam-width", default=6, type=int)
    ap.add_argument("--min-identity", default=0.9, type=float, help="least n_match / (n_match + n_sub + n_ins + n_del) of a window's fit")
    ap.add_argument("--min-call", default=8, type=int, help="least labels in a window's call")
    ap.add_argument("--max-label-len", default=255, type=int, help="longest label kept (train and evaluate take up to 255)")
    ap.add_argument("--val-fraction", default=0.05, type=float, help="share of the reads (by a hash of their id) that goes to val/")
    ap.add_argument("--windows-per-shard", default=50000, type=int)
    ap.add_argument("--manifest", default=None, help="per-window TSV")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device buffer per batch of the fit (0: a quarter of free memory)")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.chunk_len != WINDOW:
        raise SystemExit(f"label_build: --chunk-len must be {WINDOW}: a shard's `signal` feature holds {WINDOW} samples")
    if not 1 <= args.step_size <= args.chunk_len:
        raise SystemExit("label_build: --step-size must be 1..chunk-len")
    if not 0.0 <= args.val_fraction <= 1.0:
        raise SystemExit("label_build: --val-fraction must be 0..1")
    if args.windows_per_shard < 1 or args.batch_reads < 1 or args.min_call < 1:
        raise SystemExit("label_build: --windows-per-shard, --batch-reads and --min-call must be at least 1")
    if not 1 <= args.max_label_len <= 255:
        raise SystemExit("label_build: --max-label-len must be 1..255")
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"label_build: {args.fast5_dir}: no such directory")
    try:
        refs = read_ref_tsv(args.ref_tsv)
    except (OSError, ValueError) as e:
        raise SystemExit(f"label_build: {e}")
    dilations = load_dilations(args.sig_config)
    weights = load_sig_model(args.sig_model, dilations)
    for split in ("train", "val"):   # a rerun into the same directory leaves no shard of the run before
        d = os.path.join(args.output, split)
        if os.path.isdir(d):
            for f in os.listdir(d):
                if f.startswith("shard-") and f.endswith(".tfrecords"):
                    os.remove(os.path.join(d, f))
    files = sorted(fast5.list_files(args.fast5_dir))
    reads = ((r.read_id, r.get_raw_data()) for p in files for r in fast5.iter_reads(p))
    with Backend(args.device) as be:
        be.load_weights(weights, dilations)
        st = run(args, be, reads, refs)
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
    sys.exit(0)
