"""Signal-to-reference alignment ("resquiggle", "eventalign"): puts every read's REFERENCE span on its raw signal and reports, for every
reference base, which samples it sits on and what the current was there.  fast5 and `map`'s read_ref.tsv in, one event table per input
file out, on one GPU.

    python -m radian_amd.resquiggle fast5_dir read_ref.tsv -o out_dir
           [--sig-model models/sig2seq.h5 --sig-config models/sig2seq.yaml --chunk-len 1024 --step-size 128 --outlier-clip 4]
           [--precision fp32 --logits f32] [--summary PATH] [--kmer-table PATH --kmer 5] [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour.  Every read is normalised, run through the signal model and assembled as `python -m radian_amd.basecall` does
in global mode; no beam search is run.  The read's span -- column 3 of read_ref.tsv, reversed into decode order, U = T -- is aligned
against the read's probability rows (the forced CTC alignment of DESIGN.md section 16, exact to the bit) and the event of every base is
cut from the raw samples on the device (rd_resquiggle_raw).  One row of the matrix is one raw sample, so every
position is a sample index into the read.

{stem}.events.tsv   one row per reference base of every `ok` read, in span order 5'->3' (the signal runs 3'->5': the sample indices
                    decrease): read_id, ref_name, ref_pos (0-based, in the span), base, start, end (samples [start, end)), n, mean, stdv
                    (raw DAQ units; fp64 on the host from the integer sums; population form), min, max, level = (mean - median) /
                    (1.4826 MAD) with the median and MAD of the read's raw samples (mad_normalise's scale, unclipped), q (the alignment's
                    quality of that base: low where the read disagrees with the reference)
--summary           per read: read_id, status, n_samples, ref_len, score, score_per_base, median_dwell, first_sample, last_sample
--kmer-table        the pore-model table the events imply: for odd --kmer k, the k-mer of the span centred on each base (bases within k//2
                    of an end are skipped): kmer, n_events, level_mean, level_sd, dwell_mean; sorted by k-mer

A read is `ok`, or is counted and left out: `no-reference` (its id is not in the TSV), `has-N` (its span holds a letter outside ACGTU),
`no-path` (no CTC path of the span fits the read), `too-large` (its alignment does not fit --budget-bytes), `signal` (empty, or its MAD is
zero).  Every file is bit-identical across --batch-reads and across runs.  The levels are only as meaningful as the signal model: with
weights that were not trained on real reads they say nothing about a pore."""
import argparse
import math
import os
import sys

import numpy as np

from . import fast5
from .backend import Backend, CTCALIGN_NO_PATH, CTCALIGN_OK, CTCALIGN_TOO_LARGE
from .basecall import apply_artifacts, load_artifacts, report_skipped
from .fastq import _batches
from .label_build import encode_reference, read_ref_tsv

STATUSES = ("ok", "no-reference", "has-N", "no-path", "too-large", "signal")
EVENT_COLUMNS = ("read_id", "ref_name", "ref_pos", "base", "start", "end", "n", "mean", "stdv", "min", "max", "level", "q")
SUMMARY_COLUMNS = ("read_id", "status", "n_samples", "ref_len", "score", "score_per_base", "median_dwell", "first_sample", "last_sample")
KMER_COLUMNS = ("kmer", "n_events", "level_mean", "level_sd", "dwell_mean")


def read_ref_names(path):
    """{read id: transcript name}: column 2 of the rows label_build.read_ref_tsv reads (which checks their shape)"""
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if i and len(cols) == 3:
                out[cols[0]] = cols[1]
    return out


def reference_status(read_id, refs):
    """-> (status or None, codes in decode order or None): `no-reference`, `has-N`, or the labels to align"""
    if read_id not in refs:
        return "no-reference", None
    codes = encode_reference(refs[read_id])
    if (codes > 3).any():
        return "has-N", None
    return None, codes


def read_scale(raw):
    """(median, MAD) of the read's raw samples, as radian/preprocess.py's mad_normalise takes them"""
    x = np.asarray(raw, dtype=np.float64)
    median = float(np.median(x))
    return median, float(np.median(np.abs(x - median)))


def event_moments(n, s, sq):
    """(mean, stdv) of an event from its integer count, sum and sum of squares: fp64, population form, the variance clamped at 0"""
    n, s, sq = float(n), float(s), float(sq)
    mean = s / n
    return mean, math.sqrt(max(sq / n - mean * mean, 0.0))


def event_level(mean, median, mad):
    return (mean - median) / (1.4826 * mad)


def event_rows(read_id, ref_name, span, raw, ev, qual, scale=None, skipped=None):
    """the rows of one `ok` read: span as written (5'->3'); ev = (start, end, sum, sumsq, min, max) and qual in decode order (label k is
    span position L - 1 - k); scale: the (median, MAD) the levels are taken on (default: the read's own); skipped (`eventalign --events`):
    per label, true for a base the path jumped over -- it writes no row, its level is None and its dwell 0.  -> [(columns as strings)],
    levels, dwells in span order"""
    L = len(span)
    median, mad = scale if scale is not None else read_scale(raw)
    start, end, s, sq, mn, mx = ev
    rows, levels, dwells = [], [], []
    for p in range(L):
        k = L - 1 - p
        n = int(end[k]) - int(start[k])
        if skipped is not None and skipped[k]:
            levels.append(None)
            dwells.append(0)
            continue
        mean, stdv = event_moments(n, int(s[k]), int(sq[k]))
        level = event_level(mean, median, mad)
        rows.append((read_id, ref_name, str(p), span[p].upper(), str(int(start[k])), str(int(end[k])), str(n), f"{mean:.4f}", f"{stdv:.4f}",
                     str(int(mn[k])), str(int(mx[k])), f"{level:.6f}", str(int(qual[k]))))
        levels.append(level)
        dwells.append(n)
    return rows, levels, dwells


class KmerTable:
    """per k-mer: events, the sum and the sum of squares of their levels, the sum of their dwells -- accumulated in read order, base by base"""

    def __init__(self, k):
        if k < 1 or k % 2 == 0:
            raise ValueError("--kmer must be odd and at least 1")
        self.k, self.acc = k, {}

    def add(self, span, levels, dwells):
        k, h = self.k, self.k // 2
        seq = span.upper().replace("U", "T")
        for p in range(h, len(seq) - h):
            if levels[p] is None:      # a skipped base (eventalign --events)
                continue
            a = self.acc.setdefault(seq[p - h: p + h + 1], [0, 0.0, 0.0, 0])
            a[0] += 1
            a[1] += levels[p]
            a[2] += levels[p] * levels[p]
            a[3] += dwells[p]

    def rows(self):
        out = []
        for kmer in sorted(self.acc):
            n, s, sq, d = self.acc[kmer]
            mean = s / n
            out.append((kmer, str(n), f"{mean:.6f}", f"{math.sqrt(max(sq / n - mean * mean, 0.0)):.6f}", f"{d / n:.4f}"))
        return out

    def write(self, path):
        with open(path, "w") as f:
            f.write("\t".join(KMER_COLUMNS) + "\n")
            for r in self.rows():
                f.write("\t".join(r) + "\n")


def _median_of_counts(counts):
    """the median of a multiset given as {value: count} (the mean of the two middle values)"""
    n = sum(counts.values())
    if n == 0:
        return None
    lo, hi, acc, a, b = (n - 1) // 2, n // 2, 0, None, None
    for v in sorted(counts):
        acc += counts[v]
        if a is None and lo < acc:
            a = v
        if b is None and hi < acc:
            b = v
            break
    return (a + b) / 2


def run(args, be, reads, refs, names, open_out):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; refs / names: {read id: span} / {read id: transcript name};
    open_out(stem) -> the text file of that input file (its header is written here).  Returns the counters."""
    st = {"reads": 0, "written": 0, "bases": 0, "dwell": {}, "score_per_base": [], **{s: 0 for s in STATUSES}}
    kt = KmerTable(args.kmer) if args.kmer_table else None
    summ = open(args.summary, "w") if args.summary else None
    if summ:
        summ.write("\t".join(SUMMARY_COLUMNS) + "\n")

    def done(rid, status, n_samples, ref_len, extra=("-",) * 5):
        st[status] += 1
        if summ:
            summ.write("\t".join((rid, status, str(n_samples), str(ref_len)) + tuple(extra)) + "\n")

    try:
        for batch in _batches(reads, args.batch_reads):
            st["reads"] += len(batch)
            todo, verdict = [], []
            for stem, rid, raw in batch:
                raw = np.ascontiguousarray(raw, dtype=np.int16)
                status, codes = reference_status(rid, refs)
                if status is None and len(raw) == 0:
                    report_skipped(rid, 2)
                    status = "signal"
                verdict.append((stem, rid, raw, status))
                if status is None:
                    todo.append((raw, codes))
            aln = ev = rst = None
            if todo:
                aln, ev, rst = be.resquiggle_raw([t[0] for t in todo], [t[1] for t in todo], args.outlier_clip, args.chunk_len, args.step_size,
                                                 budget_bytes=args.budget_bytes, allow_too_large=True)
            r = -1
            for stem, rid, raw, status in verdict:
                ref_len = len(refs[rid]) if rid in refs else 0
                if status is not None:
                    done(rid, status, len(raw), ref_len)
                    continue
                r += 1
                a_st = int(aln.status[r])
                if int(rst[r]) != 0:
                    report_skipped(rid, int(rst[r]))
                    done(rid, "signal", len(raw), ref_len)
                elif a_st == CTCALIGN_TOO_LARGE:
                    done(rid, "too-large", len(raw), ref_len)
                elif a_st == CTCALIGN_NO_PATH:
                    done(rid, "no-path", len(raw), ref_len)
                else:
                    assert a_st == CTCALIGN_OK
                    span = refs[rid]
                    rows, levels, dwells = event_rows(rid, names.get(rid, ""), span, raw,
                                                      (ev.start[r], ev.end[r], ev.sum[r], ev.sumsq[r], ev.min[r], ev.max[r]), aln.qual[r])
                    out = open_out(stem)
                    for row in rows:
                        out.write("\t".join(row) + "\n")
                    st["written"] += 1
                    st["bases"] += len(rows)
                    for d in dwells:
                        st["dwell"][d] = st["dwell"].get(d, 0) + 1
                    score = float(aln.score[r])
                    spb = score / len(rows) if rows else float("nan")
                    if rows:
                        st["score_per_base"].append(spb)
                    if kt:
                        kt.add(span, levels, dwells)
                    md = float(np.median(dwells)) if dwells else float("nan")
                    first = int(aln.first_step[r][0]) if rows else -1
                    last = int(aln.last_step[r][-1]) if rows else -1
                    done(rid, "ok", len(raw), ref_len, (repr(score), f"{spb:.6f}", f"{md:.1f}", str(first), str(last)))
    finally:
        if summ:
            summ.close()
    if kt:
        kt.write(args.kmer_table)
    return st


def summary(st):
    md = _median_of_counts(st["dwell"])
    spb = st["score_per_base"]
    return (f"reads: {st['reads']} seen, {st['written']} written\n"
            f"bases: {st['bases']}\n"
            + (f"median dwell: {md:.1f} samples\n" if md is not None else "median dwell: -\n")
            + (f"median score per base: {float(np.median(spb)):.4f}\n" if spb else "median score per base: -\n")
            + "status: " + "; ".join(f"{s}: {st[s]}" for s in STATUSES) + "\n")


def build_parser():
    ap = argparse.ArgumentParser(prog="resquiggle", description="Align every read's reference span to its raw signal on one GPU and write the "
                                 "per-base event table: samples, current statistics, normalised level and quality of every reference base.")
    ap.add_argument("fast5_dir", help="Directory of single/multi fast5 files.")
    ap.add_argument("read_ref", help="read_ref.tsv as `map` writes it: read_id <tab> transcript name <tab> span, after a header line")
    ap.add_argument("-o", "--out-dir", required=True, help="Directory to output {stem}.events.tsv files (one per input file).")
    # the model / geometry flags of basecall (the RNA model and the beam take no part: no search is run)
    ap.add_argument("--chunk-len", default=1024, type=int)
    ap.add_argument("--step-size", default=128, type=int)
    ap.add_argument("--outlier-clip", default=4, type=int)
    ap.add_argument("--sig-model", default="models/sig2seq.h5")
    ap.add_argument("--sig-config", default="models/sig2seq.yaml")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "f16x3", "bf16x3"])
    ap.add_argument("--logits", default="f32", choices=["f32", "f16"])
    ap.add_argument("--summary", default=None, help="per-read TSV: status, score, dwell, the samples the span covers")
    ap.add_argument("--kmer-table", default=None, help="TSV of the level and dwell of every k-mer of the spans (the pore-model table the data imply)")
    ap.add_argument("--kmer", default=5, type=int, help="k of --kmer-table (odd)")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per alignment launch (0: a quarter of free memory)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not 1 <= args.step_size <= args.chunk_len:
        raise SystemExit("resquiggle: --step-size must be 1..chunk-len")
    if args.batch_reads < 1 or args.budget_bytes < 0:
        raise SystemExit("resquiggle: --batch-reads must be at least 1 and --budget-bytes at least 0")
    if args.kmer < 1 or args.kmer % 2 == 0:
        raise SystemExit("resquiggle: --kmer must be odd")
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"resquiggle: {args.fast5_dir}: no such directory")
    refs, names = read_ref_tsv(args.read_ref), read_ref_names(args.read_ref)
    os.makedirs(args.out_dir, exist_ok=True)
    args.rna_model, args.decode_type = "None", "global"   # load_artifacts: the signal model only
    art = load_artifacts(args)
    files = fast5.list_files(args.fast5_dir)   # Path.rglob order, as basecall
    stems = {}
    for p in files:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise SystemExit(f"resquiggle: {p} and {stems[stem]} would both be written to {stem}.events.tsv")
        stems[stem] = p
    outs = {}

    def open_out(stem):
        if stem not in outs:
            outs[stem] = open(os.path.join(args.out_dir, stem + ".events.tsv"), "w")
            outs[stem].write("\t".join(EVENT_COLUMNS) + "\n")
        return outs[stem]

    reads = ((os.path.splitext(os.path.basename(p))[0], r.read_id, r.get_raw_data()) for p in files for r in fast5.iter_reads(p))
    try:
        with Backend(args.device) as be:
            apply_artifacts(args, be, art)
            del art
            for stem in stems:
                open_out(stem)   # a file per input file, also when none of its reads is written
            st = run(args, be, reads, refs, names, open_out)
    finally:
        for f in outs.values():
            f.close()
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
