"""Poly(A) tail estimation: the longest flat, low-variance stretch of every read's raw signal, and its length in nucleotides.  fast5
in, one TSV out, on one GPU.

    python -m radian_amd.polya fast5_dir -o polya.tsv [--moves moves.tsv | --samples-per-base R]
           [--window 32] [--flat-sd 0.12] [--level-lo Z --level-hi Z] [--max-gap 2] [--min-samples 480]
           [--search-limit 0] [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour.  A homopolymer of 30-250 A collapses in any CTC decode, so the tail cannot be read from the bases: it is
measured on the raw samples.  Every read is cut into windows of --window samples; a window is FLAT when its standard deviation is at
most --flat-sd in mad_normalise's z units (and, with --level-lo / --level-hi, its mean lies in that band of z); flat windows at most
--max-gap non-flat windows apart form a segment; the longest segment of at least --min-samples samples (starting before --search-limit,
if given) is the tail.  The search is rd_polya_segment (integer arithmetic only), one call per batch of reads.

One row per read, in input order: read_id, status, n_samples, tail_start, tail_end (samples [start, end)), tail_samples, level and spread
(the segment's mean and standard deviation in z units: fp64 on the host from the integer sums, the median and the MAD),
samples_per_base, tail_nt = tail_samples / samples_per_base, n_candidates.  The rate is --samples-per-base, or comes from --moves (the
file `python -m radian_amd.fastq --moves` writes): (max_sample - tail_end) / n_bases over the bases whose first sample is at or after
tail_end, at least 8 of them; otherwise, and with neither option, both columns are nan.  A read that is missing from the moves file gets
nan and is counted.  status: ok, none (no segment long enough), mad-zero, short (fewer than --window samples), empty, too-large (does not
fit --budget-bytes).  The file is bit-identical across --batch-reads, --budget-bytes and runs.

THE DEFAULTS ARE NOT CALIBRATED: no read with a known tail was available when they were chosen."""
import argparse
import math
import os
import sys

import numpy as np

from . import fast5
from .backend import POLYA_OK, POLYA_STATUS_NAMES, Backend, PolyaParams, polya_q
from .fastq import _batches
from .resquiggle import event_level, event_moments

COLUMNS = ("read_id", "status", "n_samples", "tail_start", "tail_end", "tail_samples", "level", "spread", "samples_per_base", "tail_nt",
           "n_candidates")
MIN_RATE_BASES = 8


def params_of(args):
    """the integer parameters of rd_polya_segment from the command line's z units"""
    use_level = args.level_lo is not None or args.level_hi is not None
    lo = polya_q(args.level_lo) if args.level_lo is not None else -(1 << 20)
    hi = polya_q(args.level_hi) if args.level_hi is not None else (1 << 20)
    return PolyaParams(win=args.window, flat_q=polya_q(args.flat_sd), use_level=int(use_level), lo_q=lo if use_level else 0,
                       hi_q=hi if use_level else 0, max_gap=args.max_gap, min_samples=args.min_samples, search_limit=args.search_limit)


def segment_level(n, s, sq, m2, d4):
    """(level, spread) of a segment of n samples in mad_normalise's z units from the integers: mean and population sd (resquiggle's
    event_moments), median = m2 / 2, MAD = d4 / 4"""
    mean, sd = event_moments(n, s, sq)
    mad = d4 / 4.0
    return event_level(mean, m2 / 2.0, mad), sd / (1.4826 * mad)


def read_moves(path):
    """{read id: (first_step, last_step) int64 arrays} of `fastq --moves`' file"""
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if i == 0 or len(cols) != 4:
                continue
            first = np.array([int(v) for v in cols[2].split(",") if v], dtype=np.int64)
            last = np.array([int(v) for v in cols[3].split(",") if v], dtype=np.int64)
            if first.shape != last.shape:
                raise SystemExit(f"polya: {path}, line {i + 1}: first_step and last_step differ in length")
            out[cols[0]] = (first, last)
    return out


def moves_rate(first, last, tail_end):
    """samples per base behind the tail: (max_sample - tail_end) / n_bases over the bases whose first sample is >= tail_end (max_sample: one
    past the last sample any of them sits on); nan with fewer than MIN_RATE_BASES of them"""
    first, last = np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64)
    sel = first >= tail_end
    n = int(sel.sum())
    if n < MIN_RATE_BASES:
        return float("nan")
    return (int(last[sel].max()) + 1 - int(tail_end)) / n


def _fmt(v, spec):
    return "nan" if isinstance(v, float) and math.isnan(v) else format(v, spec)


def run(args, be, reads, out, moves=None):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; out: the open TSV (the header is written here).
    Returns the counters."""
    st = {"reads": 0, "no-moves": 0, "tail_samples": [], "tail_nt": [], **{s: 0 for s in POLYA_STATUS_NAMES}}
    p = params_of(args)
    out.write("\t".join(COLUMNS) + "\n")
    for batch in _batches(reads, args.batch_reads):
        st["reads"] += len(batch)
        raws = [np.ascontiguousarray(raw, dtype=np.int16) for _, _, raw in batch]
        res = be.polya_segment(raws, p, budget_bytes=args.budget_bytes, allow_too_large=True)
        for r, (_, rid, _) in enumerate(batch):
            status = int(res.status[r])
            st[POLYA_STATUS_NAMES[status]] += 1
            row = [rid, POLYA_STATUS_NAMES[status], str(len(raws[r]))]
            if status != POLYA_OK:
                out.write("\t".join(row + ["-1", "-1", "0", "nan", "nan", "nan", "nan", "0"]) + "\n")
                continue
            a, e = int(res.tail_start[r]), int(res.tail_end[r])
            level, spread = segment_level(e - a, int(res.sum[r]), int(res.sumsq[r]), int(res.m2[r]), int(res.d4[r]))
            rate = float("nan")
            if args.samples_per_base is not None:
                rate = float(args.samples_per_base)
            elif moves is not None:
                if rid in moves:
                    rate = moves_rate(*moves[rid], e)
                else:
                    st["no-moves"] += 1
            nt = (e - a) / rate if not math.isnan(rate) else float("nan")
            st["tail_samples"].append(e - a)
            if not math.isnan(nt):
                st["tail_nt"].append(nt)
            out.write("\t".join(row + [str(a), str(e), str(e - a), f"{level:.6f}", f"{spread:.6f}", _fmt(rate, ".4f"), _fmt(nt, ".2f"),
                                       str(int(res.n_candidates[r]))]) + "\n")
    return st


def summary(st):
    ts, nt = st["tail_samples"], st["tail_nt"]
    return (f"reads: {st['reads']} seen\n"
            + "status: " + "; ".join(f"{s}: {st[s]}" for s in POLYA_STATUS_NAMES) + "\n"
            + (f"median tail_samples: {float(np.median(ts)):.1f}\n" if ts else "median tail_samples: -\n")
            + (f"median tail_nt: {float(np.median(nt)):.2f}\n" if nt else "median tail_nt: -\n")
            + (f"reads missing from the moves file: {st['no-moves']}\n" if st["no-moves"] else ""))


def build_parser():
    ap = argparse.ArgumentParser(prog="polya", description="Estimate every read's poly(A) tail on one GPU: the longest flat stretch of the raw "
                                 "signal, converted to nucleotides with the read's own translocation rate.  The defaults are NOT calibrated.")
    ap.add_argument("fast5_dir", help="Directory of single/multi fast5 files.")
    ap.add_argument("-o", "--out", required=True, help="the TSV to write")
    rate = ap.add_mutually_exclusive_group()
    rate.add_argument("--moves", default=None, help="`fastq --moves`' TSV: the rate is taken from the bases behind each read's tail")
    rate.add_argument("--samples-per-base", default=None, type=float, help="a fixed translocation rate in samples per base")
    ap.add_argument("--window", default=32, type=int, help="window length in samples (8..256)")
    ap.add_argument("--flat-sd", default=0.12, type=float, help="a window is flat when its sd is at most this, in mad_normalise's z units")
    ap.add_argument("--level-lo", default=None, type=float, help="with --level-hi: a flat window's mean must lie in this band of z")
    ap.add_argument("--level-hi", default=None, type=float)
    ap.add_argument("--max-gap", default=2, type=int, help="non-flat windows tolerated inside a segment (0..1024)")
    ap.add_argument("--min-samples", default=480, type=int, help="minimum segment length in samples")
    ap.add_argument("--search-limit", default=0, type=int, help="a segment must start before this sample (0: anywhere)")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per launch (0: a quarter of free memory)")
    return ap


def check_args(args):
    if not 8 <= args.window <= 256:
        raise SystemExit("polya: --window must be 8..256")
    if not 1 <= polya_q(args.flat_sd) <= 32767:
        raise SystemExit("polya: --flat-sd must be positive and at most 86 (1..32767 in units of MAD / 256)")
    for z in (args.level_lo, args.level_hi):
        if z is not None and abs(polya_q(z)) > 1 << 20:
            raise SystemExit("polya: --level-lo / --level-hi are out of range")
    if args.level_lo is not None and args.level_hi is not None and args.level_lo > args.level_hi:
        raise SystemExit("polya: --level-lo is above --level-hi")
    if not 0 <= args.max_gap <= 1024:
        raise SystemExit("polya: --max-gap must be 0..1024")
    if args.min_samples < args.window or args.search_limit < 0:
        raise SystemExit("polya: --min-samples must be at least --window and --search-limit at least 0")
    if args.samples_per_base is not None and not args.samples_per_base > 0:
        raise SystemExit("polya: --samples-per-base must be positive")
    if args.batch_reads < 1 or args.budget_bytes < 0:
        raise SystemExit("polya: --batch-reads must be at least 1 and --budget-bytes at least 0")


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"polya: {args.fast5_dir}: no such directory")
    moves = read_moves(args.moves) if args.moves else None

    def reads():
        for path in fast5.list_files(args.fast5_dir):   # Path.rglob order, as basecall
            src = fast5.Fast5Source(path)
            try:
                for _, r in src.reads(0, src.n_reads()):
                    yield os.path.splitext(os.path.basename(path))[0], r.read_id, r.get_raw_data()
            finally:
                src.close()

    with Backend(args.device) as be, open(args.out, "w") as out:
        st = run(args, be, reads(), out, moves)
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
