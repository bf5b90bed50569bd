"""Event detection: every read's raw signal cut into events, stretches of roughly constant current.  fast5 in, one event table per input
file out, on one GPU.

    python -m radian_amd.segment fast5_dir -o out_dir [--w1 4 --t1 2.5 --w2 12 --t2 5.0 --var-floor 1]
           [--bounds PATH --start-slack 32] [--summary PATH] [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour.  Two sliding Welch t-tests run over the samples, one with a short window (--w1 samples to either side, threshold
--t1 on t) and one with a long window (--w2, --t2; --w2 0 turns it off); a sample is a boundary where t is the largest within a window's
length to either side (ties to the earlier sample), and a boundary of the long test counts only when the short test found none closer
than --w2.  --var-floor is added to every window's variance (in raw units squared), so a flat stretch of quantised signal does not give an
infinite t.  The detection is rd_segment (integer arithmetic only), one call per batch of reads; the thresholds go
in as rint(16 t^2).

--bounds            a TSV whose header has read_id and tail_end (`polya`'s output, `simulate`'s truth.tsv): detection starts at
                    tail_end - --start-slack; samples before it belong to no event.  Without it, or for a read it does not list, sample 0
{stem}.segments.tsv one row per event, reads in input order: read_id idx start end n mean stdv min max src; start / end in the read's
                    samples; mean and stdv fp64 on the host from the integer sums (population form); src 0 for a read's first event,
                    otherwise the test that cut it, 1 or 2
--summary PATH      one row per read: read_id status n_samples n_events median_len; status: ok, empty, too-long (more than 2^30 samples),
                    too-large (does not fit --budget-bytes)
The files are bit-identical across --batch-reads, --budget-bytes and runs.

The defaults were chosen on simulated reads; no read with known boundaries from a sequencer took part."""
import argparse
import os
import sys

import numpy as np

from . import fast5
from .backend import SEGMENT_OK, SEGMENT_STATUS_NAMES, Backend, SegmentParams, segment_th
from .eventalign import read_bounds, window_start
from .fastq import _batches
from .resquiggle import event_moments

COLUMNS = ("read_id", "idx", "start", "end", "n", "mean", "stdv", "min", "max", "src")
SUMMARY_COLUMNS = ("read_id", "status", "n_samples", "n_events", "median_len")


def params_of(args):
    """the integer parameters of rd_segment from the command line's"""
    return SegmentParams(w1=args.w1, w2=args.w2, th1=segment_th(args.t1), th2=segment_th(args.t2), v0=args.var_floor)


def event_rows(sums, ns):
    """the int16 rows `sigmap --events` hands to rd_sigmap: every event's mean floor((2 sum + n) / (2 n)), rounded half up"""
    sums, ns = np.asarray(sums, dtype=np.int64), np.asarray(ns, dtype=np.int64)
    return np.floor_divide(2 * sums + ns, 2 * ns).astype(np.int16)


def event_ends(start, n_samples):
    """an event ends where the next starts, or at the window's last sample"""
    return np.concatenate([start[1:], [n_samples]]).astype(np.int64)


def window_segmenter(segment, params, **kw):
    """seg(windows) -> SegmentResult: `segment` (Backend.segment or segment_host) bound to the detector's parameters, with every window as
    its own scale window -- what `sigmap --events` and `eventalign --events` cut their rows with"""
    return lambda windows: segment(windows, params, [(0, len(x)) for x in windows], **kw)


def read_rows(rid, t_lo, n_window, ev):
    """the rows of one `ok` read whose detection started at sample t_lo"""
    start = ev["start"].astype(np.int64)
    end = event_ends(start, n_window)
    rows = []
    for k in range(len(start)):
        n = int(end[k] - start[k])
        mean, stdv = event_moments(n, int(ev["sum"][k]), int(ev["sumsq"][k]))
        rows.append((rid, str(k), str(int(start[k]) + t_lo), str(int(end[k]) + t_lo), str(n), f"{mean:.4f}", f"{stdv:.4f}", str(int(ev["min"][k])),
                     str(int(ev["max"][k])), str(int(ev["src"][k]))))
    return rows, end - start


def run(args, be, reads, bounds, open_out, summary_out=None):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; open_out(stem) -> the stem's open TSV.  Returns the
    counters."""
    st = {"reads": 0, "events": 0, "samples": 0, "lens": [], **{s: 0 for s in SEGMENT_STATUS_NAMES}}
    p = params_of(args)
    if summary_out is not None:
        summary_out.write("\t".join(SUMMARY_COLUMNS) + "\n")
    for batch in _batches(reads, args.batch_reads):
        st["reads"] += len(batch)
        raws = [np.ascontiguousarray(raw, dtype=np.int16) for _, _, raw in batch]
        lo = [window_start(rid, len(raws[r]), bounds, args.start_slack)[0] for r, (_, rid, _) in enumerate(batch)]
        res = be.segment([x[t:] for x, t in zip(raws, lo)], p, budget_bytes=args.budget_bytes, allow_too_large=True)
        for r, (stem, rid, _) in enumerate(batch):
            status = int(res.status[r])
            st[SEGMENT_STATUS_NAMES[status]] += 1
            out = open_out(stem)
            median = "nan"
            if status == SEGMENT_OK:
                rows, lens = read_rows(rid, lo[r], len(raws[r]) - lo[r], res.events[r])
                for row in rows:
                    out.write("\t".join(row) + "\n")
                st["events"] += len(rows)
                st["samples"] += len(raws[r]) - lo[r]
                st["lens"].append(lens)
                median = f"{float(np.median(lens)):.1f}"
            if summary_out is not None:
                summary_out.write("\t".join((rid, SEGMENT_STATUS_NAMES[status], str(len(raws[r])), str(int(res.n_events[r])), median)) + "\n")
    return st


def summary(st):
    lens = np.concatenate(st["lens"]) if st["lens"] else np.zeros(0)
    return (f"reads: {st['reads']} seen\n"
            + "status: " + "; ".join(f"{s}: {st[s]}" for s in SEGMENT_STATUS_NAMES) + "\n"
            + f"events: {st['events']}\n"
            + (f"events per 1000 samples: {1000.0 * st['events'] / st['samples']:.2f}\n" if st["samples"] else "events per 1000 samples: -\n")
            + (f"median event length: {float(np.median(lens)):.1f}\n" if len(lens) else "median event length: -\n"))


def add_detector_arguments(ap):
    ap.add_argument("--w1", default=4, type=int, help="short window in samples (2..32)")
    ap.add_argument("--t1", default=2.5, type=float, help="threshold on the short test's t")
    ap.add_argument("--w2", default=12, type=int, help="long window in samples (above --w1, at most 64; 0: off)")
    ap.add_argument("--t2", default=5.0, type=float, help="threshold on the long test's t")
    ap.add_argument("--var-floor", default=1, type=int, help="variance added to every window, in raw units squared (1..65536)")


def check_detector_arguments(args, who):
    if not 2 <= args.w1 <= 32 or not (args.w2 == 0 or args.w1 < args.w2 <= 64):
        raise SystemExit(f"{who}: --w1 must be 2..32 and --w2 0 or above --w1 and at most 64")
    for t in (args.t1, args.t2):
        if not (t >= 0 and 16.0 * t * t < 2 ** 32 - 0.5):
            raise SystemExit(f"{who}: --t1 / --t2 must be at least 0 and below 16384")
    if not 1 <= args.var_floor <= 1 << 16:
        raise SystemExit(f"{who}: --var-floor must be 1..65536")


def build_parser():
    ap = argparse.ArgumentParser(prog="segment", description="Cut every read's raw signal into events on one GPU: two sliding t-tests and "
                                 "non-maximum suppression of their statistic.")
    ap.add_argument("fast5_dir", help="Directory of single/multi fast5 files.")
    ap.add_argument("-o", "--out-dir", required=True, help="Directory to output {stem}.segments.tsv files (one per input file).")
    add_detector_arguments(ap)
    ap.add_argument("--bounds", default=None, help="TSV with read_id and tail_end columns (polya.tsv, truth.tsv): where detection starts")
    ap.add_argument("--start-slack", default=32, type=int, help="samples before tail_end that detection starts at")
    ap.add_argument("--summary", default=None, help="write one row per read to this TSV")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per launch (0: a quarter of free memory)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_detector_arguments(args, "segment")
    if args.batch_reads < 1 or args.budget_bytes < 0 or args.start_slack < 0:
        raise SystemExit("segment: --batch-reads must be at least 1, --budget-bytes and --start-slack at least 0")
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"segment: {args.fast5_dir}: no such directory")
    bounds = read_bounds(args.bounds) if args.bounds else None
    paths = fast5.list_files(args.fast5_dir)   # Path.rglob order, as basecall
    stems = {}
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise SystemExit(f"segment: {p} and {stems[stem]} would both be written to {stem}.segments.tsv")
        stems[stem] = p
    os.makedirs(args.out_dir, exist_ok=True)
    outs = {}

    def open_out(stem):
        if stem not in outs:
            outs[stem] = open(os.path.join(args.out_dir, stem + ".segments.tsv"), "w")
            outs[stem].write("\t".join(COLUMNS) + "\n")
        return outs[stem]

    def reads():
        for path in paths:
            src = fast5.Fast5Source(path)
            stem = os.path.splitext(os.path.basename(path))[0]
            open_out(stem)   # a file without reads still gets its header
            try:
                for _, r in src.reads(0, src.n_reads()):
                    yield stem, r.read_id, r.get_raw_data()
            finally:
                src.close()

    summary_out = open(args.summary, "w") if args.summary else None
    try:
        with Backend(args.device) as be:
            st = run(args, be, reads(), bounds, open_out, summary_out)
    finally:
        for f in outs.values():
            f.close()
        if summary_out is not None:
            summary_out.close()
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
