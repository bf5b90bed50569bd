"""Sigmap: assigns every read to a transcript of a PANEL from its raw signal alone, against a k-mer PORE MODEL, and writes the read_ref.tsv
that `eventalign`, `align`, `label_build` and `pileup` take.  No basecall, no signal model and no weights take part.

    python -m radian_amd.sigmap fast5_dir transcripts.fa[.gz] -o read_ref.tsv (--kmer-table T.tsv [--fill-missing] | --model-seed S --kmer 5)
           --bounds PATH [--start-slack 32] [--query-samples 2048] [--tail-pad 8] [--max-cand 8] [--cand-slack 2] [--max-cost 0]
           [--events [--w1 4 --t1 2.5 --w2 12 --t2 5.0 --var-floor 1] [--query-events 256]]
           [--paf PATH] [--summary PATH] [--protein-coding | --field N --value S] [--bg-sd 1.0]
           [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour.  Every kept transcript becomes a TARGET: reversed into the order the pore sees it (3'->5'), U = T, with --tail-pad
A's in front -- the tail the pore sees before the 3' end, so that the first k-mers have their context.  A transcript with a letter outside
ACGTU is skipped and counted.  A state of the panel is a base of a target; its model is the k-mer centred on it within its own target.  The
alignment is the exhaustive subsequence DP of rd_sigmap (the contract is in include/radian_hip.h): eventalign's
cell with a free start and a free end in the reference, no skips and no dwell prior.  Integer arithmetic throughout; exact to the bit.

--bounds     a TSV whose header has read_id and tail_end (`polya`'s output, `simulate`'s truth.tsv).  A read the file lacks, or whose
             tail_end is negative, is `no-bound` and is not mapped: without the bound the query would be the adapter and the tail.
pass 1       the read's first --query-samples samples from t_lo = max(0, tail_end - --start-slack) against the WHOLE panel, on the scale
             (median and MAD) of the samples from t_lo to the read's end; the --max-cand best targets.  Candidates are those whose score
             is within --cand-slack x rows of the best (1/32 nat per sample; UNCALIBRATED).
pass 2       the read's last --query-samples samples (never before t_lo), on pass 1's scale, against every candidate from its pass-1 origin
             state to its target's end.  Transcripts that share their 3' end tie exactly in pass 1; the 5' end of the read tells them apart.
             The read goes to the candidate with the smallest sum of both scores, the smaller transcript index on ties; the candidates
             that tie with it are counted (n_tied).  A read that ends inside what its candidates share stays tied.
--events     the rows of both passes are EVENTS, not samples: rd_segment (`segment`'s options) cuts the samples from
             t_lo on, and a row is an event's mean, floor((2 sum + n) / (2 n)), on the scale of the samples from t_lo on.  Pass 1 takes the
             first --query-events events, pass 2 the last.  One event is one row whatever its length; there are still no skips, so an event
             that merges two bases costs a mismatch.  --cand-slack and --max-cost are per row.  --summary gains the column n_events.
--max-cost   c > 0: a read whose sum exceeds c x the rows of both passes is `unmapped` (1/32 nat per sample; UNCALIBRATED; 0 = off).

read_ref.tsv `map`'s format: one header line, then `read_id <tab> transcript name <tab> span` per mapped read, in input order.  The span runs,
             in transcript orientation, from pass 2's end state to pass 1's origin state, the pad clipped away.
--paf        `map --paf`'s twelve columns, forward strand, mapq 255; the query coordinates are SAMPLES (t_lo .. the read's length), the
             target start is the span's start, so that `compare` reads it with `eventalign`'s tables; tags s1 (the sum of both scores),
             s2 (the best sum on another transcript, -1 without one), cn (candidates), nt (tied candidates).
--summary    per read: status, samples, t_lo, the scale m2 and d4, both scores per sample, transcript, origin and end of the span, n_cand, n_tied.

The table is a `resquiggle --kmer-table` file as `simulate` reads it, or `simulate`'s STAND-IN from --model-seed.  The stand-in is no pore.
The cost is queries x panel states x rows: this maps against a panel, not against a transcriptome of 10^8 bases.  Forward strand,
unspliced, no skips.  A read is `ok`, or is counted and left out: `no-bound`, `signal` (no samples after the bound, or their MAD is zero),
`too-large` (does not fit --budget-bytes), `unmapped`.  Every file is bit-identical across --batch-reads, --budget-bytes and runs.  One GPU;
there is no CPU path."""
import argparse
import os
import sys

import numpy as np

from . import fast5
from .backend import (Backend, SigmapPanel, SEGMENT_OK, SEGMENT_TOO_LARGE, SIGMAP_EMPTY, SIGMAP_MAD_ZERO, SIGMAP_MAX_T, SIGMAP_OK, SIGMAP_TOO_LARGE)
from .eventalign import model_tables, read_bounds, window_start
from .fastq import _batches
from .map import TSV_HEADER, Transcripts
from .segment import add_detector_arguments, check_detector_arguments, event_ends, event_rows, params_of, window_segmenter
from .simulate import read_kmer_table, standin_tables

STATUSES = ("ok", "no-bound", "signal", "too-large", "unmapped")
SUMMARY_COLUMNS = ("read_id", "status", "n_samples", "t_lo", "m2", "d4", "score1_per_sample", "score2_per_sample", "transcript", "span_start",
                   "span_end", "n_cand", "n_tied")
_SM_STATUS = {SIGMAP_EMPTY: "signal", SIGMAP_MAD_ZERO: "signal", SIGMAP_TOO_LARGE: "too-large"}


class Panel:
    """the targets of the kept transcripts: codes / off as rd_sigmap takes them; tr[j]: the transcript of target j; pad"""

    def __init__(self, transcripts, pad):
        self.transcripts, self.pad = transcripts, int(pad)
        self.tr, parts, self.skipped = [], [], 0
        for t in range(len(transcripts.names)):
            c = transcripts.codes[int(transcripts.offsets[t]):int(transcripts.offsets[t + 1])]
            if len(c) == 0 or (c > 3).any():
                self.skipped += 1
                continue
            self.tr.append(t)
            parts.append(np.concatenate([np.zeros(self.pad, np.uint8), c[::-1]]))
        self.off = np.zeros(len(parts) + 1, dtype=np.int64)
        self.off[1:] = np.cumsum([len(p) for p in parts])
        self.codes = np.concatenate(parts) if parts else np.zeros(1, np.uint8)
        self.states = int(self.off[-1])

    def length(self, j):
        """bases of target j's transcript"""
        return int(self.off[j + 1] - self.off[j]) - self.pad

    def span(self, j, org, end):
        """target states org <= end -> [S, E) in transcript orientation, the pad clipped away"""
        L = self.length(j)
        return L - 1 - (max(end, self.pad) - self.pad), L - (max(org, self.pad) - self.pad)


def event_arrays(seg, windows):
    """seg(raws) -> SegmentResult is Backend.segment or segment_host bound to the detector's parameters, with every window as its own scale
    window.  -> (the windows' event rows back to back, the first row of every window, its rows (0: no scale or no events), the result)"""
    ev = seg(windows)
    parts, cnt = [], np.zeros(len(windows), dtype=np.int64)
    for k, x in enumerate(windows):
        if int(ev.status[k]) != SEGMENT_OK or int(ev.d4[k]) == 0:
            continue
        e = ev.events[k]
        parts.append(event_rows(e["sum"], event_ends(e["start"].astype(np.int64), len(x)) - e["start"]))
        cnt[k] = len(parts[-1])
    first = np.zeros(len(windows), dtype=np.int64)
    first[1:] = np.cumsum(cnt)[:-1]
    return (np.concatenate(parts) if parts else np.zeros(1, np.int16)), first, cnt, ev


def map_batch(sig, batch, panel, bounds, args, seg=None):
    """batch: [(read id, raw int16)].  sig(raw, q_lo, q_hi, **kw) -> SigmapResult is Backend.sigmap or sigmap_host bound to the panel and the
    model; seg (--events): see event_arrays.  -> one dict per read: id, status, n, t_lo and, from pass 1 on, m2, d4, T1, T2, s1, s2 (the chosen candidate's scores), j (target), S, E, score, score2
    (the best sum on another target or -1), n_cand, n_tied"""
    Q = args.query_events if seg is not None else args.query_samples
    off = np.zeros(len(batch) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r[1]) for r in batch])
    flat = np.concatenate([np.asarray(r[1], dtype=np.int16) for r in batch]) if off[-1] else np.zeros(1, np.int16)
    rows, todo = [], []
    for i, (rid, raw) in enumerate(batch):
        n = len(raw)
        t_lo, bounded = window_start(rid, n, bounds, args.start_slack)
        rows.append(dict(id=rid, status="ok" if bounded else "no-bound", n=n, t_lo=t_lo))
        if bounded:
            todo.append(i)
    if not todo:
        return rows
    base = np.array([off[i] for i in todo], dtype=np.int64)
    n = np.array([rows[i]["n"] for i in todo], dtype=np.int64)
    lo = np.array([rows[i]["t_lo"] for i in todo], dtype=np.int64)
    if seg is None:      # the rows are the samples [first, first + cnt) of flat
        arr, first, cnt = flat, base + lo, n - lo
        p1 = sig(flat, base + lo, base + np.minimum(n, lo + Q), sc_lo=base + lo, sc_hi=base + n, n_best=args.max_cand)
    else:                # ... the events [first, first + cnt) of arr
        arr, first, cnt, ev = event_arrays(seg, [flat[base[k] + lo[k]:base[k] + n[k]] for k in range(len(todo))])
        p1 = sig(arr, first, first + np.minimum(cnt, Q), m2=ev.m2, d4=ev.d4, n_best=args.max_cand)
    second = []       # (index into todo, target, origin state, pass-1 score)
    for k, i in enumerate(todo):
        row, st = rows[i], int(p1.status[k])
        row.update(m2=int(p1.m2[k]), d4=int(p1.d4[k]))
        if seg is not None:
            row.update(m2=int(ev.m2[k]), d4=int(ev.d4[k]), n_events=int(ev.n_events[k]))
        if st != SIGMAP_OK:
            row["status"] = "too-large" if seg is not None and int(ev.status[k]) == SEGMENT_TOO_LARGE else _SM_STATUS[st]
            continue
        T1 = int(min(cnt[k], Q))
        row["T1"] = T1
        for r in range(args.max_cand):
            if p1.tgt[k, r] >= 0 and p1.score[k, r] <= p1.score[k, 0] + args.cand_slack * T1:
                second.append((k, int(p1.tgt[k, r]), int(p1.org[k, r]), int(p1.score[k, r])))
    if second:
        ks = np.array([s[0] for s in second])
        tg = np.array([s[1] for s in second])
        p2 = sig(arr, first[ks] + np.maximum(0, cnt[ks] - Q), first[ks] + cnt[ks], m2=p1.m2[ks], d4=p1.d4[ks],
                 s_lo=panel.off[tg] + np.array([s[2] for s in second]), s_hi=panel.off[tg + 1], n_best=1)
    per = {}
    for c, (k, j, org, s1) in enumerate(second):
        per.setdefault(k, []).append((c, j, org, s1))
    for k, cands in per.items():
        row = rows[todo[k]]
        T2 = int(min(cnt[k], Q))
        done = sorted((s1 + int(p2.score[c, 0]), j, org, int(p2.end[c, 0]), s1, int(p2.score[c, 0])) for c, j, org, s1 in cands if int(p2.status[c]) == SIGMAP_OK)
        if not done:
            row["status"] = "too-large"
            continue
        total, j, org, end, s1, s2 = done[0]
        S, E = panel.span(j, org, end)
        row.update(T2=T2, s1=s1, s2=s2, j=j, S=S, E=E, score=total, score2=done[1][0] if len(done) > 1 else -1, n_cand=len(done),
                   n_tied=sum(1 for d in done if d[0] == total))
        if args.max_cost > 0 and total > args.max_cost * (row["T1"] + T2):
            row["status"] = "unmapped"
    return rows


def tsv_row(row, panel):
    tr = panel.transcripts
    return f"{row['id']}\t{tr.names[panel.tr[row['j']]]}\t{tr.letters(panel.tr[row['j']], row['S'], row['E'])}\n"


def paf_row(row, panel):
    L, span = panel.length(row["j"]), row["E"] - row["S"]
    cols = (row["id"], row["n"], row["t_lo"], row["n"], "+", panel.transcripts.names[panel.tr[row["j"]]], L, row["S"], row["E"], span, span, 255,
            f"s1:i:{row['score']}", f"s2:i:{row['score2']}", f"cn:i:{row['n_cand']}", f"nt:i:{row['n_tied']}")
    return "\t".join(str(c) for c in cols) + "\n"


def summary_row(row, panel):
    cols = [row["id"], row["status"], row["n"], row["t_lo"], row.get("m2", "-"), row.get("d4", "-")]
    if "j" in row:
        cols += [f"{row['s1'] / row['T1']:.6f}", f"{row['s2'] / row['T2']:.6f}", panel.transcripts.names[panel.tr[row["j"]]], row["S"], row["E"],
                 row["n_cand"], row["n_tied"]]
    else:
        cols += ["-"] * 7
    if "n_events" in row:
        cols.append(row["n_events"])
    return "\t".join(str(c) for c in cols) + "\n"


def run(args, sig, reads, panel, bounds, seg=None):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order.  Writes the files, returns the counters."""
    st = {"reads": 0, "multi": 0, "tied": 0, "per_sample": [], "margin": [], **{s: 0 for s in STATUSES}}
    outs = [open(args.output, "w"), open(args.paf, "w") if args.paf else None, open(args.summary, "w") if args.summary else None]
    try:
        outs[0].write(TSV_HEADER)
        if outs[2]:
            outs[2].write("\t".join(SUMMARY_COLUMNS + (("n_events",) if seg is not None else ())) + "\n")
        for batch in _batches(reads, args.batch_reads):
            st["reads"] += len(batch)
            for row in map_batch(sig, [(rid, raw) for _, rid, raw in batch], panel, bounds, args, seg):
                st[row["status"]] += 1
                if seg is not None and "n_events" not in row:
                    row["n_events"] = "-"
                if outs[2]:
                    outs[2].write(summary_row(row, panel))
                if row["status"] != "ok":
                    continue
                outs[0].write(tsv_row(row, panel))
                if outs[1]:
                    outs[1].write(paf_row(row, panel))
                rows_ = row["T1"] + row["T2"]
                st["multi"] += row["n_cand"] > 1
                st["tied"] += row["n_tied"] > 1
                st["per_sample"].append(row["score"] / rows_)
                if row["score2"] >= 0:
                    st["margin"].append((row["score2"] - row["score"]) / rows_)
    finally:
        for f in outs:
            if f:
                f.close()
    return st


def summary(panel, st):
    tr = panel.transcripts
    med = lambda v: f"{float(np.median(v)):.4f}" if v else "-"
    return (f"transcripts: {tr.info['records']} read, {len(panel.tr)} kept, {panel.skipped} skipped (empty or a letter outside ACGTU)\n"
            f"states: {panel.states}\n"
            f"reads: {st['reads']} seen; " + "; ".join(f"{s}: {st[s]}" for s in STATUSES) + "\n"
            f"reads with more than one candidate: {st['multi']}; tied: {st['tied']}\n"
            f"median score per sample: {med(st['per_sample'])}; median margin per sample: {med(st['margin'])}\n")


def build_parser():
    ap = argparse.ArgumentParser(prog="sigmap", description="Assign every read to a transcript of a panel from its raw signal against a k-mer pore "
                                 "model on one GPU and write read_ref.tsv.  Without --kmer-table the pore model is a stand-in and NO pore.")
    ap.add_argument("fast5_dir", help="Directory of single/multi fast5 files.")
    ap.add_argument("transcripts", help="the panel: a FASTA, plain or gzip")
    ap.add_argument("-o", "--output", required=True, help="read_ref.tsv: read_id <tab> transcript name <tab> span")
    ap.add_argument("--kmer-table", default=None, help="the pore model: a `resquiggle --kmer-table` TSV")
    ap.add_argument("--fill-missing", action="store_true", help="k-mers the table lacks take its count-weighted means")
    ap.add_argument("--model-seed", default=None, type=int, help="seed of the stand-in pore model (no --kmer-table)")
    ap.add_argument("--kmer", default=5, type=int, help="k of the stand-in (odd, 1..9)")
    ap.add_argument("--bounds", required=True, help="TSV with read_id and tail_end columns (polya.tsv, truth.tsv): where the transcript body starts")
    ap.add_argument("--start-slack", default=32, type=int, help="samples before tail_end the first query may start at")
    ap.add_argument("--query-samples", default=2048, type=int, help="samples of either query (1..16384)")
    ap.add_argument("--events", action="store_true", help="the rows are events (rd_segment), not samples; --query-events of them per pass")
    add_detector_arguments(ap)
    ap.add_argument("--query-events", default=256, type=int, help="with --events: events of either query (1..16384)")
    ap.add_argument("--tail-pad", default=8, type=int, help="A's in front of every target")
    ap.add_argument("--max-cand", default=8, type=int, help="targets pass 1 keeps (1..8)")
    ap.add_argument("--cand-slack", default=2.0, type=float, help="a candidate scores within this x rows of the best (1/32 nat per sample; uncalibrated)")
    ap.add_argument("--max-cost", default=0.0, type=float, help="> 0: a read above this x rows of both passes is unmapped (uncalibrated)")
    ap.add_argument("--paf", default=None, help="write the mappings as PAF (tags s1, s2, cn, nt)")
    ap.add_argument("--summary", default=None, help="per-read TSV: status, scale, both scores per sample, transcript, span, candidates")
    ap.add_argument("--field", default=None, type=int, help="keep only transcripts whose header, split on |, has --value in this field (0-based)")
    ap.add_argument("--value", default=None, help="see --field")
    ap.add_argument("--protein-coding", action="store_true", help="--field 7 --value protein_coding (GENCODE headers)")
    ap.add_argument("--bg-sd", default=1.0, type=float, help="the spread the model's log-sd term is taken against, in z")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per launch (0: a quarter of free memory)")
    return ap


def check_args(args):
    if (args.kmer_table is None) == (args.model_seed is None):
        raise SystemExit("sigmap: give --kmer-table or --model-seed (the stand-in, no pore), not both")
    if args.fill_missing and not args.kmer_table:
        raise SystemExit("sigmap: --fill-missing goes with --kmer-table")
    if args.kmer_table is None and (args.kmer < 1 or args.kmer > 9 or args.kmer % 2 == 0):
        raise SystemExit("sigmap: --kmer must be odd, 1..9")
    if args.protein_coding:
        if args.field is not None or args.value is not None:
            raise SystemExit("sigmap: --protein-coding is --field 7 --value protein_coding: give one or the other")
        args.field, args.value = 7, "protein_coding"
    if (args.field is None) != (args.value is None) or (args.field is not None and args.field < 0):
        raise SystemExit("sigmap: --field (from 0) and --value go together")
    if (args.batch_reads < 1 or args.budget_bytes < 0 or args.start_slack < 0 or not 1 <= args.query_samples <= SIGMAP_MAX_T or not 0 <= args.tail_pad <= 64
            or not 1 <= args.max_cand <= 8 or args.cand_slack < 0 or args.max_cost < 0 or not 0.01 <= args.bg_sd <= 32):
        raise SystemExit("sigmap: --batch-reads at least 1; --budget-bytes, --start-slack, --cand-slack and --max-cost at least 0; --query-samples "
                         "1..16384; --tail-pad 0..64; --max-cand 1..8; --bg-sd 0.01..32")
    check_detector_arguments(args, "sigmap")
    if not 1 <= args.query_events <= SIGMAP_MAX_T:
        raise SystemExit("sigmap: --query-events must be 1..16384")
    outs = [p for p in (args.output, args.paf, args.summary) if p]
    if len(set(os.path.abspath(p) for p in outs)) != len(outs):
        raise SystemExit("sigmap: -o, --paf and --summary must name different files")


def build_model(args):
    if args.kmer_table:
        k, level, sd, _ = read_kmer_table(args.kmer_table, args.fill_missing)
    else:
        k = args.kmer
        level, sd, _ = standin_tables(k, args.model_seed)
    return model_tables(k, level, sd, args.bg_sd)[0]


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"sigmap: {args.fast5_dir}: no such directory")
    panel = Panel(Transcripts.read(args.transcripts, args.field, args.value), args.tail_pad)
    if panel.states == 0:
        raise SystemExit(f"sigmap: {args.transcripts}: no transcript is kept")
    if panel.states > 2 ** 31 - 1:
        raise SystemExit(f"sigmap: {panel.states} states, more than 2^31 - 1: this maps against a panel, not a transcriptome")
    bounds = read_bounds(args.bounds)
    model = build_model(args)
    reads = ((os.path.splitext(os.path.basename(p))[0], r.read_id, r.get_raw_data()) for p in fast5.list_files(args.fast5_dir) for r in fast5.iter_reads(p))
    packed = SigmapPanel(panel.codes, panel.off)
    with Backend(args.device) as be:
        def sig(raw, q_lo, q_hi, **kw):
            return be.sigmap(raw, packed, model, q_lo, q_hi, budget_bytes=args.budget_bytes, allow_too_large=True, **kw)
        seg = window_segmenter(be.segment, params_of(args), budget_bytes=args.budget_bytes, allow_too_large=True) if args.events else None
        st = run(args, sig, reads, panel, bounds, seg)
    sys.stdout.write(summary(panel, st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
