"""Eventalign: puts every read's REFERENCE span on its raw signal against a k-mer PORE MODEL -- a table of the expected level and spread of
every k-mer -- and reports, for every reference base, which samples it sits on and what the current was there.  No signal model and no
weights take part.  fast5, `map`'s read_ref.tsv and a pore-model table in, one event table per input file out, on one GPU.

    python -m radian_amd.eventalign fast5_dir read_ref.tsv -o out_dir (--kmer-table T.tsv [--fill-missing] | --model-seed S --kmer 5)
           [--bounds PATH] [--start-slack 32] [--rescale-rounds 2] [--bg-sd 1.0]
           [--summary PATH] [--kmer-table-out PATH] [--device N] [--batch-reads R] [--budget-bytes B]
           [--events [--w1 4 --t1 2.5 --w2 12 --t2 5.0 --var-floor 1] [--skip-penalty 96 | --no-skips] [--refine]]

NO reference behaviour.  The read's span -- column 3 of read_ref.tsv, reversed into decode order, U = T -- is aligned to the samples by a
Viterbi pass over the states lead, base 1 .. base L, trail (rd_eventalign; the contract is in include/radian_hip.h):
a sample in a base's state costs its squared distance from the k-mer's level over the k-mer's variance plus the log of the spread, a
sample in the lead or the trail the same against a broad background (level 0, --bg-sd).  Every base takes at least one sample; there are
no skips and no dwell prior.  Integer arithmetic throughout; exact to the bit.

The table is a `resquiggle --kmer-table` file as `simulate` reads it, or `simulate`'s STAND-IN from --model-seed.  The stand-in is no pore.

--bounds            a TSV whose header has read_id and tail_end (`polya`'s output, `simulate`'s truth.tsv): the alignment starts at
                    max(0, tail_end - --start-slack).  A read the file lacks, or whose tail_end is negative, starts at 0 and is counted.
                    THE BOUND IS WHAT MAKES THE FIRST BASES RIGHT: without it an early k-mer that happens to match can swallow the tail
                    and the adapter (first-base errors of thousands of samples); the lead state cannot prevent that.
--rescale-rounds    round 0 takes the window's own median and MAD as the scale.  After each round the read's samples in base states are
                    regressed on their bases' model levels (x = alpha + beta l, least squares in exact rational arithmetic from five
                    integer sums) and the read is aligned again on that scale.  The last round's result is written.

{stem}.events.tsv   `resquiggle`'s thirteen columns; level is on the FITTED scale; q = max(0, 50 - floor(10 |level - model level| / model
                    sd)): a base 5 sd off its k-mer gets 0
--summary           as `resquiggle`'s, plus score_per_sample, the fitted m2 and d4 (twice the median, four times the MAD) and the rounds
--kmer-table-out    the table the events imply, as `resquiggle --kmer-table` writes it

A read is `ok`, or is counted and left out: `no-reference`, `has-N`, `signal` (empty, or the MAD of its window is zero) as in
`resquiggle`; `no-path` (fewer samples than bases), `too-long` (more than 2^19 samples in the window), `too-large` (does not fit
--budget-bytes).  Every file is bit-identical across --batch-reads, --budget-bytes and runs.  One GPU; there is no CPU path.

--events [--w1 4 --t1 2.5 --w2 12 --t2 5.0 --var-floor 1] [--skip-penalty 96 | --no-skips]
                    the rows are EVENTS, not samples (rd_eventalign_events): rd_segment (`segment`'s options) cuts
                    the window from t_lo on once, with that window as its scale window, as `sigmap --events` does; round 0 runs on that
                    scale and the refits change the scale alone.  A row is weighted by its event's samples, and the path may jump over
                    one base at a time for --skip-penalty (1/32 nat; 96 = 3 nats).  A skipped base writes no row and is left out of
                    --kmer-table-out; --summary gains the columns rows and skipped; the printed summary adds the events per base and the
                    share of bases skipped.  `no-path` then means fewer than (L + 1) / 2 events (L with --no-skips).  THE STAND-IN IS NO
                    PORE AND THE DEFAULTS COME FROM SIMULATED READS: no sequencer's read took part.  Without --events nothing changes.

--refine            (with --events) after the event rounds every OK read gets ONE pass over SAMPLE rows inside a window of 64 states that
                    follows the event path (rd_eventalign_banded): the scale is the refit of the last event round's
                    sums, the guide that round's event starts.  Where the sample path stays inside the window -- on the simulated reads it
                    strays at most 4 states of the 31 allowed -- the rows are exactly what sample mode writes on that scale: every base
                    has a row, and the scale columns are the pass's.  A read the window loses (`off-band`) or that does not fit the budget
                    keeps its event rows and is counted.  --summary gains refined (1 / 0) and edge (the bases whose rows touch the
                    window's rim) after rows and skipped, which stay the event pass's; the printed summary adds the reads refined, not
                    refined, and with edge > 0.  THE STAND-IN IS NO PORE: no sequencer's read took part.  Without --refine nothing changes.

Out of scope: dwell priors (an HSMM), skips of more than one base, a run-time band width, pooling the rescaling across reads,
conversion to pA, adapter and leader models, per-read modification calls against the table, the pipelined route, several GPUs."""
import argparse
import math
import os
import sys
from fractions import Fraction

import numpy as np

from . import fast5
from .backend import (Backend, EvalModel, EVAL_EMPTY, EVAL_MAD_ZERO, EVAL_NO_PATH, EVAL_OK, EVAL_TOO_LARGE, EVAL_TOO_LONG)
from .fastq import _batches
from .label_build import read_ref_tsv
from .resquiggle import (EVENT_COLUMNS, KmerTable, SUMMARY_COLUMNS as RESQUIGGLE_SUMMARY, _median_of_counts, event_rows, read_ref_names,
                         reference_status)
from .simulate import read_kmer_table, standin_tables

STATUSES = ("ok", "no-reference", "has-N", "no-path", "too-long", "too-large", "signal")
SUMMARY_COLUMNS = RESQUIGGLE_SUMMARY + ("score_per_sample", "m2", "d4", "rounds")
EVENTS_SUMMARY_COLUMNS = ("rows", "skipped")       # --events: the read's events and the bases its path jumped over
REFINE_SUMMARY_COLUMNS = ("refined", "edge")       # --refine: did the banded sample pass replace the event rows; the bases on the window's rim
_EVAL_STATUS = {EVAL_EMPTY: "signal", EVAL_MAD_ZERO: "signal", EVAL_NO_PATH: "no-path", EVAL_TOO_LONG: "too-long", EVAL_TOO_LARGE: "too-large"}
MAD_UNIT = 1.4826 * 256     # model units (MAD / 256) per z
SD_FLOOR = 8                # the least model sd, in MAD / 256
M2_MAX, D4_MAX = 1 << 17, 1 << 20   # the scale rd_eventalign accepts


def model_tables(k, level_q10, sd_q10, bg_sd=1.0):
    """Q10 tables in z (simulate.read_kmer_table / standin_tables) -> the EvalModel, in fp64: lvl = rint(level 1.4826 / 4) (MAD / 256),
    sd_m = max(rint(sd 1.4826 / 4), 8), w = min(rint(16 2^32 / sd_m^2), 2^32 - 1), bias = clip(rint(32 ln(sd_m / bg)), +-256); the
    background has level 0 and sd bg = bg_sd 1.4826 256.  -> (EvalModel, sd_m)"""
    level = np.asarray(level_q10, dtype=np.float64)
    sd = np.asarray(sd_q10, dtype=np.float64)
    bg = float(bg_sd) * MAD_UNIT
    lvl = np.rint(level * 1.4826 / 4)
    sd_m = np.maximum(np.rint(sd * 1.4826 / 4), SD_FLOOR)
    w = np.minimum(np.rint(16.0 * 2.0 ** 32 / (sd_m * sd_m)), 2.0 ** 32 - 1)
    bias = np.clip(np.rint(32.0 * np.log(sd_m / bg)), -256, 256)
    w_bg = min(float(np.rint(16.0 * 2.0 ** 32 / (bg * bg))), 2.0 ** 32 - 1)
    return EvalModel(k, lvl.astype(np.int32), w.astype(np.uint32), bias.astype(np.int32), (0, int(w_bg), 0)), sd_m.astype(np.int32)


def _rnd(q):
    """round half up, exactly"""
    return math.floor(q + Fraction(1, 2))


def refit(sums, m2, d4):
    """the least squares x = alpha + beta l from the five integer sums N, sum l, sum l^2, sum x, sum x l, in exact rational arithmetic ->
    (m2, d4) = (rnd(2 alpha), max(1, rnd(1024 beta))).  A read whose denominator N sum l^2 - (sum l)^2 is not positive, or whose result
    rd_eventalign would refuse, keeps its scale"""
    N, Sl, Sll, Sx, Sxl = (int(v) for v in sums)
    den = N * Sll - Sl * Sl
    if den <= 0:
        return int(m2), int(d4)
    beta = Fraction(N * Sxl - Sl * Sx, den)
    alpha = (Sx - beta * Sl) / N
    nm2, nd4 = _rnd(2 * alpha), max(1, _rnd(1024 * beta))
    if abs(nm2) > M2_MAX or nd4 > D4_MAX:
        return int(m2), int(d4)
    return nm2, nd4


def read_bounds(path):
    """{read id: tail_end} of a TSV whose header has read_id and tail_end (polya.tsv, simulate's truth.tsv)"""
    out = {}
    with open(path, "r") as f:
        header = f.readline().rstrip("\n").rstrip("\r").split("\t")
        if "read_id" not in header or "tail_end" not in header:
            raise SystemExit(f"eventalign: {path}: the header has no read_id and tail_end columns")
        i_id, i_end = header.index("read_id"), header.index("tail_end")
        for n, line in enumerate(f, start=2):
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if not line.strip():
                continue
            try:
                out[cols[i_id]] = int(cols[i_end])
            except (IndexError, ValueError):
                raise SystemExit(f"eventalign: {path}, line {n}: tail_end is not an integer")
    return out


def window_start(read_id, n_samples, bounds, slack):
    """-> (t_lo, bounded): max(0, tail_end - slack), or 0 for a read without a bound"""
    if bounds is None or bounds.get(read_id, -1) < 0:
        return 0, False
    return min(max(0, bounds[read_id] - slack), n_samples), True


def align_rounds(be_align, raws, codes, model, t_lo, rounds):
    """round 0 on the windows' own scales, then `rounds` refits -> the last EvalResult.  be_align(raws, codes, model, t_lo=, m2=, d4=)"""
    res = be_align(raws, codes, model, t_lo=t_lo, m2=None, d4=None)
    for _ in range(rounds):
        m2, d4 = np.zeros(len(raws), np.int32), np.zeros(len(raws), np.int32)   # a read that is not OK is asked again as it was
        for r in range(len(raws)):
            if int(res.status[r]) == EVAL_OK:
                m2[r], d4[r] = refit(res.fit_sums[r], res.m2[r], res.d4[r])
        res = be_align(raws, codes, model, t_lo=t_lo, m2=m2, d4=d4)
    return res


def base_quality(level_m, lvl, sd_m):
    """q of a base whose event has level level_m (MAD / 256, fp64) against its k-mer's lvl and sd_m"""
    return max(0, 50 - int(math.floor(10.0 * abs(level_m - lvl) / sd_m)))


def kmer_indices(codes, k):
    """every base's k-mer index by rd_sim_signal's rule (pore order, first base most significant, the ends repeat)"""
    L, h = len(codes), k // 2
    idx = np.zeros(L, dtype=np.int64)
    for j in range(-h, h + 1):
        idx = idx * 4 + codes[np.clip(np.arange(L) + j, 0, L - 1)].astype(np.int64)
    return idx


def read_rows(rid, name, span, raw, codes, res, r, model, sd_m):
    """the event rows of OK read r of an EvalResult (or, --events, an EvalRowsResult: a skipped base has no samples and writes no row) ->
    (rows, levels, dwells) as resquiggle.event_rows gives them"""
    ev = res.events
    m2, d4 = int(res.m2[r]), int(res.d4[r])
    start, end, s = ev.start[r], ev.end[r], ev.sum[r]
    idx = kmer_indices(codes, model.k)
    qual = np.zeros(len(codes), dtype=np.int64)
    skipped = (end == start) if hasattr(res, "n_skipped") else None
    for b in range(len(codes)):
        if skipped is not None and skipped[b]:
            continue
        mean = float(int(s[b])) / float(int(end[b]) - int(start[b]))
        qual[b] = base_quality((mean - m2 / 2.0) * 1024.0 / d4, int(model.lvl[idx[b]]), int(sd_m[idx[b]]))
    return event_rows(rid, name, span, raw, (start, end, s, ev.sumsq[r], ev.min[r], ev.max[r]), qual, scale=(m2 / 2.0, d4 / 4.0), skipped=skipped)


def events_aligner(seg, align, skip_pen):
    """--events: the be_align of align_rounds over event rows.  seg(windows) -> SegmentResult (segment.window_segmenter) cuts every read's
    window from t_lo on ONCE, at round 0, which runs on that window's own scale; the refits change the scale alone.  align is
    Backend.eventalign_events or eventalign_events_host bound to the budget.  A read the detector could not take keeps that status.
    -> (be_align, cut): cut["ev"] is the batch's SegmentResult once round 0 has run"""
    from .backend import SEGMENT_TOO_LARGE, SEGMENT_TOO_LONG
    cut = {}

    def be_align(raws, codes, mdl, t_lo, m2, d4):
        if "ev" not in cut:
            cut["ev"] = seg([x[t:] for x, t in zip(raws, t_lo)])
        ev = cut["ev"]
        if m2 is None:
            m2, d4 = ev.m2, ev.d4
        else:       # a read that is not OK is asked again as it was: on the window's scale
            m2, d4 = np.where(d4 == 0, ev.m2, m2), np.where(d4 == 0, ev.d4, d4)
        res = align(ev.events, [len(x) - t for x, t in zip(raws, t_lo)], codes, mdl, m2, d4, sample_off=t_lo, skip_pen=skip_pen)
        res.status[ev.status == SEGMENT_TOO_LONG] = EVAL_TOO_LONG
        res.status[ev.status == SEGMENT_TOO_LARGE] = EVAL_TOO_LARGE
        return res

    return be_align, cut


def refine_pass(banded, raws, codes, model, t_lo, res):
    """--refine: one banded sample pass for the OK reads of the last event round `res` (an EvalRowsResult): the scale is the refit of that
    round's sums, the guide its event starts.  banded is Backend.eventalign_banded or eventalign_banded_host bound to the budget.
    -> ({read index: index into the pass's result}, the EvalBandedResult or None)"""
    ok = [r for r in range(len(raws)) if int(res.status[r]) == EVAL_OK]
    if not ok:
        return {}, None
    scale = [refit(res.fit_sums[r], res.m2[r], res.d4[r]) for r in ok]
    fine = banded([raws[r] for r in ok], [codes[r] for r in ok], [res.events.start[r] for r in ok], model, t_lo=[t_lo[r] for r in ok],
                  m2=[m for m, _ in scale], d4=[d for _, d in scale])
    return {r: j for j, r in enumerate(ok)}, fine


def run(args, be, reads, refs, names, bounds, model, sd_m, open_out):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; refs / names: {read id: span} / {read id: transcript name};
    bounds: {read id: tail_end} or None.  Returns the counters."""
    from .segment import params_of, window_segmenter      # (segment imports this module's bounds)
    events = getattr(args, "events", False)
    refine = events and getattr(args, "refine", False)
    st = {"reads": 0, "written": 0, "bases": 0, "unbounded": 0, "dwell": {}, "score_per_sample": [], **{s: 0 for s in STATUSES}}
    if events:
        st.update(rows=0, skipped=0, span_bases=0)
        if refine:
            st.update(refined=0, not_refined=0, edge_reads=0)
        seg = window_segmenter(be.segment, params_of(args), budget_bytes=args.budget_bytes, allow_too_large=True)
    kt = KmerTable(model.k) if args.kmer_table_out else None
    summ = open(args.summary, "w") if args.summary else None
    if summ:
        summ.write("\t".join(SUMMARY_COLUMNS + (EVENTS_SUMMARY_COLUMNS if events else ()) + (REFINE_SUMMARY_COLUMNS if refine else ())) + "\n")

    def done(rid, status, n_samples, ref_len, extra=("-",) * (13 if refine else 11 if events else 9)):
        st[status] += 1
        if summ:
            summ.write("\t".join((rid, status, str(n_samples), str(ref_len)) + tuple(extra)) + "\n")

    def be_align(raws, codes, mdl, **kw):
        return be.eventalign(raws, codes, mdl, budget_bytes=args.budget_bytes, allow_too_large=True, **kw)

    def be_align_rows(*a, **kw):
        return be.eventalign_events(*a, budget_bytes=args.budget_bytes, allow_too_large=True, **kw)

    def be_banded(*a, **kw):
        return be.eventalign_banded(*a, budget_bytes=args.budget_bytes, allow_too_large=True, **kw)

    try:
        for batch in _batches(reads, args.batch_reads):
            st["reads"] += len(batch)
            todo, verdict = [], []
            for stem, rid, raw in batch:
                raw = np.ascontiguousarray(raw, dtype=np.int16)
                status, codes = reference_status(rid, refs)
                if status is None and len(raw) == 0:
                    status = "signal"
                verdict.append((stem, rid, raw, status))
                if status is None:
                    lo, bounded = window_start(rid, len(raw), bounds, args.start_slack)
                    st["unbounded"] += 0 if bounded else 1
                    todo.append((raw, codes, lo))
            cut = {}
            if events:      # the batch's events are cut once; only the scale changes between rounds
                be_align, cut = events_aligner(seg, be_align_rows, args.skip_penalty)
            res = align_rounds(be_align, [t[0] for t in todo], [t[1] for t in todo], model, [t[2] for t in todo], args.rescale_rounds) if todo else None
            where, fine = refine_pass(be_banded, [t[0] for t in todo], [t[1] for t in todo], model, [t[2] for t in todo], res) if refine and todo else ({}, None)
            r = -1
            for stem, rid, raw, status in verdict:
                ref_len = len(refs[rid]) if rid in refs else 0
                if status is not None:
                    done(rid, status, len(raw), ref_len)
                    continue
                r += 1
                e_st = int(res.status[r])
                if e_st != EVAL_OK:
                    done(rid, _EVAL_STATUS[e_st], len(raw), ref_len)
                    continue
                span, codes, lo = refs[rid], todo[r][1], todo[r][2]
                # --refine: a read whose banded pass is OK writes that pass's sample rows on that pass's scale; any other keeps its event rows
                refined = refine and int(fine.status[where[r]]) == EVAL_OK
                src, at = (fine, where[r]) if refined else (res, r)
                rows, levels, dwells = read_rows(rid, names.get(rid, ""), span, raw, codes, src, at, model, sd_m)
                out = open_out(stem)
                for row in rows:
                    out.write("\t".join(row) + "\n")
                st["written"] += 1
                st["bases"] += len(rows)
                for d in dwells:
                    st["dwell"][d] = st["dwell"].get(d, 0) + 1
                score = int(src.score[at])
                sps = score / (len(raw) - lo)
                st["score_per_sample"].append(sps)
                if kt:
                    kt.add(span, levels, dwells)
                if events:
                    dwells = [d for d, lv in zip(dwells, levels) if lv is not None]
                spb = f"{score / len(rows):.6f}" if rows else "nan"
                md = f"{float(np.median(dwells)):.1f}" if dwells else "nan"
                more = ()
                if events:      # the span's first and last sample are those of its first and last base with a row
                    first = min(int(row[4]) for row in rows) if rows else -1
                    last = max(int(row[5]) for row in rows) - 1 if rows else -1
                    n_rows, n_skip = int(cut["ev"].n_events[r]), int(res.n_skipped[r])
                    st["rows"] += n_rows
                    st["skipped"] += n_skip
                    st["span_bases"] += len(codes)
                    more = (str(n_rows), str(n_skip))
                    if refine:
                        edge = int(fine.n_edge[where[r]]) if refined else 0
                        st["refined" if refined else "not_refined"] += 1
                        st["edge_reads"] += 1 if edge else 0
                        more += ("1" if refined else "0", str(edge))
                else:
                    first = int(res.first_step[r][0]) if rows else -1
                    last = int(res.last_step[r][-1]) if rows else -1
                done(rid, "ok", len(raw), ref_len, (str(score), spb, md, str(first), str(last), f"{sps:.6f}", str(int(src.m2[at])), str(int(src.d4[at])),
                                                    str(args.rescale_rounds)) + more)
    finally:
        if summ:
            summ.close()
    if kt:
        kt.write(args.kmer_table_out)
    return st


def summary(st):
    md = _median_of_counts(st["dwell"])
    sps = st["score_per_sample"]
    return (f"reads: {st['reads']} seen, {st['written']} written; without a bound: {st['unbounded']}\n"
            f"bases: {st['bases']}\n"
            + (f"median dwell: {md:.1f} samples\n" if md is not None else "median dwell: -\n")
            + (f"median score per sample: {float(np.median(sps)):.4f}\n" if sps else "median score per sample: -\n")
            + ((f"events per base: {st['rows'] / st['span_bases']:.3f}; bases skipped: {100.0 * st['skipped'] / st['span_bases']:.2f} %\n"
                if st["span_bases"] else "events per base: -; bases skipped: -\n") if "rows" in st else "")
            + (f"refined: {st['refined']}; not refined: {st['not_refined']}; with bases on the band's rim: {st['edge_reads']}\n" if "refined" in st else "")
            + "status: " + "; ".join(f"{s}: {st[s]}" for s in STATUSES) + "\n")


def build_parser():
    from .segment import add_detector_arguments
    ap = argparse.ArgumentParser(prog="eventalign", description="Align every read's reference span to its raw signal against a k-mer pore model "
                                 "on one GPU and write the per-base event table.  Without --kmer-table the pore model is a stand-in and NO pore.")
    ap.add_argument("fast5_dir", help="Directory of single/multi fast5 files.")
    ap.add_argument("read_ref", help="read_ref.tsv as `map` writes it: read_id <tab> transcript name <tab> span, after a header line")
    ap.add_argument("-o", "--out-dir", required=True, help="Directory to output {stem}.events.tsv files (one per input file).")
    ap.add_argument("--kmer-table", default=None, help="the pore model: a `resquiggle --kmer-table` TSV")
    ap.add_argument("--fill-missing", action="store_true", help="k-mers the table lacks take its count-weighted means")
    ap.add_argument("--model-seed", default=None, type=int, help="seed of the stand-in pore model (no --kmer-table)")
    ap.add_argument("--kmer", default=5, type=int, help="k of the stand-in (odd, 1..9)")
    ap.add_argument("--bounds", default=None, help="TSV with read_id and tail_end columns (polya.tsv, truth.tsv): where the transcript body starts")
    ap.add_argument("--start-slack", default=32, type=int, help="samples before tail_end the alignment may start at")
    ap.add_argument("--rescale-rounds", default=2, type=int, help="refits of the read's scale to the model after the first alignment")
    ap.add_argument("--bg-sd", default=1.0, type=float, help="spread of the lead / trail background in z")
    ap.add_argument("--summary", default=None, help="per-read TSV: status, score, dwell, the samples the span covers, the fitted scale")
    ap.add_argument("--kmer-table-out", default=None, help="TSV of the level and dwell of every k-mer of the spans, as `resquiggle --kmer-table`")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per alignment launch (0: a quarter of free memory)")
    ap.add_argument("--events", action="store_true", help="the rows are events (rd_segment), each weighted by its samples, and a base may be "
                    "skipped (rd_eventalign_events); the stand-in is no pore, and no sequencer's read took part in choosing the defaults")
    add_detector_arguments(ap)
    ap.add_argument("--skip-penalty", default=96, type=int, help="--events: the cost of skipping one base, in 1/32 nat (0..256)")
    ap.add_argument("--no-skips", action="store_true", help="--events: no base is skipped")
    ap.add_argument("--refine", action="store_true", help="--events: after the event rounds, one pass over sample rows in a band of 64 states round "
                    "the event path (rd_eventalign_banded); a read whose pass is OK writes sample-mode rows")
    return ap


def build_model(args):
    if args.kmer_table:
        k, level, sd, _ = read_kmer_table(args.kmer_table, args.fill_missing)
    else:
        k = args.kmer
        level, sd, _ = standin_tables(k, args.model_seed)
    return model_tables(k, level, sd, args.bg_sd)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.kmer_table is None) == (args.model_seed is None):
        raise SystemExit("eventalign: give --kmer-table or --model-seed (the stand-in, no pore), not both")
    if args.fill_missing and not args.kmer_table:
        raise SystemExit("eventalign: --fill-missing goes with --kmer-table")
    if args.kmer_table is None and (args.kmer < 1 or args.kmer > 9 or args.kmer % 2 == 0):
        raise SystemExit("eventalign: --kmer must be odd, 1..9")
    if args.batch_reads < 1 or args.budget_bytes < 0 or args.start_slack < 0 or not 0 <= args.rescale_rounds <= 16 or not 0.01 <= args.bg_sd <= 32:
        raise SystemExit("eventalign: --batch-reads at least 1; --budget-bytes and --start-slack at least 0; --rescale-rounds 0..16; --bg-sd 0.01..32")
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"eventalign: {args.fast5_dir}: no such directory")
    if args.refine and not args.events:
        raise SystemExit("eventalign: --refine goes with --events")
    if args.events:
        from .segment import check_detector_arguments
        check_detector_arguments(args, "eventalign")
        if not 0 <= args.skip_penalty <= 256:
            raise SystemExit("eventalign: --skip-penalty must be 0..256")
        if args.no_skips:
            args.skip_penalty = -1
    refs, names = read_ref_tsv(args.read_ref), read_ref_names(args.read_ref)
    bounds = read_bounds(args.bounds) if args.bounds else None
    model, sd_m = build_model(args)
    os.makedirs(args.out_dir, exist_ok=True)
    files = fast5.list_files(args.fast5_dir)
    stems = {}
    for p in files:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise SystemExit(f"eventalign: {p} and {stems[stem]} would both be written to {stem}.events.tsv")
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
            for stem in stems:
                open_out(stem)   # a file per input file, also when none of its reads is written
            st = run(args, be, reads, refs, names, bounds, model, sd_m, open_out)
    finally:
        for f in outs.values():
            f.close()
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
