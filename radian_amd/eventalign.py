"""Eventalign: puts every read's REFERENCE span on its raw signal against a k-mer PORE MODEL -- a table of the expected level and spread of
every k-mer -- and reports, for every reference base, which samples it sits on and what the current was there.  No signal model and no
weights take part.  fast5, `map`'s read_ref.tsv and a pore-model table in, one event table per input file out, on one GPU.

    python -m radian_amd.eventalign fast5_dir read_ref.tsv -o out_dir (--kmer-table T.tsv [--fill-missing] | --model-seed S --kmer 5)
           [--bounds PATH] [--start-slack 32] [--rescale-rounds 2] [--bg-sd 1.0]
           [--summary PATH] [--kmer-table-out PATH] [--device N] [--batch-reads R] [--budget-bytes B]
           [--events [--w1 4 --t1 2.5 --w2 12 --t2 5.0 --var-floor 1] [--skip-penalty 96 | --no-skips] [--refine]]
           [--call SITES.tsv --paf PATH --calls-out PATH [--alt-table ALT.tsv] [--mod-base A] [--call-flank 6] [--call-threshold 0]
            [--call-sites-out PATH]]

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

--call SITES.tsv --paf PATH --calls-out PATH
                    PER-READ MODIFICATION CALLS (rd_modcall).  SITES.tsv: rows ref_name <tab> pos [<tab> level_shift
                    ...] without a header, pos 0-based on the transcript, further columns ignored -- a `simulate --modify` file is one.
                    --paf (`map --paf`, truth.paf) gives the start of every read's span on its transcript, as in `compare`; a read it
                    lacks is counted and gets no jobs, a site outside the read's span makes no job, a ref_name no read maps to is
                    reported.  After a batch's last alignment every (read, site) pair is re-aligned locally on the read's final rows
                    (the refined pass where --refine took, otherwise the last round) and scale: the rows between the first row of the
                    base --call-flank before the replaced states and the last row of the base --call-flank after them, under the
                    canonical states and under the site's alternative ones, by the FORWARD algorithm (the sum over all paths) and by the
                    best path.  The alternative: with --alt-table (a --kmer-table file whose k-mers spell the modified base as M,
                    exactly one each) every base whose k-mer covers the site takes its k-mer's entry with M at the site -- an entry the
                    table lacks, or a k-mer clipped at the span's end, keeps the canonical one and is counted; a site that is not
                    --mod-base is refused; without it the site's own state alone, its level moved by level_shift z.  Each site is tested
                    on its own, the others canonical.  calls.tsv: read_id ref_name pos base status n_states n_rows vit_ref vit_alt fwd_ref
                    fwd_alt llr call, in input read order and then the sites file's; the four values are negative log likelihoods in
                    1/32 nat, llr = (fwd_ref - fwd_alt) / 32 nats, call = 1 where llr > --call-threshold; a job that is not `ok`
                    (`no-anchor`: an anchor base without rows; `no-path`; `too-long`: more than 2^15 rows; `too-large`) carries `-`.
                    --call-sites-out: ref_name pos base n_reads n_ok n_called frac_called mean_llr per site.  THE STAND-IN IS NO PORE,
                    THRESHOLD AND FLANK ARE NOT CALIBRATED, AND NO SEQUENCER'S READ TOOK PART.  Without --call nothing changes.

Out of scope: dwell priors (an HSMM), skips of more than one base, a run-time band width, pooling the rescaling across reads,
conversion to pA, adapter and leader models, the pipelined route, several GPUs; of --call: joint hypotheses over neighbouring sites, dwell
in the likelihood, learning the alt table (EM), calibrating the threshold, sites in the lead or the trail, `resquiggle` tables."""
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
    bg = float(bg_sd) * MAD_UNIT
    lvl, sd_m, w, bias = table_entries(level_q10, sd_q10, bg_sd)
    w_bg = min(float(np.rint(16.0 * 2.0 ** 32 / (bg * bg))), 2.0 ** 32 - 1)
    return EvalModel(k, lvl.astype(np.int32), w.astype(np.uint32), bias.astype(np.int32), (0, int(w_bg), 0)), sd_m.astype(np.int32)


def table_entries(level_q10, sd_q10, bg_sd=1.0):
    """model_tables' formulas on any number of entries -> (lvl, sd_m, w, bias), fp64 arrays of integers"""
    level = np.asarray(level_q10, dtype=np.float64)
    sd = np.asarray(sd_q10, dtype=np.float64)
    bg = float(bg_sd) * MAD_UNIT
    lvl = np.rint(level * 1.4826 / 4)
    sd_m = np.maximum(np.rint(sd * 1.4826 / 4), SD_FLOOR)
    w = np.minimum(np.rint(16.0 * 2.0 ** 32 / (sd_m * sd_m)), 2.0 ** 32 - 1)
    bias = np.clip(np.rint(32.0 * np.log(sd_m / bg)), -256, 256)
    return lvl, sd_m, w, bias


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


# ------------------------------------------------------------------------------------------------ --call: per-read modification calls
CALL_COLUMNS = ("read_id", "ref_name", "pos", "base", "status", "n_states", "n_rows", "vit_ref", "vit_alt", "fwd_ref", "fwd_alt", "llr", "call")
CALL_SITE_COLUMNS = ("ref_name", "pos", "base", "n_reads", "n_ok", "n_called", "frac_called", "mean_llr")


def read_sites(path, need_shift):
    """SITES.tsv: rows ref_name <tab> pos [<tab> level_shift ...], no header -> [(ref_name, pos, level_shift or None)] in the file's order"""
    out = []
    with open(path, "r") as f:
        for n, line in enumerate(f, start=1):
            if not line.strip():
                continue
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            try:
                pos = int(cols[1])
                shift = float(cols[2]) if len(cols) > 2 else None
            except (IndexError, ValueError):
                raise SystemExit(f"eventalign: {path}, line {n}: not ref_name <tab> pos [<tab> level_shift]")
            if pos < 0 or (shift is not None and not math.isfinite(shift)):
                raise SystemExit(f"eventalign: {path}, line {n}: a negative position or a level_shift that is no number")
            if need_shift and shift is None:
                raise SystemExit(f"eventalign: {path}, line {n}: no level_shift column, and no --alt-table to take the modified levels from")
            out.append((cols[0], pos, shift))
    if not out:
        raise SystemExit(f"eventalign: {path} holds no site")
    return out


def read_alt_table(path, k, mod_base):
    """--alt-table: a `resquiggle --kmer-table` file whose k-mers spell the modified base as M, exactly one M each -> {(the pore-order place
    of M in the k-mer, the pore-order index of the k-mer with mod_base for M): (level_q10, sd_q10)}"""
    from .simulate import KMER_COLUMNS, encode
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            if i == 0 or not line.strip():
                continue
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if len(cols) != len(KMER_COLUMNS):
                raise SystemExit(f"eventalign: {path}, line {i + 1}: {len(cols)} columns, not {', '.join(KMER_COLUMNS)}")
            kmer = cols[0]
            if len(kmer) != k:
                raise SystemExit(f"eventalign: {path}, line {i + 1}: a k-mer of {len(kmer)} letters beside a model of k = {k}")
            if kmer.count("M") != 1:
                raise SystemExit(f"eventalign: {path}, line {i + 1}: {kmer} spells the modified base {kmer.count('M')} times, not once")
            try:
                level, sd = float(cols[2]), float(cols[3])
            except ValueError:
                raise SystemExit(f"eventalign: {path}, line {i + 1}: a number does not parse")
            idx = 0
            for c in encode(kmer.replace("M", mod_base), f"{path}: k-mer {kmer}")[::-1]:
                idx = idx * 4 + int(c)
            out[(k - 1 - kmer.index("M"), idx)] = (float(np.clip(np.rint(level * 1024), -(1 << 15), 1 << 15)), float(np.clip(np.rint(sd * 1024), 0, 1 << 15)))
    return out


class Caller:
    """--call: collects a batch's (read, site) jobs from the reads' final alignments, runs them (Backend.modcall) and writes calls.tsv.
    tables: (level_q10, sd_q10) of the canonical model; sites: read_sites'; paf: compare.read_paf's; alt: read_alt_table's or None"""

    def __init__(self, args, model, tables, sites, paf, alt, out):
        from .backend import MC_STATUS_NAMES
        self.args, self.model, self.level, self.sd = args, model, tables[0], tables[1]
        self.sites, self.paf, self.alt, self.out = sites, paf, alt, out
        self.by_name = {}
        for i, (name, _, _) in enumerate(sites):
            self.by_name.setdefault(name, []).append(i)
        self.names = MC_STATUS_NAMES
        self.st = {"jobs": 0, "no_paf": 0, "canonical": 0, "called": 0, "reads": 0, "seen_names": set(), **{s: 0 for s in MC_STATUS_NAMES}}
        self.site_st = [dict(base="-", n_reads=0, n_ok=0, n_called=0, llr=0) for _ in sites]
        self.batch = []     # (rid, raw, codes, m2, d4, first, last, [(site index, base, alt_first, (lvl, w, bias))])
        if out is not None:
            out.write("\t".join(CALL_COLUMNS) + "\n")

    def alt_entries(self, codes, s, shift, what):
        """the replaced states of the site at pore-order base s -> (alt_first, (lvl, w, bias))"""
        k, L = self.model.k, len(codes)
        idx = kmer_indices(codes, k)
        if self.alt is None:
            level = np.clip(np.rint(self.level[idx[s]] + shift * 1024.0), -(1 << 15), 1 << 15)
            lvl, _, w, bias = table_entries([level], [self.sd[idx[s]]], self.args.bg_sd)
            return s, (lvl.astype(np.int32), w.astype(np.uint32), bias.astype(np.int32))
        if "ACGT"[int(codes[s])] != self.args.mod_base:
            raise SystemExit(f"eventalign: --call: {what} is {'ACGT'[int(codes[s])]} on its transcript, not the --mod-base {self.args.mod_base}")
        h = k // 2
        lo, hi = max(0, s - h), min(L - 1, s + h)
        level, sd = [], []
        for b in range(lo, hi + 1):     # base b's k-mer holds the site at pore-order place h - (b - s); a k-mer clipped at the span's end keeps its entry
            e = self.alt.get((h - (b - s), int(idx[b]))) if b - h >= 0 and b + h <= L - 1 else None
            if e is None:
                self.st["canonical"] += 1
                e = (float(self.level[idx[b]]), float(self.sd[idx[b]]))
            level.append(e[0])
            sd.append(e[1])
        lvl, _, w, bias = table_entries(level, sd, self.args.bg_sd)
        return lo, (lvl.astype(np.int32), w.astype(np.uint32), bias.astype(np.int32))

    def check_sites(self, refs):
        """before anything is written: with --alt-table every site a read's span covers must be the --mod-base on it"""
        if self.alt is None:
            return
        for rid, span in refs.items():
            if rid not in self.paf:
                continue
            tname, _, tstart = self.paf[rid]
            for i in self.by_name.get(tname, ()):
                at = self.sites[i][1] - tstart
                if 0 <= at < len(span) and span[at].upper().replace("U", "T") != self.args.mod_base:
                    raise SystemExit(f"eventalign: --call: {tname}:{self.sites[i][1]} is {span[at]} on its transcript (read {rid}), not the --mod-base "
                                     f"{self.args.mod_base}")

    def add(self, rid, span, raw, codes, src, at):
        """an OK read and its final alignment (src, at): an EvalResult, EvalBandedResult or EvalRowsResult"""
        self.st["reads"] += 1
        if rid not in self.paf:
            self.st["no_paf"] += 1
            return
        tname, _, tstart = self.paf[rid]
        self.st["seen_names"].add(tname)
        L = len(codes)
        jobs = []
        for i in self.by_name.get(tname, ()):
            _, pos, shift = self.sites[i]
            if not 0 <= pos - tstart < L:
                continue
            s = L - 1 - (pos - tstart)
            base = "ACGT"[int(codes[s])]
            alt_first, entries = self.alt_entries(codes, s, shift, f"{tname}:{pos}")
            jobs.append((i, base, alt_first, entries))
        if not jobs:
            return
        ev = src.events
        start, end = ev.start[at].astype(np.int64), ev.end[at].astype(np.int64)
        rows = end > start
        first, last = np.where(rows, start, -1).astype(np.int32), np.where(rows, end - 1, -1).astype(np.int32)
        self.batch.append((rid, raw, codes, int(src.m2[at]), int(src.d4[at]), first, last, jobs))

    def flush(self, be):
        """run the batch's jobs and write their rows: input read order, then sites-file order"""
        from .backend import MC_OK
        batch, self.batch = self.batch, []
        if not batch:
            return
        job_read = [r for r, b in enumerate(batch) for _ in b[7]]
        flat = [j for b in batch for j in b[7]]
        res = be.modcall([b[1] for b in batch], [b[2] for b in batch], [b[3] for b in batch], [b[4] for b in batch], [b[5] for b in batch],
                         [b[6] for b in batch], self.model, job_read, [j[2] for j in flat], [j[3] for j in flat], flank=self.args.call_flank,
                         budget_bytes=self.args.budget_bytes, allow_too_large=True)
        for j, (r, (i, base, _, _)) in enumerate(zip(job_read, flat)):
            name, pos, _ = self.sites[i]
            status = int(res.status[j])
            ss = self.site_st[i]
            ss["base"] = base
            ss["n_reads"] += 1
            self.st["jobs"] += 1
            self.st[self.names[status]] += 1
            if status != MC_OK:
                self.out.write("\t".join((batch[r][0], name, str(pos), base, self.names[status]) + ("-",) * 8) + "\n")
                continue
            num = int(res.fwd_ref[j]) - int(res.fwd_alt[j])     # llr = num / 32 nats: exact in fp64, five decimals hold it
            called = num > 32.0 * self.args.call_threshold
            ss["n_ok"] += 1
            ss["n_called"] += int(called)
            ss["llr"] += num
            self.st["called"] += int(called)
            self.out.write("\t".join((batch[r][0], name, str(pos), base, "ok", str(int(res.n_states[j])), str(int(res.n_rows[j])), str(int(res.vit_ref[j])),
                                      str(int(res.vit_alt[j])), str(int(res.fwd_ref[j])), str(int(res.fwd_alt[j])), f"{num / 32.0:.5f}",
                                      "1" if called else "0")) + "\n")

    def write_sites(self, path):
        with open(path, "w") as f:
            f.write("\t".join(CALL_SITE_COLUMNS) + "\n")
            for (name, pos, _), s in zip(self.sites, self.site_st):
                frac = f"{s['n_called'] / s['n_ok']:.6f}" if s["n_ok"] else "nan"
                mean = f"{s['llr'] / (32.0 * s['n_ok']):.6f}" if s["n_ok"] else "nan"
                f.write("\t".join((name, str(pos), s["base"], str(s["n_reads"]), str(s["n_ok"]), str(s["n_called"]), frac, mean)) + "\n")

    def summary(self):
        st = self.st
        unknown = sorted({name for name, _, _ in self.sites} - st["seen_names"])
        ok = st["ok"]
        return (f"calls: {st['jobs']} jobs over {len(self.sites)} sites; " + "; ".join(f"{s}: {st[s]}" for s in self.names) + "\n"
                + f"calls: reads without a PAF line: {st['no_paf']} of {st['reads']}; alt entries kept canonical: {st['canonical']}\n"
                + (f"calls: sites on transcripts no read maps to: {', '.join(unknown)}\n" if unknown else "")
                + (f"calls: called modified: {st['called']} of {ok} ({100.0 * st['called'] / ok:.2f} %)\n" if ok else "calls: called modified: -\n"))


def run(args, be, reads, refs, names, bounds, model, sd_m, open_out, caller=None):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; refs / names: {read id: span} / {read id: transcript name};
    bounds: {read id: tail_end} or None; caller: --call's Caller or None.  Returns the counters."""
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
                if caller is not None:
                    caller.add(rid, span, raw, codes, src, at)
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
            if caller is not None:      # the batch's jobs run after its last alignment, on every read's final source
                caller.flush(be)
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
    ap.add_argument("--call", default=None, metavar="SITES.tsv", help="per-read modification calls at these sites (rd_modcall): rows ref_name <tab> pos "
                    "[<tab> level_shift ...] without a header, pos 0-based on the transcript; a `simulate --modify` file is one.  The stand-in is no "
                    "pore; threshold and flank are not calibrated")
    ap.add_argument("--paf", default=None, help="--call: the reads' mappings (`map --paf`, truth.paf): where each span starts on its transcript")
    ap.add_argument("--calls-out", default=None, help="--call: the per-(read, site) TSV")
    ap.add_argument("--alt-table", default=None, help="--call: the modified k-mers' levels, a --kmer-table file whose k-mers spell the modified base as M "
                    "(exactly one M each); without it the site's own state moves by the sites file's level_shift (z)")
    ap.add_argument("--mod-base", default="A", help="--alt-table: the base M stands for")
    ap.add_argument("--call-flank", default=6, type=int, help="--call: bases either side of the replaced states that are re-aligned (0..27)")
    ap.add_argument("--call-threshold", default=0.0, type=float, help="--call: call = 1 where llr (nats) is above this")
    ap.add_argument("--call-sites-out", default=None, help="--call: a per-site TSV of the reads called")
    return ap


def build_tables(args):
    """-> (k, level_q10, sd_q10) of the pore model the options name"""
    if args.kmer_table:
        k, level, sd, _ = read_kmer_table(args.kmer_table, args.fill_missing)
    else:
        k = args.kmer
        level, sd, _ = standin_tables(k, args.model_seed)
    return k, level, sd


def build_model(args):
    return model_tables(*build_tables(args), args.bg_sd)


def check_call_arguments(args):
    if args.call is None:
        for opt in ("paf", "calls_out", "alt_table", "call_sites_out"):
            if getattr(args, opt) is not None:
                raise SystemExit(f"eventalign: --{opt.replace('_', '-')} goes with --call")
        return
    if args.paf is None or args.calls_out is None:
        raise SystemExit("eventalign: --call takes --paf and --calls-out")
    if not 0 <= args.call_flank <= 27 or not math.isfinite(args.call_threshold):
        raise SystemExit("eventalign: --call-flank 0..27; --call-threshold a number")
    if args.mod_base not in ("A", "C", "G", "T", "U"):
        raise SystemExit("eventalign: --mod-base is one of A C G T U")
    args.mod_base = "T" if args.mod_base == "U" else args.mod_base
    for p in (args.call, args.paf) + ((args.alt_table,) if args.alt_table else ()):
        if not os.path.isfile(p):
            raise SystemExit(f"eventalign: {p}: no such file")


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
    check_call_arguments(args)
    refs, names = read_ref_tsv(args.read_ref), read_ref_names(args.read_ref)
    bounds = read_bounds(args.bounds) if args.bounds else None
    k, level, sd = build_tables(args)
    model, sd_m = model_tables(k, level, sd, args.bg_sd)
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
    caller = None
    if args.call is not None:
        from .compare import read_paf
        alt = read_alt_table(args.alt_table, k, args.mod_base) if args.alt_table else None
        sites, paf = read_sites(args.call, alt is None), read_paf(args.paf)
        Caller(args, model, (level, sd), sites, paf, alt, None).check_sites(refs)
        calls = open(args.calls_out, "w")
        caller = Caller(args, model, (level, sd), sites, paf, alt, calls)
    try:
        with Backend(args.device) as be:
            for stem in stems:
                open_out(stem)   # a file per input file, also when none of its reads is written
            st = run(args, be, reads, refs, names, bounds, model, sd_m, open_out, caller)
    finally:
        for f in list(outs.values()) + ([calls] if caller is not None else []):
            f.close()
    sys.stdout.write(summary(st))
    if caller is not None:
        if args.call_sites_out:
            caller.write_sites(args.call_sites_out)
        sys.stdout.write(caller.summary())
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
