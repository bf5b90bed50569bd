"""Two-sample comparison of event tables, transcript position by transcript position: where does the signal of sample A (e.g. native
RNA) differ from sample B (e.g. in-vitro transcribed, a knock-out, another condition)?  Two directories of `resquiggle` event tables and
the PAFs of `map --paf` in, one TSV out, on one GPU.

    python -m radian_amd.compare --a events_dir_A --a-paf A.paf --b events_dir_B --b-paf B.paf -o sites.tsv
           [--min-depth 10] [--min-q 0] [--channel level|dwell|both] [--alpha 0.05] [--device N] [--budget-bytes B]
           [--split [--split-min-frac 0.1] [--reads-out reads.tsv]]

NO reference behaviour.  Every `*.events.tsv` of the two directories is read in sorted file order (columns read_id, ref_name, ref_pos,
base, n, level, q); the PAFs give every read's transcript, its length and the start of the read's span (columns 1, 6, 7, 8): an event's
transcript position is that start plus ref_pos.  Site ids: the transcripts of both PAFs sorted by name, each at the sum of the lengths
before it.  Refused, naming the offender: a transcript with two lengths, a ref_name that differs from the PAF's, a position beyond its
transcript, two different bases at one site, more than 2^32 - 1 sites or 2^31 - 1 events.  A read that is absent from its PAF is counted
(`no-mapping`) and skipped; events with q < --min-q or a level that is not finite are dropped and counted.

Channels, quantised to int16 on the host: level  clip(rint(level * 1024), -32768, 32767) (1/1024 z unit, clipped at +-32);
dwell  min(n, 32767).  One call of rd_site_compare per channel (integer arithmetic only) gives every site's counts,
sums, order statistics, twice the Mann-Whitney U, the Kolmogorov-Smirnov numerator and the tie term; everything below is fp64 on the host
from those integers only:
  mean, sd (n - 1 form), median per sample;  ks_d = ks_num / (n_a n_b);  ks_p = Q(ks_d sqrt(n_a n_b / (n_a + n_b))), Q the limiting
  Kolmogorov tail;  mwu_z: the normal approximation of U with continuity 0.5 and the tie correction, signed (positive: sample A is
  larger);  mwu_p = erfc(|mwu_z| / sqrt 2);  q: Benjamini-Hochberg over mwu_p of the channel's tested sites, ties ordered by site.

One row per site seen, in site order: ref_name, pos, base, status, n_a, n_b, then per channel mean_a mean_b sd_a sd_b median_a median_b
ks_d ks_p mwu_z mwu_p q (prefixed level_ / dwell_; level columns in z units).  status: ok, low-depth (either sample below --min-depth),
one-sided (one sample has no event), deep (more than 2^20 events: no rank statistics), too-large (does not fit --budget-bytes).  Only
`ok` rows carry test columns; the rest carry nan.  The file is bit-identical across --budget-bytes and runs.

--split adds, per channel, one call of rd_site_split: the threshold on the site's pooled values that splits them
into the two clusters of least within-cluster variance, among cuts that leave each cluster at least --split-min-frac of the events
(min_frac_q16 = rint(frac * 65536)), met exactly in integers.  Each channel's columns gain, fp64 on the host from those integers only:
  cut;  frac_hi_a, frac_hi_b: the share of each sample above the cut (the stoichiometry when the high cluster is the modified one);
  mean_lo, mean_hi of the pooled clusters;  sep = (mean_hi - mean_lo) / the pooled within-cluster sd (N - 2 form; n sumsq - sum^2 in
  Python integers first);  lor: the log odds ratio of the cluster x sample table with 0.5 added to every cell (positive: sample A is
  enriched above the cut);  split_p: the G-test of that table, 1 degree of freedom, erfc(sqrt(G / 2));  split_q: Benjamini-Hochberg
  over split_p of the channel's split sites, ties ordered by site.
Only `ok` rows whose split status is OK carry them (not: every value equal, no cut that meets --split-min-frac, more than 2^16 events).
--reads-out writes rows read_id sample ref_name pos channel value cluster in input order, for every event of a site with split_q <=
--alpha: cluster is value > cut on the quantised value (1: above).  Without --split every byte written and printed is unchanged.

Out of scope: events held anywhere but host memory (about 7 B per event and channel, 4 more with --reads-out); a binary event format;
a soft EM, two-dimensional level x dwell clusters, more than two components; k-mer context and motif calls; more than two samples, or
replicates; pooling neighbouring positions; calibrating any threshold.
THRESHOLDS ARE NOT CALIBRATED: no reads with known modifications were available."""
import argparse
import math
import os
import sys

import numpy as np

from .backend import SITE_DEEP, SITE_OK, SITE_ONE_SIDED, SITE_TOO_LARGE, Backend

CHANNELS = ("level", "dwell")
STAT_COLUMNS = ("mean_a", "mean_b", "sd_a", "sd_b", "median_a", "median_b", "ks_d", "ks_p", "mwu_z", "mwu_p", "q")
SPLIT_COLUMNS = ("cut", "frac_hi_a", "frac_hi_b", "mean_lo", "mean_hi", "sep", "lor", "split_p", "split_q")
ROW_STATUS = ("ok", "low-depth", "one-sided", "deep", "too-large")
DROP_REASONS = ("no-mapping", "low-q", "bad-level")
LEVEL_UNIT = 1024
MAX_SITES, MAX_EVENTS = (1 << 32) - 1, (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ quantisation
def quantise_level(level):
    """levels in z units -> int16 in 1/1024 z unit, round half to even, clipped at the int16 range"""
    return np.clip(np.rint(np.asarray(level, dtype=np.float64) * LEVEL_UNIT), -32768, 32767).astype(np.int16)


def quantise_dwell(n):
    """dwells in samples -> int16, saturated at 32767"""
    return np.minimum(np.asarray(n, dtype=np.int64), 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------ inputs
def read_paf(path):
    """{read id: (transcript, length, target start)} of a PAF (columns 1, 6, 7, 8); a read's first row counts"""
    out = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            cols = line.rstrip("\n").rstrip("\r").split("\t")
            if len(cols) < 9:
                if line.strip():
                    raise SystemExit(f"compare: {path}, line {i + 1}: fewer than 9 PAF columns")
                continue
            try:
                length, start = int(cols[6]), int(cols[7])
            except ValueError:
                raise SystemExit(f"compare: {path}, line {i + 1}: target length / start are not integers")
            if length < 1 or not 0 <= start < length:
                raise SystemExit(f"compare: {path}, line {i + 1}: target start {start} outside the transcript's length {length}")
            out.setdefault(cols[0], (cols[5], length, start))
    return out


def transcript_offsets(pafs):
    """(names sorted, {name: (first site id, length)}, sites in all) over the transcripts of the PAFs"""
    lengths = {}
    for paf in pafs:
        for name, length, _ in paf.values():
            if lengths.setdefault(name, length) != length:
                raise SystemExit(f"compare: transcript {name} has two different lengths in the PAFs ({lengths[name]} and {length})")
    names, offsets, at = sorted(lengths), {}, 0
    for name in names:
        offsets[name] = (at, lengths[name])
        at += lengths[name]
    if at > MAX_SITES:
        raise SystemExit(f"compare: {at} sites in all, more than 2^32 - 1")
    return names, offsets, at


def list_event_files(directory):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(".events.tsv"))


def load_events(paths, paf, offsets, min_q, bases, st, reads=None):
    """the events of one sample: (site uint32, level int16, dwell int16) arrays.  bases: {site: base}, shared by both samples; st: the
    sample's counters.  reads (--reads-out): {"ids": [read ids], "index": [per kept event, its read's place in ids]}, appended to"""
    read_at = {}
    site, level, dwell = [], [], []
    skipped = set()
    for path in paths:
        st["files"] += 1
        with open(path, "r") as f:
            header = f.readline().rstrip("\n").rstrip("\r").split("\t")
            try:
                ix = [header.index(c) for c in ("read_id", "ref_name", "ref_pos", "base", "n", "level", "q")]
            except ValueError:
                raise SystemExit(f"compare: {path}: the header lacks one of read_id, ref_name, ref_pos, base, n, level, q")
            for i, line in enumerate(f):
                cols = line.rstrip("\n").rstrip("\r").split("\t")
                if len(cols) < len(header):
                    if line.strip():
                        raise SystemExit(f"compare: {path}, line {i + 2}: {len(cols)} columns, the header has {len(header)}")
                    continue
                rid, ref_name, ref_pos, base, n, lv, q = (cols[j] for j in ix)
                st["events"] += 1
                if rid not in paf:
                    if rid not in skipped:
                        skipped.add(rid)
                        st["reads-no-mapping"] += 1
                    st["no-mapping"] += 1
                    continue
                tname, tlen, tstart = paf[rid]
                if ref_name != tname:
                    raise SystemExit(f"compare: {path}, line {i + 2}: read {rid} is on {ref_name} here and on {tname} in the PAF")
                pos = tstart + int(ref_pos)
                if not 0 <= pos < tlen:
                    raise SystemExit(f"compare: {path}, line {i + 2}: position {pos} is outside {tname} ({tlen} bases)")
                s = offsets[tname][0] + pos
                if bases.setdefault(s, base) != base:
                    raise SystemExit(f"compare: {path}, line {i + 2}: {tname} position {pos} is {base} here and {bases[s]} elsewhere")
                if int(q) < min_q:
                    st["low-q"] += 1
                    continue
                lv = float(lv)
                if not math.isfinite(lv):
                    st["bad-level"] += 1
                    continue
                if reads is not None:
                    if rid not in read_at:
                        read_at[rid] = len(reads["ids"])
                        reads["ids"].append(rid)
                    reads["index"].append(read_at[rid])
                site.append(s)
                level.append(lv)
                dwell.append(int(n))
    st["kept"] = len(site)
    return np.array(site, dtype=np.uint32), quantise_level(level), quantise_dwell(dwell)


# ------------------------------------------------------------------------------------------------ statistics from the integers
def kolmogorov_tail(lam):
    """Q(lam) = 2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 lam^2), the tail of the limiting Kolmogorov distribution; below lam = 1 through the
    theta-function form 1 - sqrt(2 pi) / lam sum_{k >= 1} exp(-(2k - 1)^2 pi^2 / (8 lam^2)), which converges fast there"""
    if lam <= 0.0:
        return 1.0
    if lam < 1.0:
        s = 0.0
        for k in range(1, 8):
            s += math.exp(-((2 * k - 1) ** 2) * math.pi * math.pi / (8.0 * lam * lam))
        return min(1.0, max(0.0, 1.0 - math.sqrt(2.0 * math.pi) / lam * s))
    s = 0.0
    for k in range(1, 200):
        term = math.exp(-2.0 * k * k * lam * lam)
        s += term if k % 2 else -term
        if term <= 1e-17 * s:
            break
    return min(1.0, max(0.0, 2.0 * s))


def sample_moments(n, s, sq, med2, unit):
    """(mean, sd in the n - 1 form, median) of one sample from its integers, in units of `unit`; nan where they do not exist"""
    n, s, sq = int(n), int(s), int(sq)
    if n == 0:
        return (float("nan"),) * 3
    sd = math.sqrt((n * sq - s * s) / (n * (n - 1))) / unit if n > 1 else float("nan")   # (n sq - s^2 >= 0, exact in Python ints)
    return s / n / unit, sd, int(med2) / 2.0 / unit


def ks_test(ks_num, n0, n1):
    """(ks_d, ks_p)"""
    d = int(ks_num) / (int(n0) * int(n1))
    return d, kolmogorov_tail(d * math.sqrt(int(n0) * int(n1) / (int(n0) + int(n1))))


def mwu_test(u2, tie, n0, n1):
    """(mwu_z, mwu_p): the normal approximation of U = u2 / 2 with continuity correction 0.5 and tie correction; z = 0, p = 1 when every
    value is tied"""
    u2, tie, n0, n1 = int(u2), int(tie), int(n0), int(n1)
    N = n0 + n1
    var = n0 * n1 / 12.0 * ((N + 1) - tie / (N * (N - 1)))
    dev = u2 / 2.0 - n0 * n1 / 2.0
    if var <= 0.0 or dev == 0.0:
        return 0.0, 1.0
    z = (dev - math.copysign(0.5, dev)) / math.sqrt(var)
    return z, min(1.0, math.erfc(abs(z) / math.sqrt(2.0)))


def benjamini_hochberg(ps):
    """q values of the p values in `ps` (a list in site order): ranks by ascending p, ties by position"""
    m = len(ps)
    order = sorted(range(m), key=lambda i: (ps[i], i))
    q, best = [0.0] * m, 1.0
    for rank in range(m, 0, -1):
        i = order[rank - 1]
        best = min(best, ps[i] * m / rank)
        q[i] = best
    return q


def split_stats(n, n_lo, sum_, sum_lo, sumsq, sumsq_lo, cut, unit):
    """[cut, frac_hi_a, frac_hi_b, mean_lo, mean_hi, sep, lor, split_p] of one split site from its integers (pairs: sample 0, 1), in units
    of `unit`.  sep is inf when both clusters have no spread, nan at N = 2"""
    n, n_lo, sum_, sum_lo, sumsq, sumsq_lo = ([int(v[0]), int(v[1])] for v in (n, n_lo, sum_, sum_lo, sumsq, sumsq_lo))
    n_hi = [n[c] - n_lo[c] for c in (0, 1)]
    L, H, N = n_lo[0] + n_lo[1], n_hi[0] + n_hi[1], n[0] + n[1]
    s_lo, q_lo = sum_lo[0] + sum_lo[1], sumsq_lo[0] + sumsq_lo[1]
    s_hi, q_hi = sum_[0] + sum_[1] - s_lo, sumsq[0] + sumsq[1] - q_lo
    mean_lo, mean_hi = s_lo / L / unit, s_hi / H / unit
    w_lo, w_hi = L * q_lo - s_lo * s_lo, H * q_hi - s_hi * s_hi          # n sumsq - sum^2 >= 0, exact in Python ints
    if N <= 2:
        sep = float("nan")
    elif w_lo == 0 and w_hi == 0:
        sep = float("inf")
    else:
        sep = (mean_hi - mean_lo) / (math.sqrt((w_lo / L + w_hi / H) / (N - 2)) / unit)
    lor = math.log((n_hi[0] + 0.5) * (n_lo[1] + 0.5) / ((n_lo[0] + 0.5) * (n_hi[1] + 0.5)))
    g = 0.0
    for obs, row, col in ((n_lo[0], L, n[0]), (n_lo[1], L, n[1]), (n_hi[0], H, n[0]), (n_hi[1], H, n[1])):
        if obs:
            g += 2.0 * obs * math.log(obs * N / (row * col))
    return [int(cut) / unit, n_hi[0] / n[0], n_hi[1] / n[1], mean_lo, mean_hi, sep, lor, min(1.0, math.erfc(math.sqrt(max(g, 0.0) / 2.0)))]


def row_status(status, n0, n1, min_depth):
    if status == SITE_TOO_LARGE:
        return "too-large"
    if status == SITE_ONE_SIDED:
        return "one-sided"
    if n0 < min_depth or n1 < min_depth:
        return "low-depth"
    return "deep" if status == SITE_DEEP else "ok"


def _fmt(v, spec):
    return "nan" if math.isnan(v) else format(v, spec)


def write_table(out, names, offsets, bases, results, min_depth, alpha, splits=None):
    """results: {channel: SiteResult (or anything with its arrays)}, every channel over the same events' sites.  Writes the header and one
    row per site; returns {row status: sites, "significant": {channel: sites with q <= alpha}}.  splits (--split): {channel: SplitResult}
    over the same sites: the SPLIT_COLUMNS follow each channel's, and the return gains "split": {channel: {site: cut of every site with
    split_q <= alpha}}."""
    channels = [c for c in CHANNELS if c in results]
    first = results[channels[0]]
    n_out = len(first.out_site)
    starts = [offsets[name][0] for name in names]
    cols = {}
    status = [row_status(int(first.status[j]), int(first.n[j][0]), int(first.n[j][1]), min_depth) for j in range(n_out)]
    for ch in channels:
        r, unit = results[ch], float(LEVEL_UNIT) if ch == "level" else 1.0
        rows, tested, ps = [], [], []
        for j in range(n_out):
            nan = float("nan")
            n0, n1 = int(r.n[j][0]), int(r.n[j][1])
            if int(r.status[j]) == SITE_TOO_LARGE:
                rows.append([nan] * 11)
                continue
            a = sample_moments(n0, r.sum[j][0], r.sumsq[j][0], r.med2[j][0], unit)
            b = sample_moments(n1, r.sum[j][1], r.sumsq[j][1], r.med2[j][1], unit)
            row = [a[0], b[0], a[1], b[1], a[2], b[2], nan, nan, nan, nan, nan]
            if status[j] == "ok":
                row[6:8] = ks_test(r.ks_num[j], n0, n1)
                row[8:10] = mwu_test(r.u2[j], r.tie[j], n0, n1)
                tested.append(j)
                ps.append(row[9])
            rows.append(row)
        for j, q in zip(tested, benjamini_hochberg(ps)):
            rows[j][10] = q
        cols[ch] = rows
        if splits is not None:
            sp = splits[ch]
            if not np.array_equal(sp.out_site, r.out_site) or not np.array_equal(sp.n, r.n):
                raise SystemExit(f"compare: internal: the split's sites of channel {ch} are not the comparison's")
            tested, ps = [], []
            for j in range(n_out):
                row = [float("nan")] * 9
                if status[j] == "ok" and int(sp.status[j]) == SITE_OK:
                    row[:8] = split_stats(sp.n[j], sp.n_lo[j], sp.sum[j], sp.sum_lo[j], sp.sumsq[j], sp.sumsq_lo[j], sp.cut[j], unit)
                    tested.append(j)
                    ps.append(row[7])
                rows[j] += row
            for j, q in zip(tested, benjamini_hochberg(ps)):
                rows[j][19] = q
    columns = STAT_COLUMNS + (SPLIT_COLUMNS if splits is not None else ())
    out.write("\t".join(["ref_name", "pos", "base", "status", "n_a", "n_b"] + [f"{ch}_{c}" for ch in channels for c in columns]) + "\n")
    st = {s: 0 for s in ROW_STATUS}
    st["significant"] = {ch: 0 for ch in channels}
    if splits is not None:
        st["split"] = {ch: {} for ch in channels}
    t = 0
    for j in range(n_out):
        s = int(first.out_site[j])
        while t + 1 < len(starts) and starts[t + 1] <= s:
            t += 1
        st[status[j]] += 1
        row = [names[t], str(s - starts[t]), bases[s], status[j], str(int(first.n[j][0])), str(int(first.n[j][1]))]
        for ch in channels:
            v = cols[ch][j]
            row += [_fmt(x, ".6f") for x in v[:7]] + [_fmt(v[7], ".6e"), _fmt(v[8], ".4f"), _fmt(v[9], ".6e"), _fmt(v[10], ".6e")]
            if not math.isnan(v[10]) and v[10] <= alpha:
                st["significant"][ch] += 1
            if splits is not None:
                row += [_fmt(x, ".6f") for x in v[11:18]] + [_fmt(v[18], ".6e"), _fmt(v[19], ".6e")]
                if not math.isnan(v[19]) and v[19] <= alpha:
                    st["split"][ch][s] = int(splits[ch].cut[j])
        out.write("\t".join(row) + "\n")
    return st


def summary(sample_st, st, channels, alpha):
    text = ""
    for name in ("a", "b"):
        s = sample_st[name]
        text += f"sample {name.upper()}: {s['files']} files, {s['events']} events read, {s['kept']} kept\n"
        text += "  dropped: " + "; ".join(f"{r}: {s[r]}" for r in DROP_REASONS) + f" ({s['reads-no-mapping']} reads absent from the PAF)\n"
    text += "sites: " + "; ".join(f"{s}: {st[s]}" for s in ROW_STATUS) + "\n"
    for ch in channels:
        text += f"{ch}: {st['significant'][ch]} sites with q <= {alpha:g}\n"
    if "split" in st:
        for ch in channels:
            text += f"{ch} split: {len(st['split'][ch])} sites with split_q <= {alpha:g} (thresholds not calibrated)\n"
    return text


def write_reads(out, names, offsets, reads, site, cond, values, channels, called):
    """--reads-out: one row per event, in input order, and channel whose site is in called[channel] ({site: cut}); cluster 1: value > cut"""
    out.write("read_id\tsample\tref_name\tpos\tchannel\tvalue\tcluster\n")
    starts = [offsets[name][0] for name in names]
    n_rows = 0
    for i in range(len(site)):
        s = int(site[i])
        for ch in channels:
            cut = called[ch].get(s)
            if cut is None:
                continue
            t = int(np.searchsorted(starts, s, side="right")) - 1
            v = int(values[ch][i])
            shown = format(v / LEVEL_UNIT, ".6f") if ch == "level" else str(v)
            out.write(f"{reads['ids'][reads['index'][i]]}\t{'ab'[int(cond[i])]}\t{names[t]}\t{s - starts[t]}\t{ch}\t{shown}\t{int(v > cut)}\n")
            n_rows += 1
    return n_rows


# ------------------------------------------------------------------------------------------------ the command
def build_parser():
    ap = argparse.ArgumentParser(prog="compare", description="Compare two samples' event tables site by site on one GPU: Kolmogorov-Smirnov "
                                 "and Mann-Whitney tests of level and dwell at every transcript position.  Thresholds are NOT calibrated.")
    ap.add_argument("--a", required=True, help="directory of sample A's {stem}.events.tsv files (resquiggle)")
    ap.add_argument("--a-paf", required=True, help="sample A's mappings (map --paf)")
    ap.add_argument("--b", required=True, help="directory of sample B's {stem}.events.tsv files")
    ap.add_argument("--b-paf", required=True, help="sample B's mappings")
    ap.add_argument("-o", "--out", required=True, help="the TSV to write")
    ap.add_argument("--min-depth", default=10, type=int, help="a site is tested when both samples have at least this many events")
    ap.add_argument("--min-q", default=0, type=int, help="events with a quality below this are dropped")
    ap.add_argument("--channel", default="both", choices=["level", "dwell", "both"])
    ap.add_argument("--alpha", default=0.05, type=float, help="the summary counts sites with q at most this")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per launch (0: a quarter of free memory)")
    ap.add_argument("--split", action="store_true", help="also split every site's pooled values into two clusters, exactly: stoichiometry columns")
    ap.add_argument("--split-min-frac", default=0.1, type=float, help="the least share of a site's events either cluster may hold (0 .. 0.5)")
    ap.add_argument("--reads-out", default=None, help="with --split: per-read cluster calls at the sites with split_q at most --alpha")
    return ap


def check_args(args):
    if args.min_depth < 1:
        raise SystemExit("compare: --min-depth must be at least 1")
    if args.min_q < 0:
        raise SystemExit("compare: --min-q must be at least 0")
    if not 0.0 < args.alpha <= 1.0:
        raise SystemExit("compare: --alpha must be in (0, 1]")
    if args.budget_bytes < 0:
        raise SystemExit("compare: --budget-bytes must be at least 0")
    if not 0.0 <= args.split_min_frac <= 0.5:
        raise SystemExit("compare: --split-min-frac must be in 0 .. 0.5")
    if args.reads_out is not None and not args.split:
        raise SystemExit("compare: --reads-out goes with --split")
    for d in (args.a, args.b):
        if not os.path.isdir(d):
            raise SystemExit(f"compare: {d}: no such directory")
    for p in (args.a_paf, args.b_paf):
        if not os.path.isfile(p):
            raise SystemExit(f"compare: {p}: no such file")


def load(args):
    """-> (names, offsets, n_sites, bases, site, cond, {channel: values}, per-sample counters); with --reads-out the counters hold "reads":
    the read ids and every kept event's index into them (uint32)"""
    pafs = {"a": read_paf(args.a_paf), "b": read_paf(args.b_paf)}
    names, offsets, n_sites = transcript_offsets([pafs["a"], pafs["b"]])
    bases, parts, sample_st = {}, [], {}
    reads = {"ids": [], "index": []} if getattr(args, "reads_out", None) else None
    for name, directory in (("a", args.a), ("b", args.b)):
        st = sample_st[name] = {"files": 0, "events": 0, "kept": 0, "reads-no-mapping": 0, **{r: 0 for r in DROP_REASONS}}
        parts.append(load_events(list_event_files(directory), pafs[name], offsets, args.min_q, bases, st, reads))
    if len(parts[0][0]) + len(parts[1][0]) > MAX_EVENTS:
        raise SystemExit(f"compare: {len(parts[0][0]) + len(parts[1][0])} events in all, more than 2^31 - 1")
    site = np.concatenate([parts[0][0], parts[1][0]])
    cond = np.concatenate([np.zeros(len(parts[0][0]), np.uint8), np.ones(len(parts[1][0]), np.uint8)])
    values = {"level": np.concatenate([parts[0][1], parts[1][1]]), "dwell": np.concatenate([parts[0][2], parts[1][2]])}
    if reads is not None:
        sample_st["reads"] = {"ids": reads["ids"], "index": np.array(reads["index"], dtype=np.uint32)}
    return names, offsets, n_sites, bases, site, cond, values, sample_st


def run(args, be, out):
    names, offsets, n_sites, bases, site, cond, values, sample_st = load(args)
    reads = sample_st.pop("reads", None)
    channels = [c for c in CHANNELS if args.channel in (c, "both")]
    results = {ch: be.site_compare(site, cond, values[ch], n_sites, budget_bytes=args.budget_bytes, allow_too_large=True) for ch in channels}
    splits = None
    if args.split:
        q16 = int(np.rint(args.split_min_frac * 65536))
        splits = {ch: be.site_split(site, cond, values[ch], n_sites, min_frac_q16=q16, budget_bytes=args.budget_bytes, allow_too_large=True)
                  for ch in channels}
    st = write_table(out, names, offsets, bases, results, args.min_depth, args.alpha, splits)
    if reads is not None:
        with open(args.reads_out, "w") as f:
            st["read-rows"] = write_reads(f, names, offsets, reads, site, cond, values, channels, st["split"])
    return sample_st, st, channels


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    with Backend(args.device) as be, open(args.out, "w") as out:
        sample_st, st, channels = run(args, be, out)
    sys.stdout.write(summary(sample_st, st, channels, args.alpha))
    sys.stdout.flush()
    return sample_st, st


if __name__ == "__main__":
    main()
