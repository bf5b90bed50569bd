"""Map basecalled reads onto a transcriptome on the GPU and write the read_ref.tsv that `align` and `label_build` take.

    python -m radian_amd.map reads.fasta transcripts.fa[.gz] -o read_ref.tsv
           [--mapped-fasta PATH] [--paf PATH] [--stats PATH] [--protein-coding | --field N --value S]
           [--k 14] [--w 8] [--max-occ 500] [--min-anchors 3] [--min-score 40] [--max-gap 1000] [--bandwidth 500] [--piece 512]
           [--device N] [--budget-bytes B] [--batch-reads R]

The reference makes this file outside its own tree, with minimap2 against a transcriptome (radian/align.py:62,87; radian/accuracy.py
parses minimap2's SAM).  Here the whole step runs in the HIP library: (w,k)-minimizer seeds of the transcripts in an index on the
device, anchors, chains and the best transcript of every read (rd_map_index, rd_map_batch: the contract is in include/radian_hip.h),
then the ends of the span the read covers by fitting the read's first and last --piece bases into the transcript around the chain's
first and last anchors (rd_fit_batch, align's scores).  Both inputs are read as written, 5'->3', U = T; mapping is forward strand
only (direct RNA has no reverse-strand reads; accuracy.py:30-32 drops them).  One GPU; there is no CPU path.

  read_ref.tsv   one header line, then `read_id <tab> transcript name <tab> span` per mapped read, in input order: the name is the
                 FASTA header up to the first white space, the span the stretch of the transcript the read covers in ACGT, any other
                 letter kept as N.  Unmapped reads are left out.
  --mapped-fasta the reads that mapped, as written (`align` raises the reference's KeyError for a read the TSV does not hold).
  --paf          the twelve PAF columns, forward strand, mapq 255: the read whole (0..length) against the span; column 10 is the chain
                 score capped by the shorter of the two, column 11 the longer of the two; tags s1:i: chain score, s2:i: the best
                 chain score on another transcript, cn:i: anchors in the chain.
  --stats        what radian/accuracy.py reports: `read_id ref_name n_match n_ins n_del n_sub` per mapped read (ref_name = field 0
                 of the name split on `|`, accuracy.py:43-44,70) and its summary lines on stdout (:82-91; the reverse, secondary and
                 supplementary lines print 0).  Deviation: the counts come from a global alignment of the span against the read with
                 align's scores and soft clip (rd_align_batch), not from a SAM CIGAR and NM tag.  accuracy.py:47 counts protein-coding
                 transcripts only: --protein-coding keeps only those in the index, so every mapped read is one.

A read is unmapped when it has a letter other than ACGTU (non-ACGT), no seed on a usable key (no-seed), no chain of --min-anchors
anchors scoring --min-score (no-chain), more anchors than --budget-bytes holds (too-large), or an empty fitted span (empty-span).
The bytes written depend on the inputs and options only -- not on --batch-reads, --budget-bytes or the run.
"""
import argparse
import gzip
import os
import sys
import time

import numpy as np

from . import lm
from .align import rates, read_fasta, summary as rates_summary
from .backend import ALIGN_SCORES, MAP_EMPTY_SPAN, MAP_NO_CHAIN, MAP_NO_SEED, MAP_OK, MAP_TOO_LARGE, Backend

TSV_HEADER = "read_id\ttranscript\tsequence\n"
STATS_HEADER = "read_id\tref_name\tn_match\tn_ins\tn_del\tn_sub\n"
REASONS = {MAP_NO_SEED: "no-seed", MAP_NO_CHAIN: "no-chain", MAP_TOO_LARGE: "too-large", MAP_EMPTY_SPAN: "empty-span", -1: "non-ACGT"}
_CODE = np.full(256, 255, dtype=np.uint8)
for _k, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _letters:
        _CODE[ord(_c)] = _k
_LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


def encode_read(seq):
    """a sequence as written -> codes (A C G T/U = 0..3 in either case, anything else 255)"""
    return _CODE[np.frombuffer(seq.encode("latin-1", "replace"), dtype=np.uint8)]


def fasta_names(path, field=None, value=None):
    """names (the header up to the first white space) of the records rd_fasta_scan keeps: those whose header, split on `|`, has `value` in
    field `field`"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    val = None if value is None else str(value).encode()
    names = []
    for line in raw.split(b"\n"):
        if not line.startswith(b">"):
            continue
        hdr = line[1:].rstrip(b"\r")
        if field is not None:
            cols = hdr.split(b"|")
            if field >= len(cols) or cols[field] != val:
                continue
        tok = hdr.split()
        names.append(tok[0].decode("latin-1") if tok else "")
    return names


class Transcripts:
    """the kept records of a transcriptome FASTA: codes (0..3, 255 = a break), offsets, names"""

    def __init__(self, codes, offsets, names, info=None):
        self.codes, self.offsets, self.names = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.int64), list(names)
        self.info = info or {"records": len(self.names), "kept": len(self.names), "bases": int(self.offsets[-1])}
        if len(self.names) != len(self.offsets) - 1:
            raise ValueError(f"{len(self.names)} names for {len(self.offsets) - 1} records")
        self.fit_codes = np.where(self.codes > 3, 4, self.codes).astype(np.uint8)   # rd_fit_batch's reference codes: 4 matches nothing

    @classmethod
    def read(cls, path, field=None, value=None):
        codes, offsets, info = lm.read_fasta(path, field, value)
        return cls(codes, offsets, fasta_names(path, field, value), info)

    def length(self, t):
        return int(self.offsets[t + 1] - self.offsets[t])

    def fit_slice(self, t, lo, hi):
        o = int(self.offsets[t])
        return self.fit_codes[o + lo: o + hi]

    def letters(self, t, lo, hi):
        return _LETTERS[self.fit_slice(t, lo, hi)].tobytes().decode("ascii")


def pieces(L, n, k, piece, q0, r0, q1, r1):
    """the head and tail of the span rule: ((read lo, read hi, transcript lo, transcript hi) of the head, the same of the tail)"""
    c = max(0, q0 + k - piece)
    hl = q0 + k - c
    head = (c, q0 + k, max(0, r0 + k - 2 * hl), r0 + k)
    te = min(L, q1 + piece)
    tail = (q1, te, r1, min(n, r1 + 2 * (te - q1)))
    return head, tail


def map_records(be, tr, records, args, counters=None):
    """records: [(read id, sequence as written)].  Returns one dict per read, in order: id, seq, status (MAP_*, or -1: a letter other
    than ACGTU), and for MAP_OK t, S, E, score, score2, n_anchors."""
    out = []
    counters = counters if counters is not None else {}
    for name in ("t_map", "t_fit", "anchors", "launches"):
        counters.setdefault(name, 0)
    for b0 in range(0, len(records), args.batch_reads):
        batch = records[b0: b0 + args.batch_reads]
        codes = [encode_read(seq) for _, seq in batch]
        clean = [i for i, c in enumerate(codes) if not (c > 3).any()]
        t0 = time.perf_counter()
        res = be.map_batch([codes[i] for i in clean], args.min_anchors, args.min_score, args.max_gap, args.bandwidth, args.budget_bytes,
                           allow_too_large=True, with_stats=True)
        t1 = time.perf_counter()
        counters["anchors"] += res.stats["anchors"]
        counters["launches"] += res.stats["launches"]
        rows = [{"id": rid, "seq": seq, "status": -1} for rid, seq in batch]
        refs, queries, owner = [], [], []
        for j, i in enumerate(clean):
            row = rows[i]
            row["status"] = int(res.status[j])
            if row["status"] != MAP_OK:
                continue
            t = int(res.t[j])
            row.update(t=t, score=int(res.score[j]), score2=int(res.score2[j]), n_anchors=int(res.n_anchors[j]))
            L, n = len(codes[i]), tr.length(t)
            head, tail = pieces(L, n, args.k, args.piece, int(res.q0[j]), int(res.r0[j]), int(res.q1[j]), int(res.r1[j]))
            for lo, hi, rlo, rhi in (head, tail):
                refs.append(tr.fit_slice(t, rlo, rhi))
                queries.append(codes[i][lo:hi])
            row["_pieces"] = (head, tail)
            owner.append(i)
        if owner:
            fit = be.fit_batch(refs, queries, np.arange(len(queries), dtype=np.int32), ALIGN_SCORES)
            for p, i in enumerate(owner):
                row = rows[i]
                (c, _, w0, _), (q1, te, r1, _) = row.pop("_pieces")
                L, n = len(codes[i]), tr.length(row["t"])
                S = max(0, w0 + int(fit.ref_start[2 * p]) - c)
                E = min(n, r1 + int(fit.ref_end[2 * p + 1]) + (L - q1 - (te - q1)))
                if E <= S:
                    rows[i] = {"id": row["id"], "seq": row["seq"], "status": MAP_EMPTY_SPAN}
                else:
                    row.update(S=S, E=E)
        counters["t_map"] += t1 - t0
        counters["t_fit"] += time.perf_counter() - t1
        out.extend(rows)
    return out


def tsv_row(row, tr):
    return f"{row['id']}\t{tr.names[row['t']]}\t{tr.letters(row['t'], row['S'], row['E'])}\n"


def paf_row(row, tr):
    L, n, span = len(row["seq"]), tr.length(row["t"]), row["E"] - row["S"]
    cols = (row["id"], L, 0, L, "+", tr.names[row["t"]], n, row["S"], row["E"], min(row["score"], L, span), max(L, span), 255,
            f"s1:i:{row['score']}", f"s2:i:{row['score2']}", f"cn:i:{row['n_anchors']}")
    return "\t".join(str(c) for c in cols) + "\n"


def stats_row(row, tr, counts):
    n_match, n_sub, n_ins, n_del = (int(c) for c in counts)
    return f"{row['id']}\t{tr.names[row['t']].split('|')[0]}\t{n_match}\t{n_ins}\t{n_del}\t{n_sub}\n"


def write_outputs(args, tr, rows, be=None):
    """read_ref.tsv and the optional files of the mapped rows.  Returns the text of --stats' summary lines (or "")."""
    mapped = [r for r in rows if r["status"] == MAP_OK]
    with open(args.output, "w") as f:
        f.write(TSV_HEADER)
        for r in mapped:
            f.write(tsv_row(r, tr))
    if args.mapped_fasta:
        with open(args.mapped_fasta, "w") as f:
            for r in mapped:
                f.write(f">{r['id']}\n{r['seq']}\n")
    if args.paf:
        with open(args.paf, "w") as f:
            for r in mapped:
                f.write(paf_row(r, tr))
    if not args.stats:
        return ""
    per_read = []
    with open(args.stats, "w") as f:
        f.write(STATS_HEADER)
        for b0 in range(0, len(mapped), args.batch_reads):
            batch = mapped[b0: b0 + args.batch_reads]
            res = be.align([tr.letters(r["t"], r["S"], r["E"]) for r in batch], [r["seq"].replace("U", "T") for r in batch], ALIGN_SCORES)
            for r, counts, st in zip(batch, res.counts, res.status):
                if st != 0 or int(counts.sum()) == 0:
                    continue   # (the soft clip left nothing to count: align would raise for this read)
                f.write(stats_row(r, tr, counts))
                per_read.append(rates(*(int(c) for c in counts)))
    text = (f"N unmapped reads: {len(rows) - len(mapped)}\nN reverse strand reads: 0\nN secondary reads: 0\nN supplementary reads: 0\n"
            f"N mapped reads: {len(per_read)}\n")
    return text + (rates_summary(per_read) if per_read else "")


def summary(tr, index, rows, counters):
    mapped = [r for r in rows if r["status"] == MAP_OK]
    why = {name: sum(1 for r in rows if r["status"] == code) for code, name in REASONS.items()}
    lines = [f"transcripts: {tr.info['records']} read, {tr.info['kept']} kept; bases: {tr.info['bases']}",
             f"minimizers indexed: {index['entries']} on {index['keys']} keys; keys dropped by --max-occ: {index['keys_dropped']}",
             f"reads: {len(rows)} seen, {len(mapped)} mapped, {len(rows) - len(mapped)} unmapped (" + ", ".join(f"{k}: {v}" for k, v in why.items()) + ")",
             f"ambiguous between transcripts (s2 = s1): {sum(1 for r in mapped if r['score2'] == r['score'])}",
             f"anchors: {counters.get('anchors', 0)} in {counters.get('launches', 0)} launches; seconds: index {counters.get('t_index', 0.0):.2f}, "
             f"map {counters.get('t_map', 0.0):.2f}, fit {counters.get('t_fit', 0.0):.2f}"]
    return "\n".join(lines) + "\n"


def build_parser():
    ap = argparse.ArgumentParser(prog="map", description="Map reads onto transcripts on one GPU and write align's / label_build's read_ref.tsv.")
    ap.add_argument("fasta", help="basecalled reads (FASTA), 5'->3' as written")
    ap.add_argument("transcripts", help="transcriptome FASTA, 5'->3' as in GENCODE / Ensembl cDNA files (.gz accepted)")
    ap.add_argument("-o", "--output", required=True, help="read_ref.tsv: read_id <tab> transcript name <tab> span")
    ap.add_argument("--mapped-fasta", default=None, help="write the reads that mapped (the FASTA `align` takes with the TSV)")
    ap.add_argument("--paf", default=None, help="write the mappings as PAF (tags s1, s2, cn)")
    ap.add_argument("--stats", default=None, help="write radian/accuracy.py's per-read counts and print its summary")
    ap.add_argument("--field", default=None, type=int, help="keep only transcripts whose header, split on |, has --value in this field (0-based)")
    ap.add_argument("--value", default=None, help="see --field")
    ap.add_argument("--protein-coding", action="store_true", help="--field 7 --value protein_coding (GENCODE headers; accuracy.py:47)")
    ap.add_argument("--k", default=14, type=int, help="seed length, 8..15")
    ap.add_argument("--w", default=8, type=int, help="k-mers per minimizer window, 1..64")
    ap.add_argument("--max-occ", default=500, type=int, help="a seed with more index entries than this is not used")
    ap.add_argument("--min-anchors", default=3, type=int, help="least anchors in a chain")
    ap.add_argument("--min-score", default=40, type=int, help="least chain score")
    ap.add_argument("--max-gap", default=1000, type=int, help="largest step between chained anchors, in read and in transcript")
    ap.add_argument("--bandwidth", default=500, type=int, help="largest difference between the two steps")
    ap.add_argument("--piece", default=512, type=int, help="bases of the read's head and tail fitted for the span's ends, 1..1024")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--budget-bytes", default=0, type=int, help="anchor workspace per launch of the mapping (0: a quarter of free memory)")
    ap.add_argument("--batch-reads", default=4096, type=int, help="reads per call of the library (the output does not depend on it)")
    return ap


def check_args(args):
    """argument errors, each naming its flag; resolves --protein-coding"""
    if args.protein_coding:
        if args.field is not None or args.value is not None:
            raise SystemExit("map: --protein-coding is --field 7 --value protein_coding: give one or the other")
        args.field, args.value = 7, "protein_coding"
    if (args.field is None) != (args.value is None):
        raise SystemExit("map: --field and --value go together")
    if args.field is not None and args.field < 0:
        raise SystemExit("map: --field counts from 0")
    for flag, lo, hi in (("k", 8, 15), ("w", 1, 64), ("max_occ", 1, None), ("min_anchors", 1, None), ("min_score", 0, None),
                         ("max_gap", 1, (1 << 24) - 1), ("bandwidth", 0, (1 << 24) - 1), ("piece", 1, 1024), ("batch_reads", 1, None),
                         ("budget_bytes", 0, None), ("device", 0, None)):
        v = getattr(args, flag)
        if v < lo or (hi is not None and v > hi):
            raise SystemExit(f"map: --{flag.replace('_', '-')} must be {lo}..{hi}" if hi is not None else f"map: --{flag.replace('_', '-')} must be at least {lo}")
    outs = [p for p in (args.output, args.mapped_fasta, args.paf, args.stats) if p]
    for p in outs:
        if os.path.abspath(p) in (os.path.abspath(args.fasta), os.path.abspath(args.transcripts)):
            raise SystemExit(f"map: output {p!r} is one of the inputs")
    if len(set(os.path.abspath(p) for p in outs)) != len(outs):
        raise SystemExit("map: -o, --mapped-fasta, --paf and --stats must name different files")
    return args


def main(argv=None):
    args = check_args(build_parser().parse_args(argv))
    for what, path in (("reads", args.fasta), ("transcripts", args.transcripts)):
        if not os.path.exists(path):
            raise SystemExit(f"map: {what} {path}: no such file")
    try:
        tr = Transcripts.read(args.transcripts, args.field, args.value)
    except ValueError as e:
        raise SystemExit(f"map: transcripts {e}")
    if tr.info["kept"] == 0:
        raise SystemExit(f"map: none of the {tr.info['records']} records of {args.transcripts} passes --field {args.field} --value {args.value}"
                         if args.field is not None else f"map: {args.transcripts} holds no record")
    records = read_fasta(args.fasta)
    counters = {}
    with Backend(args.device) as be:
        t0 = time.perf_counter()
        try:
            index = be.map_index(tr.codes, tr.offsets, args.k, args.w, args.max_occ)
        except Exception as e:
            raise SystemExit(f"map: {e}")
        counters["t_index"] = time.perf_counter() - t0
        rows = map_records(be, tr, records, args, counters)
        stats_text = write_outputs(args, tr, rows, be)
    sys.stdout.write(summary(tr, index, rows, counters))
    sys.stdout.write(stats_text)
    sys.stdout.flush()
    return rows


if __name__ == "__main__":
    main()
    sys.exit(0)
