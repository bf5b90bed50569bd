"""Quantify transcripts from basecalled direct-RNA reads on the GPU: how many molecules of each transcript the run holds.

    python -m radian_amd.quant reads.fasta transcripts.fa[.gz] -o quant.tsv
           [--assign PATH] [--protein-coding | --field N --value S]
           [--k 14] [--w 8] [--max-occ 500] [--min-anchors 3] [--min-score 40] [--max-gap 1000] [--bandwidth 500]
           [--max-cand 16] [--min-frac 0.9] [--max-3p-dist -1] [--weight equal|score] [--max-iter 1000] [--tol 0.001]
           [--device N] [--batch-reads R] [--budget-bytes B]

`map` puts a read on the one transcript with the best chain and breaks ties towards the smaller index; among isoforms that is wrong
for a large part of the reads.  Here every read keeps its candidate transcripts -- the qualifying chains that score at least
--min-frac of the read's best and, with --max-3p-dist >= 0, end at most that many bases before the transcript's 3' end (direct RNA is
sequenced from the 3' end) -- at most --max-cand of them (rd_map_candidates), and an expectation-maximisation over the candidate sets
divides every read among its candidates in proportion to the transcripts' current counts times the candidate's weight (rd_quant_em).
The EM runs in fixed-point integers (units of 2^-20 reads): the files are bit-identical across --batch-reads, --budget-bytes and runs.
One read is one molecule, so there is no length normalisation: est_count estimates molecules, and tpm is count * 10^6 / sum of
counts.  The defaults of --min-frac and --max-3p-dist are conventions of dRNA quantifiers, not calibrated.  One GPU; no CPU path.

  quant.tsv  one header line, then one row per kept transcript in index order: ref_name, length, est_count (six decimals), tpm (three
             decimals), n_unique and n_multi: the single- and multi-candidate reads that name the transcript.
  --assign   one header line, then `read_id status n_qual n_cand ref_name share` per read: the candidate with the largest final share
             (of equal shares the smaller transcript index); `*` and 0 for a read without candidates.
  --weight   equal: every candidate weighs 1; score: w = max(1, score * 4096 // best score of the read).
"""
import argparse
import os
import sys

import numpy as np

from .align import read_fasta
from .backend import MAP_NO_CHAIN, MAP_NO_SEED, MAP_OK, MAP_TOO_LARGE, QUANT_MAX_W, QUANT_ONE, Backend
from .map import Transcripts, encode_read

QUANT_HEADER = "ref_name\tlength\test_count\ttpm\tn_unique\tn_multi\n"
ASSIGN_HEADER = "read_id\tstatus\tn_qual\tn_cand\tref_name\tshare\n"
STATUS_NAMES = {MAP_OK: "ok", MAP_NO_SEED: "no-seed", MAP_NO_CHAIN: "no-chain", MAP_TOO_LARGE: "too-large", -1: "non-ACGT"}


def fmt_q20(v):
    """an integer in units of 2^-20 with six decimals, truncated, by integer arithmetic"""
    v = int(v)
    return f"{v >> 20}.{((v & (QUANT_ONE - 1)) * 10 ** 6) >> 20:06d}"


def fmt_tpm(count, total):
    """count * 10^6 / total with three decimals, truncated, from the integer in 1/1000 units"""
    m = int(count) * 10 ** 9 // int(total) if total else 0
    return f"{m // 1000}.{m % 1000:03d}"


def weights_of(scores, mode):
    """the weights of a read's candidates (scores in candidate order: the first is the best)"""
    if mode == "equal":
        return [1] * len(scores)
    best = int(scores[0])
    return [max(1, int(s) * QUANT_MAX_W // best) for s in scores]


def collect_candidates(be, records, args):
    """records: [(read id, sequence as written)] -> one dict per read in order: id, status (MAP_*, or -1: a letter other than ACGTU),
    n_qual, n_cand, cand: [(t, w)]"""
    frac_q10 = int(round(args.min_frac * 1024))
    rows = []
    for b0 in range(0, len(records), args.batch_reads):
        batch = records[b0: b0 + args.batch_reads]
        codes = [encode_read(seq) for _, seq in batch]
        clean = [i for i, c in enumerate(codes) if not (c > 3).any()]
        res = be.map_candidates([codes[i] for i in clean], args.max_cand, frac_q10, args.max_3p_dist, args.min_anchors, args.min_score, args.max_gap,
                                args.bandwidth, args.budget_bytes, allow_too_large=True)
        out = [dict(id=rid, status=-1, n_qual=0, n_cand=0, cand=[]) for rid, _ in batch]
        for j, i in enumerate(clean):
            n = int(res.n_cand[j])
            w = weights_of(res.cands[j, :n, 1], args.weight) if n else []
            out[i].update(status=int(res.status[j]), n_qual=int(res.n_qual[j]), n_cand=n, cand=[(int(res.cands[j, c, 0]), w[c]) for c in range(n)])
        rows.extend(out)
    return rows


def csr_of(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r["cand"]) for r in rows], out=off[1:])
    flat = [p for r in rows for p in r["cand"]]
    return off, np.array([t for t, _ in flat], dtype=np.int32), np.array([w for _, w in flat], dtype=np.uint16)


def quant_text(tr, rows, count):
    n_unique, n_multi = [0] * len(tr.names), [0] * len(tr.names)
    for r in rows:
        for t, _ in r["cand"]:
            (n_unique if len(r["cand"]) == 1 else n_multi)[t] += 1
    total = sum(int(c) for c in count)
    lines = [QUANT_HEADER]
    for t, name in enumerate(tr.names):
        lines.append(f"{name}\t{tr.length(t)}\t{fmt_q20(count[t])}\t{fmt_tpm(count[t], total)}\t{n_unique[t]}\t{n_multi[t]}\n")
    return "".join(lines)


def assign_text(tr, rows, off, share):
    lines = [ASSIGN_HEADER]
    for i, r in enumerate(rows):
        name, best = "*", 0
        if r["cand"]:
            s = [int(v) for v in share[off[i]: off[i + 1]]]
            j = min(range(len(s)), key=lambda c: (-s[c], r["cand"][c][0]))
            name, best = tr.names[r["cand"][j][0]], s[j]
        lines.append(f"{r['id']}\t{STATUS_NAMES[r['status']]}\t{r['n_qual']}\t{r['n_cand']}\t{name}\t{fmt_q20(best)}\n")
    return "".join(lines)


def summary(tr, index, rows, res):
    why = {name: sum(1 for r in rows if r["status"] == code) for code, name in STATUS_NAMES.items()}
    st = res.stats
    lines = [f"transcripts: {tr.info['records']} read, {tr.info['kept']} kept; bases: {tr.info['bases']}",
             f"minimizers indexed: {index['entries']} on {index['keys']} keys; keys dropped by --max-occ: {index['keys_dropped']}",
             f"reads: {len(rows)} seen (" + ", ".join(f"{k}: {v}" for k, v in why.items()) + ")",
             f"reads with more than one candidate: {sum(1 for r in rows if r['n_cand'] > 1)}; truncated at --max-cand: "
             f"{sum(1 for r in rows if r['n_qual'] > r['n_cand'])}",
             f"EM: {st['iterations']} iterations, last delta {fmt_q20(st['last_delta'])} reads, lost mass {fmt_q20(st['lost'])} reads",
             f"transcripts with a non-zero count: {sum(1 for c in res.count if int(c) > 0)}"]
    return "\n".join(lines) + "\n"


def build_parser():
    ap = argparse.ArgumentParser(prog="quant", description="Estimate the molecules of every transcript from basecalled direct-RNA reads on one GPU.")
    ap.add_argument("fasta", help="basecalled reads (FASTA), 5'->3' as written")
    ap.add_argument("transcripts", help="transcriptome FASTA, 5'->3' as in GENCODE / Ensembl cDNA files (.gz accepted)")
    ap.add_argument("-o", "--output", required=True, help="quant.tsv: ref_name length est_count tpm n_unique n_multi")
    ap.add_argument("--assign", default=None, help="write every read's candidate with the largest final share")
    ap.add_argument("--field", default=None, type=int, help="keep only transcripts whose header, split on |, has --value in this field (0-based)")
    ap.add_argument("--value", default=None, help="see --field")
    ap.add_argument("--protein-coding", action="store_true", help="--field 7 --value protein_coding (GENCODE headers)")
    ap.add_argument("--k", default=14, type=int, help="seed length, 8..15")
    ap.add_argument("--w", default=8, type=int, help="k-mers per minimizer window, 1..64")
    ap.add_argument("--max-occ", default=500, type=int, help="a seed with more index entries than this is not used")
    ap.add_argument("--min-anchors", default=3, type=int, help="least anchors in a chain")
    ap.add_argument("--min-score", default=40, type=int, help="least chain score")
    ap.add_argument("--max-gap", default=1000, type=int, help="largest step between chained anchors, in read and in transcript")
    ap.add_argument("--bandwidth", default=500, type=int, help="largest difference between the two steps")
    ap.add_argument("--max-cand", default=16, type=int, help="candidates kept per read, 1..64")
    ap.add_argument("--min-frac", default=0.9, type=float, help="a candidate scores at least this fraction of the read's best chain (a convention, not calibrated)")
    ap.add_argument("--max-3p-dist", default=-1, type=int, help="a candidate ends at most this many bases before the transcript's 3' end; -1: off (a convention, not calibrated)")
    ap.add_argument("--weight", default="equal", choices=("equal", "score"), help="candidate weights: 1, or the chain score relative to the read's best")
    ap.add_argument("--max-iter", default=1000, type=int, help="EM iterations at most, 0..100000")
    ap.add_argument("--tol", default=0.001, type=float, help="stop when no transcript's count moves by more than this many reads")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--budget-bytes", default=0, type=int, help="anchor workspace per launch of the mapping (0: a quarter of free memory)")
    ap.add_argument("--batch-reads", default=4096, type=int, help="reads per call of the library (the output does not depend on it)")
    return ap


def check_args(args):
    """argument errors, each naming its flag; resolves --protein-coding"""
    if args.protein_coding:
        if args.field is not None or args.value is not None:
            raise SystemExit("quant: --protein-coding is --field 7 --value protein_coding: give one or the other")
        args.field, args.value = 7, "protein_coding"
    if (args.field is None) != (args.value is None):
        raise SystemExit("quant: --field and --value go together")
    if args.field is not None and args.field < 0:
        raise SystemExit("quant: --field counts from 0")
    for flag, lo, hi in (("k", 8, 15), ("w", 1, 64), ("max_occ", 1, None), ("min_anchors", 1, None), ("min_score", 0, None),
                         ("max_gap", 1, (1 << 24) - 1), ("bandwidth", 0, (1 << 24) - 1), ("max_cand", 1, 64), ("min_frac", 0, 1),
                         ("max_3p_dist", -1, None), ("max_iter", 0, 100000), ("tol", 0, None), ("batch_reads", 1, None), ("budget_bytes", 0, None),
                         ("device", 0, None)):
        v = getattr(args, flag)
        if not v >= lo or (hi is not None and v > hi):
            raise SystemExit(f"quant: --{flag.replace('_', '-')} must be {lo}..{hi}" if hi is not None else f"quant: --{flag.replace('_', '-')} must be at least {lo}")
    outs = [p for p in (args.output, args.assign) if p]
    for p in outs:
        if os.path.abspath(p) in (os.path.abspath(args.fasta), os.path.abspath(args.transcripts)):
            raise SystemExit(f"quant: output {p!r} is one of the inputs")
    if len(set(os.path.abspath(p) for p in outs)) != len(outs):
        raise SystemExit("quant: -o and --assign must name different files")
    return args


def main(argv=None):
    args = check_args(build_parser().parse_args(argv))
    for what, path in (("reads", args.fasta), ("transcripts", args.transcripts)):
        if not os.path.exists(path):
            raise SystemExit(f"quant: {what} {path}: no such file")
    try:
        tr = Transcripts.read(args.transcripts, args.field, args.value)
    except ValueError as e:
        raise SystemExit(f"quant: transcripts {e}")
    if tr.info["kept"] == 0:
        raise SystemExit(f"quant: none of the {tr.info['records']} records of {args.transcripts} passes --field {args.field} --value {args.value}"
                         if args.field is not None else f"quant: {args.transcripts} holds no record")
    records = read_fasta(args.fasta)
    with Backend(args.device) as be:
        try:
            index = be.map_index(tr.codes, tr.offsets, args.k, args.w, args.max_occ)
        except Exception as e:
            raise SystemExit(f"quant: {e}")
        rows = collect_candidates(be, records, args)
        off, t, w = csr_of(rows)
        res = be.quant_em(off, t, w, len(tr.names), args.max_iter, int(round(args.tol * QUANT_ONE)), with_share=True)
    with open(args.output, "w") as f:
        f.write(quant_text(tr, rows, res.count))
    if args.assign:
        with open(args.assign, "w") as f:
            f.write(assign_text(tr, rows, off, res.share))
    sys.stdout.write(summary(tr, index, rows, res))
    sys.stdout.flush()
    return rows, res


if __name__ == "__main__":
    main()
    sys.exit(0)
