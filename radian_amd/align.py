"""Drop-in for radian/align.py: read accuracy of a basecalled FASTA against per-read reference sequences, aligned on the MI355X.

    python -m radian_amd.align reads.fasta read_ref.tsv [--out PATH] [--device N] [--budget-bytes B] [--dump-alignments PATH]

Same positional arguments, output and stdout as radian/align.py:59-109: the TSV's first line is skipped and every other line is
`read, txt, seq` (tab separated; a later id overrides an earlier one); each FASTA record's sequence, with upper-case U replaced by T,
is aligned globally against its read's reference sequence with pairwise2.align.globalms(ref, seq, 2, -4, -4, -2) semantics
(byte equality, a gap of length L costs -4 - 2 (L - 1), end gaps penalised); analyse_alignment's soft clip and counts give the
per-read line `read_id n_match n_ins n_del n_sub` of `fasta.replace(".fasta", ".tsv")`, and the five summary lines (median / mean
of accuracy, insertion, deletion, substitution and total error rates in percent) are printed as the reference prints them.
The alignment, clip and counts run in the HIP library (rd_align_batch, align.hip); there is no CPU fallback.

What differs (documented deviations):
  - the reference takes one of the co-optimal alignments at random (random.choice, align.py:89); here the traceback's tie-break is
    fixed -- diagonal, then deletion (ref base against a read gap), then insertion; inside a gap run extending before closing --
    so a run is deterministic.  The score is always the optimum; where the optimal alignment is unique the counts are the
    reference's;
  - every read id is looked up in the TSV before anything is aligned or written: a missing id raises the reference's KeyError
    and leaves no partial TSV;
  - an output path equal to the FASTA's (a name without ".fasta") is refused instead of overwriting the FASTA;
  - the reference's IndexError (the soft clip running past the end of an alignment, align.py:33,39) and ZeroDivisionError (no
    counted column left after the clip, align.py:93) name the read.  As in the reference, the lines of the reads before it are
    in the TSV;
  - extras: --out, --device, --budget-bytes (device workspace per batch of pairs; 0 = a quarter of the free device memory) and
    --dump-alignments (pairwise2.format_alignment's three lines per read, for debugging).
"""
import argparse
import sys

import numpy as np

from .backend import ALIGN_CLIP_INDEX_ERROR, ALIGN_SCORES, Backend


def read_ref_tsv(path):
    """{read id: reference sequence} -- radian/align.py:67-74"""
    read_ref = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            if i == 0:
                continue  # header
            read, txt, seq = line.strip("\n").split("\t")
            read_ref[read] = seq
    return read_ref


def read_fasta(path):
    """[(id, sequence)] as Bio.SeqIO.parse(path, "fasta") gives them: text before the first '>' is skipped, the id is the first
    whitespace-delimited token of the title, sequence lines are joined with trailing whitespace, spaces and CRs removed"""
    records = []
    title, lines = None, []
    with open(path, "r") as f:
        for line in f:
            if line.startswith(">"):
                if title is not None:
                    records.append((title, lines))
                title, lines = line[1:].rstrip(), []
            elif title is not None:
                lines.append(line.rstrip())
    if title is not None:
        records.append((title, lines))
    out = []
    for t, ls in records:
        rid = t.split(None, 1)[0] if t.split() else ""
        out.append((rid, "".join(ls).replace(" ", "").replace("\r", "")))
    return out


def output_path(fasta):
    """radian/align.py:64, refusing to overwrite the input"""
    out = fasta.replace(".fasta", ".tsv")
    if out == fasta:
        raise SystemExit(f"align: output path {out!r} would overwrite the FASTA (its name has no '.fasta'); give --out")
    return out


def rates(n_match, n_sub, n_ins, n_del):
    """[acc, p_ins, p_del, p_sub, p_err] in percent -- radian/align.py:93-97, the same float64 operations"""
    tot = n_match + n_sub + n_ins + n_del
    return [n_match / tot * 100, n_ins / tot * 100, n_del / tot * 100, n_sub / tot * 100, (n_ins + n_del + n_sub) / tot * 100]


def summary(stats):
    """the five print lines of radian/align.py:104-109"""
    stats = np.asarray(stats)
    return (f"Accuracy\tMEDIAN: {np.median(stats[:,0]):.2f}\tMEAN: {np.mean(stats[:,0]):.2f}\n"
            f"Insertions\tMEDIAN: {np.median(stats[:,1]):.2f}\tMEAN: {np.mean(stats[:,1]):.2f}\n"
            f"Deletions\tMEDIAN: {np.median(stats[:,2]):.2f}\tMEAN: {np.mean(stats[:,2]):.2f}\n"
            f"Substitutions\tMEDIAN: {np.median(stats[:,3]):.2f}\tMEAN: {np.mean(stats[:,3]):.2f}\n\n"
            f"Total error\tMEDIAN: {np.median(stats[:,4]):.2f}\tMEAN: {np.mean(stats[:,4]):.2f}\n\n")


def format_alignment(ops, ref, seq):
    """pairwise2.format_alignment's three lines (ref, match line, read) of an alignment given as M / X / D / I columns"""
    g, mline, p = [], [], []
    i = j = 0
    for o in ops.decode("ascii"):
        if o in "MX":
            g.append(ref[i]), p.append(seq[j]), mline.append("|" if o == "M" else ".")
            i += 1
            j += 1
        elif o == "D":
            g.append(ref[i]), p.append("-"), mline.append(" ")
            i += 1
        else:
            g.append("-"), p.append(seq[j]), mline.append(" ")
            j += 1
    return "".join(g) + "\n" + "".join(mline) + "\n" + "".join(p) + "\n"


def build_parser():
    ap = argparse.ArgumentParser(description="Read accuracy of a basecalled FASTA against per-read reference sequences (GPU).")
    ap.add_argument("fasta", help="basecalled reads (FASTA)")
    ap.add_argument("ref_tsv", help="TSV with a header line, then read_id <tab> text <tab> reference sequence")
    ap.add_argument("--out", default=None, help="per-read TSV (default: the FASTA path with '.fasta' replaced by '.tsv')")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per batch of pairs (0: a quarter of free memory)")
    ap.add_argument("--dump-alignments", default=None, metavar="PATH",
                    help="write each read's alignment (score and format_alignment's three lines) here")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    out_file = args.out if args.out is not None else output_path(args.fasta)
    if out_file == args.fasta:
        raise SystemExit(f"align: --out {out_file!r} is the FASTA itself")
    read_ref = read_ref_tsv(args.ref_tsv)
    records = read_fasta(args.fasta)
    for rid, _ in records:   # the reference's KeyError (align.py:82), before anything is written
        if rid not in read_ref:
            raise KeyError(rid)
    refs = [read_ref[rid] for rid, _ in records]
    seqs = [seq.replace("U", "T") for _, seq in records]
    with Backend(args.device) as be:
        res = be.align(refs, seqs, ALIGN_SCORES, budget_bytes=args.budget_bytes, with_ops=args.dump_alignments is not None)
    if args.dump_alignments is not None:
        with open(args.dump_alignments, "w") as f:
            for k, (rid, _) in enumerate(records):
                f.write(f">{rid}\tscore={int(res.score[k])}\tstatus={int(res.status[k])}\n")
                f.write(format_alignment(res.ops[k], refs[k], seqs[k]))
    stats = []
    with open(out_file, "w") as out:
        out.write("read_id\tn_match\tn_ins\tn_del\tn_sub\n")
        for k, (rid, _) in enumerate(records):
            if res.status[k] == ALIGN_CLIP_INDEX_ERROR:
                raise IndexError(f"read {rid}: the soft clip ran past the end of its alignment (radian/align.py:33,39)")
            n_match, n_sub, n_ins, n_del = (int(c) for c in res.counts[k])
            if n_match + n_sub + n_ins + n_del == 0:
                raise ZeroDivisionError(f"read {rid}: no counted alignment column is left after the soft clip (radian/align.py:93)")
            stats.append(rates(n_match, n_sub, n_ins, n_del))
            out.write(f"{rid}\t{n_match}\t{n_ins}\t{n_del}\t{n_sub}\n")
    sys.stdout.write(summary(stats))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
