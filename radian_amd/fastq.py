"""Basecalls with per-base qualities and signal positions: fast5 in, FASTQ (and a move table) out, on one GPU.

    python -m radian_amd.fastq fast5_dir out_dir [basecall's model / LM / geometry / beam flags]
           [--moves PATH] [--summary PATH] [--device N] [--batch-reads R] [--budget-bytes B]

NO reference behaviour: radian/basecall.py writes bare FASTA.  Every read is basecalled as `python -m radian_amd.basecall` does in
global mode (same flags, same artefacts, the same labels bit for bit) through the blocking fused route rd_basecall_raw_global_q,
which then aligns the read's labels against the very probability rows its beam search read (forced CTC alignment, DESIGN.md
section 16).  One {stem}.fastq per input file; bases 5' to 3' as basecall writes them (the labels reversed), the qualities reversed
with them, chr(33 + Q), Q = min(50, floor(-10 log10(1 - p))) with p the model's probability of the base at the step it was emitted.
Q is the model's own confidence, NOT calibrated against observed error rates.

--moves    TSV: read_id, n_samples, first_step, last_step -- comma-separated, one entry per written base in written order (so the
           values decrease); in global mode one row is one raw sample: these are sample indices into the read
--summary  TSV: read_id, length, viterbi_score, mean_q = -10 log10(mean e_i)

--decode-type chunk is refused: a stitched consensus has no single time axis.  A read whose alignment has no path, or does not fit
--budget-bytes, is still written, with '!' qualities, and counted."""
import math
import os
import sys

import numpy as np

from . import fast5
from .backend import Backend, CTCALIGN_OK, CTCALIGN_STATUS_NAMES
from .basecall import apply_artifacts, build_parser as basecall_parser, load_artifacts, report_skipped
from .sequence_assembly import labels_to_str


def _batches(reads, max_reads, max_samples=32 << 20):
    batch, samples = [], 0
    for r in reads:
        batch.append(r)
        samples += len(r[2])
        if len(batch) >= max_reads or samples >= max_samples:
            yield batch
            batch, samples = [], 0
    if batch:
        yield batch


def mean_q(qual):
    """-10 log10 of the mean error the qualities stand for (e = 10^(-Q/10)); inf for no bases"""
    if len(qual) == 0:
        return float("inf")
    e = float(np.mean(10.0 ** (-np.asarray(qual, dtype=np.float64) / 10)))
    return -10.0 * math.log10(e)


def run(args, be, reads, open_out):
    """reads: iterable of (file stem, read id, raw int16 samples) in input order; open_out(stem) -> the text file of that input file.
    Returns the counters."""
    st = {"reads": 0, "written": 0, "skipped": 0, "bases": 0, "mean_q": [], **{s: 0 for s in CTCALIGN_STATUS_NAMES}}
    use_lm = getattr(args, "_lm_loaded", False)
    moves = open(args.moves, "w") if args.moves else None
    summ = open(args.summary, "w") if args.summary else None
    if moves:
        moves.write("read_id\tn_samples\tfirst_step\tlast_step\n")
    if summ:
        summ.write("read_id\tlength\tviterbi_score\tmean_q\n")
    try:
        for batch in _batches(reads, args.batch_reads):
            st["reads"] += len(batch)
            todo = []
            for stem, rid, raw in batch:
                raw = np.ascontiguousarray(raw, dtype=np.int16)
                if len(raw) == 0:
                    report_skipped(rid, 2)
                    st["skipped"] += 1
                else:
                    todo.append((stem, rid, raw))
            if not todo:
                continue
            labels, status, aln = be.basecall_raw_global_q([raw for _, _, raw in todo], args.outlier_clip, args.chunk_len, args.step_size,
                                                           args.beam_width, use_lm, args.sig_threshold, args.rna_threshold,
                                                           budget_bytes=args.budget_bytes, allow_too_large=True)
            for r, (stem, rid, raw) in enumerate(todo):
                if status[r] != 0:
                    report_skipped(rid, status[r])
                    st["skipped"] += 1
                    continue
                if labels[r] is None:
                    raise KeyError(f"read {rid}: the RNA model holds no entry for a context of the beam search (radian/decode.py:83)")
                seq = labels_to_str(labels[r])[::-1]
                a_st = int(aln.status[r])
                qual = aln.qual[r][::-1] if a_st == CTCALIGN_OK else np.zeros(len(seq), dtype=np.uint8)
                open_out(stem).write(f"@{rid}\n{seq}\n+\n{''.join(chr(33 + int(q)) for q in qual)}\n")
                st["written"] += 1
                st["bases"] += len(seq)
                st[CTCALIGN_STATUS_NAMES[a_st]] += 1
                mq = mean_q(qual)
                if len(seq):
                    st["mean_q"].append(mq)
                if moves:
                    first, last = aln.first_step[r][::-1], aln.last_step[r][::-1]
                    moves.write(f"{rid}\t{len(raw)}\t{','.join(str(int(v)) for v in first)}\t{','.join(str(int(v)) for v in last)}\n")
                if summ:
                    summ.write(f"{rid}\t{len(seq)}\t{float(aln.score[r])!r}\t{mq:.3f}\n")
    finally:
        for f in (moves, summ):
            if f:
                f.close()
    return st


def summary(st):
    mq = st["mean_q"]
    return (f"reads: {st['reads']} seen, {st['written']} written; empty or flat signal: {st['skipped']}\n"
            f"bases: {st['bases']}\n"
            + (f"median of the reads' mean Q: {float(np.median(mq)):.2f}\n" if mq else "median of the reads' mean Q: -\n")
            + "alignment: " + "; ".join(f"{s}: {st[s]}" for s in CTCALIGN_STATUS_NAMES) + "\n")


def build_parser():
    ap = basecall_parser()
    ap.prog = "fastq"
    ap.description = "Basecall a nanopore dRNA sequencing run to FASTQ: per-base qualities and signal positions from a forced CTC alignment, on one GPU."
    for a in ap._actions:
        if a.dest == "fasta_dir":
            a.dest, a.metavar, a.help = "out_dir", "out_dir", "Directory to output fastq files (one per input file)."
    ap.add_argument("--moves", default=None, help="TSV of the signal positions of every written base")
    ap.add_argument("--summary", default=None, help="per-read TSV: length, Viterbi score, mean Q")
    ap.add_argument("--batch-reads", default=512, type=int, help="reads per device batch (the output does not depend on it)")
    ap.add_argument("--budget-bytes", default=0, type=int, help="device workspace per alignment launch (0: a quarter of free memory)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.decode_type != "global":
        raise SystemExit("fastq: --decode-type chunk is refused: a stitched consensus has no single time axis to place its bases on "
                         "(qualities and signal positions exist for global decoding only)")
    if args.gpus != 1:
        raise SystemExit("fastq: one GPU (--gpus 1)")
    if not 1 <= args.step_size <= args.chunk_len:
        raise SystemExit("fastq: --step-size must be 1..chunk-len")
    if args.batch_reads < 1 or args.budget_bytes < 0:
        raise SystemExit("fastq: --batch-reads must be at least 1 and --budget-bytes at least 0")
    if not os.path.isdir(args.fast5_dir):
        raise SystemExit(f"fastq: {args.fast5_dir}: no such directory")
    os.makedirs(args.out_dir, exist_ok=True)
    art = load_artifacts(args)
    files = fast5.list_files(args.fast5_dir)   # Path.rglob order, as basecall
    stems = {}
    for p in files:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise SystemExit(f"fastq: {p} and {stems[stem]} would both be written to {stem}.fastq")
        stems[stem] = p
    outs = {}

    def open_out(stem):
        if stem not in outs:
            outs[stem] = open(os.path.join(args.out_dir, stem + ".fastq"), "w")
        return outs[stem]

    reads = ((os.path.splitext(os.path.basename(p))[0], r.read_id, r.get_raw_data()) for p in files for r in fast5.iter_reads(p))
    try:
        with Backend(args.device) as be:
            apply_artifacts(args, be, art)
            del art
            st = run(args, be, reads, open_out)
    finally:
        for f in outs.values():
            f.close()
    sys.stdout.write(summary(st))
    sys.stdout.flush()
    return st


if __name__ == "__main__":
    main()
