"""Build the RNA k-mer model the global beam search decodes with, from a transcriptome FASTA, on the GPU.

    python -m radian_amd.lm_build transcripts.fa[.gz] -o rnamodel.json [--context-len 11] [--protein-coding | --field N --value S]
           [--as-written] [--unseen backoff|uniform|absent] [--pseudocount 0] [--rna-threshold 0.5] [--heldout other.fa]
    python -m radian_amd.lm_build --score rnamodel.json --heldout other.fa

The reference ships one model (human protein-coding mRNA, models/rnamodel_12mer_pc.json) and nothing that makes one.  What a row of the
model means is fixed by the reference's lookup (radian/decode.py:42-49,77-96,152-158): labelings are in decode order, 3'->5' (the FASTA
line is written reversed, basecall.py:130), and the row of a context is the distribution of the label that follows it.  So the windows
of k + 1 labels are counted on the transcripts reversed (--as-written: as they stand), lower orders are exact marginals, and a context
the transcriptome does not hold takes the row of its longest suffix that it does hold (--unseen backoff), a uniform row, or none
(--unseen absent: a sparse model, whose absent contexts end a read like the reference's KeyError).  The file written is the reference's
JSON, readable by `basecall --rna-model` here and there.  No CPU path: the counts, the table and the scores come from the GPU.
"""
import argparse
import os
import sys

from . import lm
from .backend import Backend

UNSEEN = ("backoff", "uniform", "absent")


def build_parser():
    ap = argparse.ArgumentParser(prog="lm_build", description="Build (or score) the RNA k-mer model of `basecall --rna-model` from a transcriptome FASTA on one GPU.")
    ap.add_argument("fasta", nargs="?", default=None, help="transcripts, 5'->3' as in GENCODE / Ensembl cDNA files (.gz accepted)")
    ap.add_argument("-o", "--output", default=None, help="the model file to write (JSON, the reference's format)")
    ap.add_argument("--context-len", default=11, type=int, help="labels of context, 1..13 (the reference's --context-len; default 11)")
    ap.add_argument("--field", default=None, type=int, help="keep only records whose header, split on |, has --value in this field (0-based)")
    ap.add_argument("--value", default=None, help="see --field")
    ap.add_argument("--protein-coding", action="store_true", help="--field 7 --value protein_coding (GENCODE headers; the reference's evaluator keeps these)")
    ap.add_argument("--as-written", action="store_true", help="count the records as they stand: the input is already in decode order (3'->5')")
    ap.add_argument("--unseen", default="backoff", choices=UNSEEN, help="row of a context without a count at order k (default: back off to its longest counted suffix)")
    ap.add_argument("--pseudocount", default=0.0, type=float, help="alpha added to each of a row's four counts (default 0)")
    ap.add_argument("--rna-threshold", default=0.5, type=float, help="entropy below which the decoder consults the model (basecall's flag; default 0.5)")
    ap.add_argument("--heldout", default=None, help="another FASTA to score against the model (same filter and direction)")
    ap.add_argument("--score", default=None, help="an existing model file to score --heldout against, instead of building one")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    return ap


def _share(a, b):
    return f"{100.0 * a / b:.2f} %" if b else "-"


def _read(path, field, value, what):
    if not os.path.exists(path):
        raise SystemExit(f"lm_build: {what} {path}: no such file")
    try:
        return lm.read_fasta(path, field, value)
    except ValueError as e:
        raise SystemExit(f"lm_build: {what} {e}")


def _print_score(sc, path, r):
    print(f"held-out {path}: {sc['windows']} windows, mean -ln p = {sc['mean_nll']:.6f} over {sc['scored']} with p > 0; "
          f"p = 0: {sc['zero']}; context absent: {sc['absent']}; gate open (entropy < {r:g}): {_share(sc['gate_windows'], sc['windows'])}")


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.protein_coding:
        if args.field is not None or args.value is not None:
            raise SystemExit("lm_build: --protein-coding is --field 7 --value protein_coding: give one or the other")
        args.field, args.value = 7, "protein_coding"
    if (args.field is None) != (args.value is None):
        raise SystemExit("lm_build: --field and --value go together")
    if args.field is not None and args.field < 0:
        raise SystemExit("lm_build: --field counts from 0")
    if not 1 <= args.context_len <= 13:
        raise SystemExit("lm_build: --context-len must be 1..13")
    if not (0.0 <= args.pseudocount < float("inf")):
        raise SystemExit("lm_build: --pseudocount must be a number >= 0")
    if args.rna_threshold != args.rna_threshold:
        raise SystemExit("lm_build: --rna-threshold must be a number")
    r = args.rna_threshold
    if args.score is not None:
        if args.fasta is not None or args.output is not None:
            raise SystemExit("lm_build: --score scores an existing model: give neither a FASTA to build from nor -o/--output")
        if args.heldout is None:
            raise SystemExit("lm_build: --score needs --heldout")
        if not os.path.exists(args.score):
            raise SystemExit(f"lm_build: --score {args.score}: no such file")
        codes, offsets, info = _read(args.heldout, args.field, args.value, "--heldout")
        table, k = lm.load_json(args.score)
        with Backend(args.device) as be:
            be.load_lm(table, k)
            sc = be.score_lm(codes, offsets, as_written=args.as_written, r_threshold=r)
        print(f"model {args.score}: {k} labels of context, {4 ** k - lm.n_missing(table)} of {4 ** k} contexts")
        _print_score(sc, args.heldout, r)
        return sc
    if args.fasta is None:
        raise SystemExit("lm_build: give a FASTA of transcripts (or --score MODEL --heldout FASTA)")
    if args.output is None:
        raise SystemExit("lm_build: -o/--output is required")
    k = args.context_len
    codes, offsets, info = _read(args.fasta, args.field, args.value, "input")
    if info["kept"] == 0:
        raise SystemExit(f"lm_build: none of the {info['records']} records of {args.fasta} passes --field {args.field} --value {args.value}"
                         if args.field is not None else f"lm_build: {args.fasta} holds no record")
    held = _read(args.heldout, args.field, args.value, "--heldout") if args.heldout else None
    with Backend(args.device) as be:
        table, st = be.build_lm(codes, offsets, k, as_written=args.as_written, unseen=args.unseen, pseudocount=args.pseudocount, r_threshold=r)
        sc = be.score_lm(held[0], held[1], as_written=args.as_written, r_threshold=r) if held else None
    rows, nbytes = lm.write_json(args.output, table, k)
    print(f"records: {info['records']} read, {info['kept']} kept; bases: {info['bases']}; windows of {k + 1} labels counted: {st['windows']}")
    print(f"contexts seen at order {k}: {st['contexts_seen']} of {st['contexts']} ({_share(st['contexts_seen'], st['contexts'])})")
    filled = ", ".join(f"order {j}: {n}" for j, n in st["rows_per_order"].items())
    extra = "".join(f", {name}: {st[key]}" for name, key in (("uniform", "uniform_rows"), ("absent", "absent_rows")) if st[key])
    print(f"rows filled -- {filled}{extra}")
    print(f"gate open (entropy < {r:g}): {_share(st['gate_contexts'], st['contexts'])} of contexts, {_share(st['gate_windows'], st['windows'])} of counted windows")
    if sc is not None:
        _print_score(sc, args.heldout, r)
    print(f"wrote {args.output}: {rows} contexts, {nbytes} bytes")
    return st


if __name__ == "__main__":
    main()
    sys.exit(0)
