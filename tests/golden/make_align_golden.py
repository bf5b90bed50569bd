#!/usr/bin/env python3
"""Generate tests/golden/align_clip_cases.json from the upstream reference's analyse_alignment (radian/align.py:9-57).

    python tests/golden/make_align_golden.py <reference checkout>/radian

Imports the reference's align.py read-only -- with placeholder Bio, Bio.pairwise2 (format_alignment) and Bio.SeqIO modules, since
Biopython is not needed by analyse_alignment itself -- and calls analyse_alignment on pairwise2.format_alignment-shaped text
(ref line, match line, read line, score line) of a few hundred alignments: every column pattern of length 0..4 over
{match, mismatch, deletion, insertion}, with A/C/G/T/N characters, and seeded random ones with gap-heavy ends.  Stores inputs and
outputs (the four counts or the exception's name) only.  Nothing in the tests reads the reference."""
import itertools
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref_dir):
    bio = types.ModuleType("Bio")
    pw = types.ModuleType("Bio.pairwise2")
    pw.format_alignment = None
    seqio = types.ModuleType("Bio.SeqIO")
    bio.pairwise2, bio.SeqIO = pw, seqio
    sys.modules.setdefault("Bio", bio)
    sys.modules.setdefault("Bio.pairwise2", pw)
    sys.modules.setdefault("Bio.SeqIO", seqio)
    sys.path.insert(0, ref_dir)
    import align as ref_align
    return ref_align


def format_columns(ops, rng, p_n=0.2):
    """the three lines of pairwise2.format_alignment for a column pattern: M (same base), X (two different ones), D (ref base,
    read gap), I (ref gap, read base); some characters are N"""
    def base():
        return "N" if rng.random() < p_n else rng.choice("ACGT")
    gt, mid, pred = [], [], []
    for o in ops:
        if o == "M":
            c = base()
            gt.append(c), pred.append(c), mid.append("|")
        elif o == "X":
            a = base()
            b = rng.choice([x for x in "ACGTN" if x != a])
            gt.append(a), pred.append(b), mid.append(".")
        elif o == "D":
            gt.append(base()), pred.append("-"), mid.append(" ")
        else:
            gt.append("-"), pred.append(base()), mid.append(" ")
    return "".join(gt), "".join(mid), "".join(pred)


def main():
    ref = load_reference(sys.argv[1])
    rng = random.Random(20261015)
    patterns = ["".join(p) for L in range(5) for p in itertools.product("MXDI", repeat=L)]
    for _ in range(240):   # random alignments: junk (insertions) and overhangs (deletions) at the ends, errors inside
        body = "".join(rng.choices("MMMMMMXDI", k=rng.randint(0, 40)))
        head = "".join(rng.choices("IIID", k=rng.randint(0, 8)))
        tail = "".join(rng.choices("IIID", k=rng.randint(0, 8)))
        patterns.append(head + body + tail)
    cases = []
    for ops in patterns:
        gt, mid, pred = format_columns(ops, rng)
        text = f"{gt}\n{mid}\n{pred}\n  Score=0\n"
        try:
            out = list(ref.analyse_alignment(text))
        except Exception as e:   # IndexError is part of the contract
            out = type(e).__name__
        cases.append({"gt": gt, "mid": mid, "pred": pred, "out": out})
    path = os.path.join(HERE, "align_clip_cases.json")
    with open(path, "w") as f:
        json.dump({"source": "radian/align.py analyse_alignment", "cases": cases}, f, indent=0)
    kinds = {}
    for c in cases:
        k = c["out"] if isinstance(c["out"], str) else ("empty" if c["out"] == [0, 0, 0, 0] else "counts")
        kinds[k] = kinds.get(k, 0) + 1
    print(f"{len(cases)} cases -> {path}: {kinds}")


if __name__ == "__main__":
    main()
