#!/usr/bin/env python3
"""The reference's evaluator entry point: `python3 align.py reads.fasta read_ref.tsv` (radian/align.py) -- same arguments, output
TSV and printed summary.  Everything lives in radian_amd.align (alignment, clip and counts on the MI355X); this file only makes the
command a RADIAN user types work unchanged, from any working directory."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from radian_amd.align import main  # noqa: E402

if __name__ == "__main__":
    main()
