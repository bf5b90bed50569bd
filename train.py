#!/usr/bin/env python3
"""The reference's trainer entry point: `python3 train.py -s shards_dir [-g models/sig2seq.yaml] [-c checkpoint -e epoch]`
(radian/train.py) on one GPU.  Everything lives in radian_amd.train; this file only makes the command a RADIAN user types work,
from any working directory."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from radian_amd.train import main  # noqa: E402

if __name__ == "__main__":
    main()
