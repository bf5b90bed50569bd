"""How good are these weights on held-out windows?  The reference's val_loss (radian/train.py:48-79: Keras ctc_batch_cost on
`{shards_dir}/val/*.tfrecords`, radian/model.py:77-98) and a greedy edit distance, on the MI355X, without TensorFlow.

    python -m radian_amd.evaluate shards_dir [--split val|train] [--sig-model models/sig2seq.h5] [--sig-config models/sig2seq.yaml]
                                  [--batch-size 32] [--precision fp32|f16x3|bf16x3] [--device N] [--out windows.tsv]

Shards are `{shards_dir}/{split}/*.tfrecords`, sorted by name and read record by record (the order of get_dataset(..., val=True),
radian/data.py).  Every window goes through the signal model (the whole 1024-sample window, as Keras's forward sees it), then:
  loss         -log of the summed probability of the label's CTC paths over the first signal_length rows, with
               p = (y + 1e-7) / sum(y + 1e-7) -- Keras ctc_batch_cost (log(y + epsilon)) into TF v1 ctc_loss (log-softmax) --
               in fp64; +inf when no path exists (label_length + adjacent equal labels > signal_length), as in TF;
  val_loss     the mean of the per-window losses (what Keras reports: per-batch means, weighted by batch size), inf when any
               window is infeasible -- the count of those and the mean over the finite ones are printed too;
  greedy       argmax of each counted row (lowest class on a tie), repeats collapsed, blanks dropped; its Levenshtein distance to the
               label, raw and divided by label_length (tf.edit_distance's default normalisation; windows without labels are left
               out of the normalised figures).  The reference's compute_mean_ed_greedy (train.py:25-46) has no body: this
               definition is this project's own.
--batch-size only sets how many windows go to the GPU per call; results do not depend on it.  --out writes one TSV row per window:
file, record, input_length, label_length, loss, greedy_length, edit_distance.  There is no CPU fallback.
"""
import argparse
import glob
import os
import sys

import numpy as np

from .backend import CTC_INFEASIBLE, Backend
from .basecall import load_dilations, load_sig_model
from .tfrecord import read_shard


def shard_files(shards_dir, split):
    """sorted `{shards_dir}/{split}/*.tfrecords` (radian/train.py:48-79)"""
    files = sorted(glob.glob(os.path.join(shards_dir, split, "*.tfrecords")))
    if not files:
        raise SystemExit(f"evaluate: no shards match {os.path.join(shards_dir, split, '*.tfrecords')}")
    return files


def evaluate_shards(be, files, batch_size):
    """[(file, record, input_length, label_length, loss, status, greedy_length, edit_distance)] over every record of files, in order"""
    rows = []
    for path in files:
        sh = read_shard(path)
        name = os.path.basename(path)
        for lo in range(0, len(sh), batch_size):
            hi = min(lo + batch_size, len(sh))
            labels = [sh.label(i) for i in range(lo, hi)]
            res = be.ctc_eval(sh.signals[lo:hi], sh.input_len[lo:hi], labels, sh.label_len[lo:hi])
            for k in range(hi - lo):
                rows.append((name, lo + k, int(sh.input_len[lo + k]), int(sh.label_len[lo + k]), float(res.loss[k]), int(res.status[k]),
                             int(res.greedy_len[k]), int(res.edit_distance[k])))
    return rows


def summary(rows):
    """the summary lines printed after a run"""
    loss = np.array([r[4] for r in rows], dtype=np.float64)
    infeasible = sum(1 for r in rows if r[5] == CTC_INFEASIBLE)
    finite = loss[np.isfinite(loss)]
    ed = np.array([r[7] for r in rows], dtype=np.float64)
    nz = [(r[7], r[3]) for r in rows if r[3] > 0]
    edn = np.array([e / l for e, l in nz], dtype=np.float64)
    f = lambda a, fn: f"{fn(a):.6f}" if a.size else "nan"
    return (f"val_loss\t{f(loss, np.mean)}\n"
            f"infeasible_windows\t{infeasible}\n"
            f"val_loss_finite\t{f(finite, np.mean)}\n"
            f"edit_distance\tMEDIAN: {f(ed, np.median)}\tMEAN: {f(ed, np.mean)}\n"
            f"edit_distance_normalised\tMEDIAN: {f(edn, np.median)}\tMEAN: {f(edn, np.mean)}\n"
            f"windows\t{len(rows)}\n")


def build_parser():
    ap = argparse.ArgumentParser(description="CTC loss (Keras val_loss) and greedy edit distance of a signal model on labelled TFRecord windows (GPU).")
    ap.add_argument("shards_dir", help="directory holding {split}/*.tfrecords")
    ap.add_argument("--split", default="val", choices=["val", "train"])
    ap.add_argument("--sig-model", default="models/sig2seq.h5")
    ap.add_argument("--sig-config", default="models/sig2seq.yaml")
    ap.add_argument("--batch-size", default=32, type=int, help="windows per GPU call (results do not depend on it)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "f16x3", "bf16x3"], help="matrix products of the signal model (as basecall)")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--out", default=None, help="per-window TSV")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("evaluate: --batch-size must be at least 1")
    files = shard_files(args.shards_dir, args.split)
    dilations = load_dilations(args.sig_config)
    weights = load_sig_model(args.sig_model, dilations)
    with Backend(args.device) as be:
        be.set_precision(args.precision)
        be.load_weights(weights, dilations)
        rows = evaluate_shards(be, files, args.batch_size)
    if args.out:
        with open(args.out, "w") as f:
            f.write("file\trecord\tinput_length\tlabel_length\tloss\tgreedy_length\tedit_distance\n")
            for r in rows:
                f.write(f"{r[0]}\t{r[1]}\t{r[2]}\t{r[3]}\t{r[4]!r}\t{r[6]}\t{r[7]}\n")
    sys.stdout.write(summary(rows))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
