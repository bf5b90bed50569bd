"""Train the signal model on labelled windows: the reference's trainer (radian/train.py:48-93, data.py, model.py:16-40,91-158) on
one MI355X, without TensorFlow.

    python -m radian_amd.train -s shards_dir [-g models/sig2seq.yaml] [-c model-03.rdnw -e 3] [--sig-model init.rdnw]
                               [--epochs N] [--steps-per-epoch K] [--batch-size 32] [--seed 0] [--out-dir .] [--device 0]
                               [--log steps.tsv]

What it keeps from the reference:
  data        `{shards_dir}/train/*.tfrecords` (data.py's records: signal, signal_length, label, label_length), batches of
              train.batch_size windows; validation on `{shards_dir}/val/*.tfrecords` every train.val_freq epochs with the loss of
              `python -m radian_amd.evaluate` (the reference's val_loss);
  model       sig2seq.yaml's graph, Keras's initial weights (weights.keras_init_weights: the distributions, not TensorFlow's
              random stream), ctc_batch_cost averaged over the batch;
  optimiser   train.opt.adam (TF 2.4 Adam: epsilon added to sqrt(v)); only weights are checkpointed, so a resume starts a fresh
              optimiser, as Keras's does;
  checkpoints model-{epoch:02d}.rdnw after every epoch (weights.pack_blob; loadable by basecall and evaluate --sig-model);
              `-c checkpoint -e epoch` resumes after that epoch (an .h5 of Keras weights or an .rdnw).
What differs:
  the stream  shuffle(50001).repeat() becomes an endless sequence of permutations of all training windows, permutation p a
              function of (--seed, p) only; every batch is full (batches run across permutation boundaries).  Step s of the run
              takes stream positions s * batch_size onwards, so a resume at epoch e starts at step e * steps_per_epoch and sees
              the batches the continuous run would have seen;
  steps       --steps-per-epoch defaults to one pass over the training windows (the reference's 911506 is its own dataset's);
  infeasible  a window without a CTC path (label_length + repeats > signal_length) contributes zero loss and zero gradient, and
              the batch mean still divides by the batch size; Keras would turn the whole step into inf / NaN.  Their count is
              printed;
  scope       one GPU.  The reference's multi-worker setup (tensorflow_nodefile, MultiWorkerMirroredStrategy) is not read;
              Keras .h5 checkpoints are not written; sgd, adagrad and cc_opt, amsgrad, clipnorm / clipvalue, dropout and batch
              norm, and a model.tcn.kernel_initializer other than he_normal, are refused with the yaml field named;
  memory      every training window is held in host memory for the run: 4 KiB of signal per window plus its labels (about 4 GB per
              million windows), as read from the shards.
Every epoch prints `epoch k/N loss L val_loss V infeasible I` (val_loss `-` on epochs without validation).  --log writes one TSV
row per step: epoch, step, loss, infeasible windows.  There is no CPU fallback.
"""
import argparse
import functools
import math
import os
import sys

import numpy as np

from .backend import Backend
from .basecall import load_dilations, load_sig_model
from .evaluate import evaluate_shards, shard_files
from .tfrecord import read_shard
from .weights import DEFAULT_DILATIONS, keras_init_weights, pack_blob

# sig2seq.yaml's train section: what `-g none` stands for
DEFAULT_TRAIN = {"batch_size": 32, "n_epochs": 1000, "val_freq": 1,
                 "opt": {"type": "adam", "adam": {"lr": 0.0001, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "amsgrad": False,
                                                   "clipnorm": False, "clipvalue": False}}}


class ConfigError(ValueError):
    pass


def train_settings(cfg):
    """the yaml's (parsed) train / model sections -> {batch_size, n_epochs, val_freq, lr, beta_1, beta_2, epsilon}; raises
    ConfigError naming the field of any setting this trainer does not implement"""
    tr = cfg.get("train", {})
    opt = tr.get("opt", {})
    kind = opt.get("type", "adam")
    if kind != "adam":
        raise ConfigError(f"train.opt.type is {kind!r}: only 'adam' is implemented (sgd, adagrad and cc_opt are not)")
    adam = opt.get("adam", {})
    if adam.get("amsgrad", False):
        raise ConfigError("train.opt.adam.amsgrad is set: AMSGrad is not implemented")
    for f in ("clipnorm", "clipvalue"):
        if adam.get(f, False) not in (False, None):
            raise ConfigError(f"train.opt.adam.{f} is {adam[f]!r}: gradient clipping is not implemented")
    tcn = cfg.get("model", {}).get("tcn", {})
    if float(tcn.get("dropout_rate", 0.0) or 0.0) > 0:
        raise ConfigError(f"model.tcn.dropout_rate is {tcn['dropout_rate']}: dropout is not implemented")
    if tcn.get("use_batch_norm", False):
        raise ConfigError("model.tcn.use_batch_norm is set: batch norm is not implemented")
    init = tcn.get("kernel_initializer", "he_normal")
    if init != "he_normal":
        raise ConfigError(f"model.tcn.kernel_initializer is {init!r}: only 'he_normal' (sig2seq.yaml's) is implemented")
    out = {"batch_size": int(tr.get("batch_size", 32)), "n_epochs": int(tr.get("n_epochs", 1000)), "val_freq": int(tr.get("val_freq", 1))}
    for k, d in (("lr", 1e-4), ("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7)):
        out[k] = float(adam.get(k, d))
    if out["batch_size"] < 1 or out["val_freq"] < 1:
        raise ConfigError("train.batch_size and train.val_freq must be at least 1")
    return out


def load_config(path):
    """(train settings, dilations) of a sig2seq.yaml; `none` stands for sig2seq.yaml's own values"""
    if not path or path.lower() == "none":
        return train_settings({"train": DEFAULT_TRAIN}), DEFAULT_DILATIONS
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    settings = train_settings(cfg)   # before load_dilations, whose check of dropout / batch norm names no field
    return settings, load_dilations(path)


def checkpoint_name(epoch):
    """Keras's ModelCheckpoint("model-{epoch:02d}.h5") after epoch index epoch - 1, as an .rdnw"""
    return f"model-{epoch:02d}.rdnw"


@functools.lru_cache(maxsize=2)
def pass_permutation(seed, p, n):
    """the order of the training windows in pass p of the stream (read-only).  Building one costs O(n); the two most recent passes
    are kept, so a step costs O(batch_size) and a pass's permutation is built once however many steps read it."""
    perm = np.random.default_rng([int(seed), int(p)]).permutation(int(n))
    perm.setflags(write=False)
    return perm


def batch_indices(seed, n, batch_size, step):
    """window indices of global step `step`: stream positions [step * batch_size, (step + 1) * batch_size)"""
    out = np.empty(batch_size, dtype=np.int64)
    pos = step * batch_size
    k = 0
    while k < batch_size:
        p, off = divmod(pos + k, n)
        perm = pass_permutation(int(seed), int(p), int(n))
        take = min(batch_size - k, n - off)
        out[k: k + take] = perm[off: off + take]
        k += take
    return out


def epoch_steps(epoch_index, steps_per_epoch):
    """the global steps of epoch index e (0-based, Keras's): a resume with -e e starts at step e * steps_per_epoch"""
    return range(epoch_index * steps_per_epoch, (epoch_index + 1) * steps_per_epoch)


class Windows:
    """every record of the training shards, in file then record order, kept shard by shard as read (no concatenated copy): host
    memory is the shards' own size, 4 KiB of signal per window plus one byte per label (about 4 GB per million windows)"""

    def __init__(self, files):
        self.shards = [read_shard(path) for path in files]
        self.start = np.cumsum([0] + [len(sh) for sh in self.shards])

    def __len__(self):
        return int(self.start[-1])

    def batch(self, idx):
        """(signals [b, 1024], input_len [b], labels) of the windows idx"""
        idx = np.asarray(idx, dtype=np.int64)
        which = np.searchsorted(self.start, idx, side="right") - 1
        sig = np.empty((idx.size, 1024), dtype=np.float32)
        il = np.empty(idx.size, dtype=np.int32)
        labs = []
        for k, (f, i) in enumerate(zip(which, idx - self.start[which])):
            sh = self.shards[f]
            sig[k] = sh.signals[i]
            il[k] = sh.input_len[i]
            labs.append(sh.label(i))
        return sig, il, labs


def build_parser():
    ap = argparse.ArgumentParser(
        description="Train the signal model on labelled TFRecord windows (CTC loss, Adam) on one GPU.  The reference's multi-worker "
                    "setup (tensorflow_nodefile) is not read: training runs on one GPU.")
    ap.add_argument("-s", "--shards-dir", required=True, help="directory holding train/*.tfrecords and val/*.tfrecords")
    ap.add_argument("-g", "--config-file", default="models/sig2seq.yaml", help="sig2seq.yaml (`none`: its default values)")
    ap.add_argument("-c", "--checkpoint", default=None, help="weights to resume from (.h5 of Keras weights or .rdnw)")
    ap.add_argument("-e", "--initial_epoch", default=0, type=int, help="epochs already done by the checkpoint")
    ap.add_argument("--sig-model", default=None, help="initial weights to fine-tune (.h5 / .rdnw; default: Keras's initialisers)")
    ap.add_argument("--epochs", default=None, type=int, help="epoch to train up to (default: train.n_epochs)")
    ap.add_argument("--steps-per-epoch", default=None, type=int, help="default: one pass over the training windows")
    ap.add_argument("--batch-size", default=None, type=int, help="default: train.batch_size")
    ap.add_argument("--seed", default=0, type=int, help="initial weights and the order of the training stream")
    ap.add_argument("--out-dir", default=".", help="where model-{epoch:02d}.rdnw go")
    ap.add_argument("--device", default=0, type=int, help="GPU index")
    ap.add_argument("--log", default=None, help="per-step TSV: epoch, step, loss, infeasible")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        cfg, dilations = load_config(args.config_file)
    except ConfigError as e:
        raise SystemExit(f"train: {args.config_file}: {e}")
    bs = args.batch_size or cfg["batch_size"]
    epochs = cfg["n_epochs"] if args.epochs is None else args.epochs
    if bs < 1:
        raise SystemExit("train: --batch-size must be at least 1")
    if args.initial_epoch < 0 or (args.initial_epoch and not args.checkpoint):
        raise SystemExit("train: -e/--initial_epoch needs -c/--checkpoint")
    if args.checkpoint and args.sig_model:
        raise SystemExit("train: give either -c/--checkpoint or --sig-model")
    data = Windows(shard_files(args.shards_dir, "train"))
    val_files = shard_files(args.shards_dir, "val")
    if len(data) == 0:
        raise SystemExit("train: the training shards hold no windows")
    spe = args.steps_per_epoch or max(1, math.ceil(len(data) / bs))
    if args.checkpoint:
        w = load_sig_model(args.checkpoint, dilations)
    elif args.sig_model:
        w = load_sig_model(args.sig_model, dilations)
    else:
        w = keras_init_weights(args.seed, dilations)
    os.makedirs(args.out_dir, exist_ok=True)
    log = open(args.log, "w") if args.log else None
    if log:
        log.write("epoch\tstep\tloss\tinfeasible\n")
    with Backend(args.device) as be:
        be.load_weights(w, dilations)   # a fresh optimiser: zero moments, t = 0
        for e in range(args.initial_epoch, epochs):
            losses, infeasible = [], 0
            for step in epoch_steps(e, spe):
                sig, il, labs = data.batch(batch_indices(args.seed, len(data), bs, step))
                loss, status = be.train_step(sig, il, labs, lr=cfg["lr"], beta1=cfg["beta_1"], beta2=cfg["beta_2"], epsilon=cfg["epsilon"])
                bad = int((status != 0).sum())
                mean = float(loss[status == 0].sum() / len(loss))
                losses.append(mean)
                infeasible += bad
                if log:
                    log.write(f"{e + 1}\t{step}\t{mean!r}\t{bad}\n")
            with open(os.path.join(args.out_dir, checkpoint_name(e + 1)), "wb") as f:
                f.write(pack_blob(be.get_weights(), dilations))
            val = "-"
            if (e + 1) % cfg["val_freq"] == 0:
                rows = evaluate_shards(be, val_files, bs)
                val = f"{np.mean(np.array([r[4] for r in rows], dtype=np.float64)):.6f}"
            print(f"epoch {e + 1}/{epochs} loss {np.mean(losses):.6f} val_loss {val} infeasible {infeasible}", flush=True)
    if log:
        log.close()


if __name__ == "__main__":
    main()
