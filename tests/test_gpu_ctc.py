"""GPU checks of the model evaluation on labelled windows (rd_ctc_probs / rd_ctc_eval / Backend.ctc_* / python -m radian_amd.evaluate)
against the CPU restatement of the contract (tests/_ctc_ref.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _ctc_ref as ref
import _tfrecord_writer as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def _peaked(rng, T, peak):
    y = rng.dirichlet([0.2] * 5, size=T) * (1 - peak)
    y[np.arange(T), rng.integers(0, 5, size=T)] += peak
    return y.astype(np.float32)


def _cases(rng):
    """(probs [1024, 5], input_len, label) covering the edge shapes"""
    cases = []
    for L in (0, 1, 2, 25, 63, 64, 65, 127, 128, 200, 255):
        for n in (1, 64, 65, 700, 1024):
            y = rng.dirichlet([0.5] * 5, size=1024).astype(np.float32)
            cases.append((y, n, rng.integers(0, 4, size=L)))
    for L in (1, 5, 63, 255):                    # all-repeat labels, feasible and not
        for n in (2 * L - 1, 2 * L, 1024):
            if 1 <= n <= 1024:
                cases.append((rng.dirichlet([0.5] * 5, size=1024).astype(np.float32), n, np.full(L, int(rng.integers(0, 4)))))
    for _ in range(40):                          # peaked rows (a trained model's) and flat rows
        L = int(rng.integers(0, 80))
        cases.append((_peaked(rng, 1024, 0.97), int(rng.integers(max(1, L), 1025)), rng.integers(0, 4, size=L)))
    flat = np.full((1024, 5), 0.2, dtype=np.float32)
    cases += [(flat, 1024, rng.integers(0, 4, size=100)), (flat, 1, np.array([], dtype=np.int64)), (flat, 5, np.array([2]))]
    # exact argmax ties: pairs of classes with equal probability, the blank included
    y = np.zeros((1024, 5), dtype=np.float32)
    for t in range(1024):
        a, b = rng.choice(5, size=2, replace=False)
        y[t, a] = y[t, b] = 0.375
        y[t, [c for c in range(5) if c not in (a, b)]] = 0.25 / 3
    cases.append((y, 1024, rng.integers(0, 4, size=60)))
    onehot = np.zeros((1024, 5), dtype=np.float32)   # zeros: epsilon matters, tiny probabilities
    onehot[np.arange(1024), rng.integers(0, 5, size=1024)] = 1.0
    cases.append((onehot, 1024, rng.integers(0, 4, size=40)))
    cases.append((onehot, 300, rng.integers(0, 4, size=255)))   # infeasible
    return cases


def _check(res, cases, order=None):
    for k, (y, n, lab) in enumerate(cases):
        loss, st, gl, ed = ref.evaluate(y, n, lab)
        assert res.status[k] == st, k
        assert res.greedy_len[k] == gl, k
        assert res.edit_distance[k] == ed, k
        if math.isinf(loss):
            assert math.isinf(res.loss[k]) and res.loss[k] > 0, k
        else:
            assert res.loss[k] == pytest.approx(loss, rel=1e-9, abs=0), (k, n, len(lab))


def test_ctc_probs_equals_reference(be):
    rng = np.random.default_rng(11)
    cases = _cases(rng)
    probs = np.stack([c[0] for c in cases])
    res = be.ctc_probs(probs, [c[1] for c in cases], [c[2] for c in cases], with_greedy=True)
    _check(res, cases)
    assert (res.status == 1).sum() >= 4 and (res.status == 0).sum() >= 50
    for k, (y, n, lab) in enumerate(cases):
        assert res.greedy[k].tolist() == ref.greedy(y, n), k


def test_results_do_not_depend_on_batch_or_order(be):
    rng = np.random.default_rng(12)
    cases = _cases(rng)[:70]
    probs = np.stack([c[0] for c in cases])
    il = np.array([c[1] for c in cases])
    labs = [c[2] for c in cases]
    full = be.ctc_probs(probs, il, labs)
    perm = rng.permutation(len(cases))
    sh = be.ctc_probs(probs[perm], il[perm], [labs[i] for i in perm])
    for j, i in enumerate(perm):
        assert sh.loss[j].tobytes() == full.loss[i].tobytes()
        assert (sh.status[j], sh.greedy_len[j], sh.edit_distance[j]) == (full.status[i], full.greedy_len[i], full.edit_distance[i])
    for bs in (1, 7, 32):
        for lo in range(0, len(cases), bs):
            r = be.ctc_probs(probs[lo: lo + bs], il[lo: lo + bs], labs[lo: lo + bs])
            assert r.loss.tobytes() == full.loss[lo: lo + bs].tobytes() and (r.edit_distance == full.edit_distance[lo: lo + bs]).all()


def test_bad_arguments_are_refused_before_launch(be):
    from radian_amd.backend import RadianHipError
    y = np.full((1, 1024, 5), 0.2, dtype=np.float32)
    with pytest.raises(RadianHipError, match="label_length 256"):
        be.ctc_probs(y, [1024], [np.zeros(256, dtype=np.int64)])
    with pytest.raises(RadianHipError, match="input_length 0"):
        be.ctc_probs(y, [0], [[1]])
    with pytest.raises(RadianHipError, match="input_length 1025"):
        be.ctc_probs(y, [1025], [[1]])
    assert be.ctc_probs(y[:0], [], []).loss.size == 0


def test_ctc_eval_equals_forward_then_reference(be):
    from radian_amd import weights
    rng = np.random.default_rng(13)
    be.load_weights(weights.synthetic_weights(seed=77))
    n = 24
    win = rng.normal(size=(n, 1024)).astype(np.float32)
    il = rng.integers(1, 1025, size=n)
    il[:3] = (1, 1024, 512)
    labs = [rng.integers(0, 4, size=int(rng.integers(0, min(il[i], 255) + 1))) for i in range(n)]
    res = be.ctc_eval(win, il, labs)
    probs = be.forward(win)
    _check(res, [(probs[i], int(il[i]), labs[i]) for i in range(n)])
    same = be.ctc_probs(probs, il, labs)
    assert same.loss.tobytes() == res.loss.tobytes() and (same.edit_distance == res.edit_distance).all()


def test_command_line_end_to_end(be, tmp_path):
    from radian_amd import weights
    rng = np.random.default_rng(14)
    recs = {}
    for split, files in (("val", ("b.tfrecords", "a.tfrecords")), ("train", ("c.tfrecords",))):
        os.makedirs(tmp_path / split)
        for name, packed in zip(files, (True, False)):
            rs = []
            for i in range(int(rng.integers(5, 40))):
                sl = int(rng.integers(1, 1025))
                ll = int(rng.integers(0, 64))
                lab = rng.integers(0, 4, size=ll).astype(float).tolist() + [0.0] * (63 - ll)
                rs.append((rng.normal(size=1024).astype(np.float32), lab, sl, ll))
            rs.append((rng.normal(size=1024).astype(np.float32), [1.0] * 30, 40, 30))   # infeasible
            tw.write_shard(tmp_path / split / name, rs, packed=packed)
            recs[(split, name)] = rs
    out = tmp_path / "w.tsv"
    cmd = [sys.executable, "-m", "radian_amd.evaluate", str(tmp_path), "--sig-model", "synthetic:77", "--sig-config", "none",
           "--batch-size", "7", "--out", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    be.load_weights(weights.synthetic_weights(seed=77))
    exp_rows = []
    for name in ("a.tfrecords", "b.tfrecords"):   # sorted
        rs = recs[("val", name)]
        probs = be.forward(np.stack([x[0] for x in rs]))
        for i, (sig, lab, sl, ll) in enumerate(rs):
            loss, st, gl, ed = ref.evaluate(probs[i], sl, [int(v) for v in lab[:ll]])
            exp_rows.append((name, i, sl, ll, loss, st, gl, ed))
    lines = out.read_text().splitlines()
    assert lines[0] == "file\trecord\tinput_length\tlabel_length\tloss\tgreedy_length\tedit_distance"
    assert len(lines) == len(exp_rows) + 1
    for line, e in zip(lines[1:], exp_rows):
        f = line.split("\t")
        assert (f[0], int(f[1]), int(f[2]), int(f[3]), int(f[5]), int(f[6])) == (e[0], e[1], e[2], e[3], e[6], e[7])
        got = float(f[4])
        assert (math.isinf(got) and math.isinf(e[4])) or got == pytest.approx(e[4], rel=1e-9)
    summ = dict(l.split("\t", 1) for l in r.stdout.strip().splitlines())
    n_inf = sum(e[5] for e in exp_rows)
    assert n_inf >= 2 and summ["val_loss"] == "inf" and int(summ["infeasible_windows"]) == n_inf and int(summ["windows"]) == len(exp_rows)
    fin = [e[4] for e in exp_rows if not math.isinf(e[4])]
    assert float(summ["val_loss_finite"]) == pytest.approx(np.mean(fin), rel=1e-6)
    eds = np.array([e[7] for e in exp_rows], dtype=float)
    assert summ["edit_distance"] == f"MEDIAN: {np.median(eds):.6f}\tMEAN: {np.mean(eds):.6f}"
    # the batch size steers batching only
    r2 = subprocess.run(cmd[:-4] + ["--batch-size", "64", "--out", str(tmp_path / "w2.tsv")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and r2.stdout == r.stdout and (tmp_path / "w2.tsv").read_text() == out.read_text()
