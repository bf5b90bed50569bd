"""GPU checks of training (rd_train_grad / rd_train_step / rd_get_weights / python -m radian_amd.train) against the CPU
restatement of the contract (tests/_train_ref.py: torch autograd in fp64, numpy Keras-Adam)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _train_ref as ref
import _tfrecord_writer as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = (1, 2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def _names(dil=DIL):
    from radian_amd import weights
    return weights.tensor_shapes(dil)


def _split(flat, dil=DIL):
    out, o = {}, 0
    for name, shape in _names(dil):
        n = int(np.prod(shape))
        out[name] = np.asarray(flat[o:o + n], dtype=np.float64)
        o += n
    return out


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _rows(rng, T, peak):
    y = rng.dirichlet([0.3] * 5, size=T) * (1 - peak)
    y[np.arange(T), rng.integers(0, 5, size=T)] += peak
    return y.astype(np.float32)


def test_ctc_gradient_against_torch_fp64(be):
    """dL/dz row by row (rd_train_ctc_grad) against torch fp64 autograd through Keras's chain on z = log(y): L = 0, repeated labels,
    L = 255, short input_length, and an infeasible window, which must give zero rows; rows past input_length are exactly zero"""
    pytest.importorskip("torch")
    rng = np.random.default_rng(21)
    cases = [(1024, []), (1024, [2, 2, 2, 1, 1]), (1024, list(rng.integers(0, 4, size=255))), (40, list(rng.integers(0, 4, size=12))),
             (7, [1]), (700, [3] * 200), (10, [1, 1, 1, 1, 1, 1])]          # the last: 6 labels + 5 repeats > 10 rows
    y = np.stack([_rows(rng, 1024, 0.0 if k % 2 else 0.9) for k in range(len(cases))])
    il = [c[0] for c in cases]
    labs = [c[1] for c in cases]
    gz, loss, st = be.train_ctc_grad(y, il, labs)
    rl, rg = ref.ctc_grad_z(np.log(y.astype(np.float64)), il, labs)
    assert list(st) == [0] * 6 + [1] and np.isinf(loss[6]) and not gz[6].any()
    assert loss[:6].sum() / len(cases) == pytest.approx(rl, rel=1e-9)
    for k, (n, lab) in enumerate(cases[:6]):
        assert not gz[k, n:].any(), k
        assert _rel(gz[k, :n], rg[k, :n]) < 1e-6, (k, n, len(lab), _rel(gz[k, :n], rg[k, :n]))
        assert np.abs(gz[k, :n] - rg[k, :n]).max() <= 1e-6 * np.abs(rg[k, :n]).max() + 1e-12, k


def test_infeasible_window_adds_nothing_to_the_weight_gradient(be):
    from radian_amd import weights
    rng = np.random.default_rng(20)
    be.load_weights(weights.synthetic_weights(seed=5, head_gain=0.3))
    x = rng.normal(size=(2, 1024)).astype(np.float32)
    g, loss, st = be.train_grad(x, [10, 1024], [[1, 1, 1, 1, 1, 1], [2, 3]])    # window 0: 6 labels + 5 repeats > 10 rows
    assert list(st) == [1, 0] and np.isinf(loss[0]) and np.isfinite(loss[1])
    g1, _, _ = be.train_grad(x[1:], [1024], [[2, 3]])
    assert np.array_equal(g, g1 / 2)   # the infeasible window adds nothing; the mean divides by 2
    gi, li, si = be.train_grad(x[:1], [10], [[1, 1, 1, 1, 1, 1]])
    assert si[0] == 1 and not gi.any()


def test_full_gradient_against_torch_fp64(be, capsys):
    """every one of the 30 tensors, 8 windows, He-normal weights with a soft head; tolerance 4x the error of the restatement in the
    kernel's arithmetic (fp32 network, fp64 CTC; the largest over ref.summation_variants: batch orders, one thread, and the ReLU
    units within rounding of zero on their other side), and as before 4x the all-fp32 restatement's, whose fp32 CTC makes it wider.
    Measured on an MI355X without the ReLU variant: block 0's first kernel at 3.96e-4 against a yardstick of 6.0e-5 (6.6x); one such
    unit alone moves that tensor by up to 5.3e-4 (CPU, fp64), and seven of them account for the GPU's error down to 6.7e-7"""
    torch = pytest.importorskip("torch")
    from radian_amd import weights
    rng = np.random.default_rng(22)
    w = weights.synthetic_weights(seed=6, head_gain=0.3)
    be.load_weights(w)
    x = rng.normal(size=(8, 1024)).astype(np.float32)
    il = [1024, 1024, 900, 512, 1024, 300, 1024, 64]
    labs = [rng.integers(0, 4, size=int(rng.integers(0, min(n // 3, 255) + 1))) for n in il]
    g, loss, st = be.train_grad(x, il, labs)
    rl, rg, _ = ref.loss_and_grad(w, x, il, labs, DIL)
    _, rg32, _ = ref.loss_and_grad(w, x, il, labs, DIL, dtype=torch.float32)
    assert not st.any()
    assert loss.sum() / 8 == pytest.approx(rl, rel=1e-5)
    G, R, R32 = _split(g), _split(rg), _split(rg32)
    yard = ref.gradient_yardstick(w, x, il, labs, DIL, ref.summation_variants(8, flip=ref.relu_candidates(w, x, DIL)), ref_grads=R)
    worst, worst_a = [], []
    for name, _ in _names():
        noise = _rel(R32[name], R[name])
        err = _rel(G[name], R[name])
        worst.append((err / max(noise, 1e-12), name, err, noise))
        worst_a.append((err / max(yard[name], 1e-7), name, err, yard[name]))
    with capsys.disabled():
        r, name, err, noise = max(worst)
        print(f"\n[train] gradient rel-L2 vs fp64: worst ratio {r:.2f} ({name}: gpu {err:.2e}, torch fp32 {noise:.2e})")
        r, name, err, noise = max(worst_a)
        print(f"[train] default graph, 8 windows: worst ratio to the yardstick {r:.2f} ({name}: gpu {err:.2e}, yardstick {noise:.2e})")
    for (_, name, err, noise), (_, _, _, y) in zip(worst, worst_a):
        assert err <= 4 * max(noise, 1e-7), (name, err, noise)
        assert err <= ref.bound(y), (name, err, y)


def _adam_close(got, exp):
    """op-order tolerance, per element: the GPU rounds each Adam operation as numpy's float32 does, so only alpha's pow may differ
    (by an ulp), which moves a weight by at most one rounding: |got - exp| <= 2.5e-7 |exp| + 1e-9"""
    err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    bound = 2.5e-7 * np.abs(exp.astype(np.float64)) + 1e-9
    assert (err <= bound).all(), float((err - bound).max())


def test_adam_steps_are_keras_adam_of_the_gpu_gradients(be):
    """three steps: t advances, beta^t and the moments carry from call to call"""
    from radian_amd import weights
    rng = np.random.default_rng(23)
    w = weights.keras_init_weights(1)
    be.load_weights(w)
    m, v = np.zeros_like(w), np.zeros_like(w)
    prev = w
    for t in (1, 2, 3):
        x = rng.normal(size=(4, 1024)).astype(np.float32)
        il = [1024] * 4
        labs = [rng.integers(0, 4, size=50) for _ in range(4)]
        g, loss0, _ = be.train_grad(x, il, labs)
        loss, _ = be.train_step(x, il, labs, lr=1e-3)
        assert loss.tobytes() == loss0.tobytes()
        got = be.get_weights()
        exp, m, v = ref.keras_adam(prev, g, m, v, t, lr=1e-3)
        _adam_close(got, exp)
        assert np.abs(got - prev).max() > 1e-5
        prev = got
    be.train_reset()      # t back to 1, zero moments: the next step is a first step again
    g, _, _ = be.train_grad(x, il, labs)
    be.train_step(x, il, labs, lr=1e-3)
    exp, _, _ = ref.keras_adam(prev, g, np.zeros_like(w), np.zeros_like(w), 1, lr=1e-3)
    _adam_close(be.get_weights(), exp)


def _batches(rng, n_steps, n=4):
    out = []
    for _ in range(n_steps):
        x = rng.normal(size=(n, 1024)).astype(np.float32)
        out.append((x, [1024] * n, [rng.integers(0, 4, size=40) for _ in range(n)]))
    return out


def test_two_contexts_train_bit_identically():
    from radian_amd import Backend, weights
    rng = np.random.default_rng(24)
    w = weights.keras_init_weights(2)
    bs = _batches(rng, 5)
    res = []
    for _ in range(2):
        with Backend(0) as b:
            b.load_weights(w)
            for x, il, labs in bs:
                b.train_step(x, il, labs, lr=1e-3)
            res.append(b.get_weights())
    assert res[0].tobytes() == res[1].tobytes()


def test_packed_images_follow_the_trained_weights():
    from radian_amd import Backend, weights
    rng = np.random.default_rng(25)
    w = weights.keras_init_weights(3)
    x = rng.normal(size=(3, 1024)).astype(np.float32)
    with Backend(0) as b, Backend(0) as fresh, Backend(0) as clone:
        b.load_weights(w)
        before = b.forward(x)
        for xb, il, labs in _batches(rng, 3):
            b.train_step(xb, il, labs, lr=1e-3)
        tw_ = b.get_weights()
        fresh.load_weights(tw_)
        assert b.forward(x).tobytes() == fresh.forward(x).tobytes()
        assert b.forward(x).tobytes() != before.tobytes()
        for prec in ("bf16x3", "f16x3"):
            b.set_precision(prec)
            fresh.set_precision(prec)
            assert b.forward(x).tobytes() == fresh.forward(x).tobytes(), prec
        b.set_precision("fp32")
        b._check(b._L.rd_clone_artifacts(clone._h, b._h))
        clone.set_precision("bf16x3")
        fresh.set_precision("bf16x3")
        assert clone.forward(x).tobytes() == fresh.forward(x).tobytes()
        # weights that arrived by a clone: the library knows the parameter count, so the training calls work on them
        assert clone.get_weights().tobytes() == tw_.tobytes()
        clone.set_precision("fp32")
        xb, il, labs = _batches(rng, 1)[0]
        assert clone.train_grad(xb, il, labs)[0].tobytes() == b.train_grad(xb, il, labs)[0].tobytes()


def _teacher_set(rng, n_win, seed=41, gain=3.0):
    """64 signals labelled by the greedy decode of a synthetic teacher; every label feasible and at most 255 long"""
    from radian_amd import Backend, weights
    x = rng.normal(size=(n_win, 1024)).astype(np.float32)
    with Backend(0) as t:
        t.load_weights(weights.synthetic_weights(seed=seed, head_gain=gain))
        y = t.forward(x)
    il, labs = [], []
    for i in range(n_win):
        best = y[i].argmax(1)
        out, prev, n = [], 4, 1024
        for r, c in enumerate(best):
            if c != 4 and c != prev:
                if len(out) == 255:
                    n = r
                    break
                out.append(int(c))
            prev = c
        il.append(n)
        labs.append(np.array(out, dtype=np.int64))
    return x, il, labs


def test_it_learns(be, capsys):
    from radian_amd import weights
    rng = np.random.default_rng(26)
    x, il, labs = _teacher_set(rng, 64)
    be.load_weights(weights.keras_init_weights(7))
    curve = []
    for s in range(300):
        loss, st = be.train_step(x, il, labs, lr=1e-3)
        assert not st.any()
        curve.append(float(loss.mean()))
    with capsys.disabled():
        print("\n[train] learning curve (batch mean loss, every 25 steps): " + " ".join(f"{v:.1f}" for v in curve[::25]) + f" ... {curve[-1]:.1f}")
    # measured on an MI355X: 622 at the start, a rise to about 2000 while the head saturates, 109 after 300 steps
    assert min(curve[-10:]) <= 0.3 * curve[0], (curve[0], curve[-10:])


def _write_split(tmp_path, split, rng, n, files=1):
    os.makedirs(tmp_path / split, exist_ok=True)
    for f in range(files):
        recs = []
        for _ in range(n):
            L = int(rng.integers(1, 60))
            recs.append((rng.normal(size=1024).astype(np.float32), [int(c) for c in rng.integers(0, 4, size=L)], 1024, L))
        tw.write_shard(str(tmp_path / split / f"s{f}.tfrecords"), recs)


def _run(args, cwd):
    p = subprocess.run([sys.executable, "-m", *args], cwd=cwd, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_command_line_end_to_end(tmp_path):
    rng = np.random.default_rng(27)
    _write_split(tmp_path, "train", rng, 10, files=2)
    _write_split(tmp_path, "val", rng, 7)
    common = ["radian_amd.train", "-s", str(tmp_path), "-g", "none", "--epochs", "2", "--steps-per-epoch", "3", "--batch-size", "4",
              "--seed", "9"]
    out = _run(common + ["--out-dir", str(tmp_path / "run"), "--log", str(tmp_path / "steps.tsv")], ROOT)
    lines = [l for l in out.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and lines[1].startswith("epoch 2/2 loss ")
    for k in (1, 2):
        assert os.path.exists(tmp_path / "run" / f"model-{k:02d}.rdnw")
    val2 = lines[1].split("val_loss ")[1].split()[0]
    ev = _run(["radian_amd.evaluate", str(tmp_path), "--sig-config", "none", "--sig-model", str(tmp_path / "run" / "model-02.rdnw")], ROOT)
    assert ev.splitlines()[0] == f"val_loss\t{val2}"
    assert len(open(tmp_path / "steps.tsv").read().splitlines()) == 1 + 6
    # resume after epoch 1: epoch 2 only, from model-01's weights with fresh moments
    outs = []
    for r in ("a", "b"):
        o = _run(common + ["-c", str(tmp_path / "run" / "model-01.rdnw"), "-e", "1", "--out-dir", str(tmp_path / r)], ROOT)
        assert [l.split()[1] for l in o.splitlines() if l.startswith("epoch ")] == ["2/2"]
        assert not os.path.exists(tmp_path / r / "model-01.rdnw")
        outs.append(open(tmp_path / r / "model-02.rdnw", "rb").read())
    assert outs[0] == outs[1]
    assert outs[0] != open(tmp_path / "run" / "model-02.rdnw", "rb").read()   # Keras restarts the optimiser on a resume


def test_bad_input_is_refused_before_launch(be):
    from radian_amd import weights
    from radian_amd.backend import RadianHipError
    be.load_weights(weights.keras_init_weights(8))
    w0 = be.get_weights()
    x = np.zeros((1, 1024), dtype=np.float32)
    with pytest.raises(RadianHipError, match="label_length 256"):
        be.train_step(x, [1024], [np.zeros(256, dtype=np.int64)])
    with pytest.raises(RadianHipError, match="input_length 0"):
        be.train_step(x, [0], [[1]])
    # (Backend refuses label 4 in Python; the library's own check is reached through the C entry point)
    il, lab, off, ll = np.array([1024], np.int32), np.array([4], np.uint8), np.array([0], np.int64), np.array([1], np.int32)
    grad, loss, st = np.zeros(w0.size, np.float32), np.zeros(1), np.zeros(1, np.int32)
    with pytest.raises(RadianHipError, match="not 0..3"):
        be._check(be._L.rd_train_grad(be._h, x.ctypes.data, 1, il.ctypes.data, lab.ctypes.data, off.ctypes.data, ll.ctypes.data,
                                      grad.ctypes.data, loss.ctypes.data, st.ctypes.data))
    be.set_precision("bf16x3")
    with pytest.raises(RadianHipError, match="exact fp32 only"):
        be.train_step(x, [1024], [[1]])
    be.set_precision("fp32")
    assert be.get_weights().tobytes() == w0.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# Gradients under the yardstick of the kernel's own arithmetic (ref.gradient_yardstick: fp32 network, fp64 CTC, the largest error
# over several summation orders and over the ReLU units that rounding can put on either side of zero), at the batch sizes where
# train_run's weight-gradient split changes and on other graphs.

def _check_gradient(be, capsys, tag, seed, dil, n, special=False, one_thread=True):
    """train_grad on `dil` and a ref.batch_case against torch fp64: statuses, the mean loss to 1e-5, every tensor's relative L2
    error within 4x max(yardstick, 1e-7).  Prints the worst ratio before it asserts.  -> ({name: gpu grad}, {name: fp64 grad})"""
    pytest.importorskip("torch")
    from radian_amd import weights
    dil = tuple(dil)
    w = weights.synthetic_weights(seed=seed, head_gain=0.3, dilations=dil)
    x, il, labs = ref.batch_case(seed + 1000, n, special=special)
    be.load_weights(w, dil)
    g, loss, st = be.train_grad(x, il, labs)
    rl, _, R = ref.loss_and_grad(w, x, il, labs, dil)
    variants = ref.summation_variants(n, one_thread=one_thread, flip=ref.relu_candidates(w, x, dil))
    yard = ref.gradient_yardstick(w, x, il, labs, dil, variants, ref_grads=R)
    G = _split(g, dil)
    rows = [(_rel(G[k], R[k]) / max(yard[k], 1e-7), k, _rel(G[k], R[k]), yard[k]) for k, _ in _names(dil)]
    with capsys.disabled():
        r, name, err, y = max(rows)
        print(f"\n[train] {tag}: worst ratio to the yardstick {r:.2f} ({name}: gpu {err:.2e}, yardstick {y:.2e})")
    feasible = np.ones(n, dtype=bool)
    if special:
        feasible[n - 1] = False
    assert np.array_equal(st == 0, feasible) and np.isinf(loss[~feasible]).all() and np.isfinite(loss[feasible]).all()
    assert loss[feasible].sum() / n == pytest.approx(rl, rel=1e-5)
    for _, name, err, y in rows:
        assert err <= ref.bound(y), (tag, name, err, y)
    return G, R


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_gradient_across_the_weight_gradient_split_regimes(be, capsys, n):
    """dilations (1, 3).  train_run cuts each weight-gradient GEMM into min(64, 4 n) splits: 256 rows each up to n = 16 (4, 60, 64
    splits here), 16 n rows from n = 17 (272 and 528 here), which start inside windows, so that only the shifted-row mask keeps a
    tap out of the window before.  From 15 windows on the batch holds a window without a label, one with 255 labels and one
    without a CTC path"""
    _check_gradient(be, capsys, f"dilations (1, 3), {n} windows", 50 + n, (1, 3), n, special=n >= 15)


def test_gradient_of_the_shipped_configuration(be, capsys):
    """the default graph at train.batch_size's default of 32: all 30 tensors.  The yardstick here is the largest over three batch
    orders; its one-thread variant is left out to keep the reference near 15 s, which can only make the bound tighter"""
    _check_gradient(be, capsys, "default graph, 32 windows", 90, DIL, 32, special=True, one_thread=False)


@pytest.mark.parametrize("dil,n", [((3,), 5), ((1, 512, 5), 3), ((2, 1024, 7), 3), ((1, 2, 4, 8) * 4, 2), ((1,), 1)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gradient_on_other_graphs(be, capsys, dil, n):
    """one block (the backward's b == 0 branch straight after the head), a dilation that is no power of two, dilations whose taps
    lie in the padding, 16 blocks (the most rd_load_weights takes).  A tap shifted by 1024 rows or more reads only padding: its
    slice of both convs' kernel gradients is exactly zero, in the reference as well"""
    G, R = _check_gradient(be, capsys, f"dilations {dil if len(dil) < 8 else '(1, 2, 4, 8) x 4'}, {n} windows", 70 + len(dil), dil, n)
    for b, d in enumerate(dil):
        for conv in ("conv1D_0", "conv1D_1"):
            name = f"tcn/residual_block_{b}/{conv}/kernel"
            for grads in (G, R):
                k = grads[name].reshape(3, -1, 256)
                for tap in range(2):
                    if (2 - tap) * d >= 1024:
                        assert not k[tap].any(), (name, tap)


@pytest.mark.parametrize("dil,n", [((3,), 5), ((1, 2, 4, 8) * 4, 2)], ids=["3", "16-blocks"])
def test_adam_and_the_images_on_other_graphs(be, dil, n):
    """three steps on one block and on 16 (pack_kernel's table at its longest): each is Keras-Adam of the GPU's own gradient, and
    the packed images then equal those of a fresh context given get_weights(), in fp32 and bf16x3"""
    from radian_amd import Backend, weights
    w = weights.synthetic_weights(seed=61, head_gain=0.3, dilations=dil)
    be.load_weights(w, dil)
    m, v = np.zeros_like(w), np.zeros_like(w)
    prev = w
    for t in (1, 2, 3):
        x, il, labs = ref.batch_case(62 + t, n)
        g, loss0, _ = be.train_grad(x, il, labs)
        loss, _ = be.train_step(x, il, labs, lr=1e-3)
        assert loss.tobytes() == loss0.tobytes()
        got = be.get_weights()
        exp, m, v = ref.keras_adam(prev, g, m, v, t, lr=1e-3)
        _adam_close(got, exp)
        assert np.abs(got - prev).max() > 1e-5
        prev = got
    with Backend(0) as fresh:
        fresh.load_weights(prev, dil)
        for prec in ("fp32", "bf16x3"):
            be.set_precision(prec)
            fresh.set_precision(prec)
            try:
                assert be.forward(x).tobytes() == fresh.forward(x).tobytes(), prec
            finally:
                be.set_precision("fp32")


def test_resident_step_equals_the_host_step():
    """rd_train_step_resident (windows already in device memory) against rd_train_step on a second context: the same weights and
    losses byte for byte.  Dilations (1, 3), 17 windows"""
    from radian_amd import Backend, weights
    dil, n = (1, 3), 17
    w = weights.synthetic_weights(seed=65, head_gain=0.3, dilations=dil)
    x, il, labs = ref.batch_case(66, n, special=True)
    with Backend(0) as host, Backend(0) as res:
        host.load_weights(w, dil)
        res.load_weights(w, dil)
        d = res.dev_alloc(x.nbytes)
        try:
            res.h2d(d, x)
            for _ in range(2):
                lh, sh = host.train_step(x, il, labs, lr=1e-3)
                lr_, sr = res.train_step(d, il, labs, lr=1e-3, resident_n=n)
                assert lh.tobytes() == lr_.tobytes() and sh.tobytes() == sr.tobytes()
        finally:
            res.dev_free(d)
        assert list(sh) == [0] * (n - 1) + [1]
        got = res.get_weights()
        assert got.tobytes() == host.get_weights().tobytes() and got.tobytes() != w.tobytes()
