"""CPU checks of the training contract's pieces: the reference helper's CTC gradient (tests/_train_ref.py) against finite
differences and brute force, its Keras-Adam against a step worked by hand, the training stream's order, the config refusals and
the checkpoint / resume arithmetic of python -m radian_amd.train."""
import numpy as np
import pytest

import _train_ref as ref


def _case(rng, B, T):
    z = rng.normal(size=(B, T, 5)) * 2.0
    return z


def test_ctc_grad_matches_finite_differences():
    pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    z = _case(rng, 3, 9)
    il = [9, 6, 9]
    labs = [[0, 1, 1, 2], [3], [2, 2, 2]]
    loss, g = ref.ctc_grad_z(z, il, labs)
    h = 1e-6
    for _ in range(30):
        b, t, k = rng.integers(3), rng.integers(9), rng.integers(5)
        zp, zm = z.copy(), z.copy()
        zp[b, t, k] += h
        zm[b, t, k] -= h
        fd = (ref.ctc_grad_z(zp, il, labs)[0] - ref.ctc_grad_z(zm, il, labs)[0]) / (2 * h)
        assert g[b, t, k] == pytest.approx(fd, abs=1e-7, rel=1e-5)
    assert np.all(g[1, 6:] == 0)   # rows beyond input_length


def test_ctc_loss_matches_brute_force_over_all_paths():
    pytest.importorskip("torch")
    rng = np.random.default_rng(2)
    for T, lab in ((1, []), (3, [1]), (4, [1, 1]), (5, [0, 2, 0]), (6, [3, 3, 1]), (6, [2])):
        z = _case(rng, 1, T)
        loss, _ = ref.ctc_grad_z(z, [T], [lab])
        assert loss == pytest.approx(ref.brute_force_loss(z[0], T, lab), rel=1e-10)
    z = _case(rng, 2, 6)
    loss, g = ref.ctc_grad_z(z, [6, 2], [[1, 2], [1, 1]])    # window 1 infeasible: zero loss, zero gradient, mean over 2
    assert loss == pytest.approx(ref.brute_force_loss(z[0], 6, [1, 2]) / 2, rel=1e-10)
    assert np.all(g[1] == 0)


MUT_DIL = (1, 3)
MUT_N = 17


@pytest.fixture(scope="module")
def mutation_case():
    """dilations (1, 3), 17 windows of mixed lengths (one without a label, one with 255, one without a CTC path): the fp64
    gradient, the yardstick over the batch orders (the one-thread variant apart) and the all-fp32 restatement, each computed once"""
    torch = pytest.importorskip("torch")
    from radian_amd import weights
    w = weights.synthetic_weights(seed=31, head_gain=0.3, dilations=MUT_DIL)
    x, il, labs = ref.batch_case(32, MUT_N, special=True)
    assert min(len(l) for l in labs) == 0 and max(len(l) for l in labs) == 255 and len(set(il)) > 2
    _, _, R = ref.loss_and_grad(w, x, il, labs, MUT_DIL)
    variants = ref.summation_variants(MUT_N, one_thread=False, flip=ref.relu_candidates(w, x, MUT_DIL))
    yard = ref.gradient_yardstick(w, x, il, labs, MUT_DIL, variants, ref_grads=R)
    _, _, R32 = ref.loss_and_grad(w, x, il, labs, MUT_DIL, dtype=torch.float32)
    old = {k: ref.rel_l2(R32[k], R[k]) for k in R}
    return dict(w=w, x=x, il=il, labs=labs, R=R, yard=yard, old=old)


def _rejected(grads, case, which):
    """the tensors whose error against fp64 is beyond 4x the yardstick `which`"""
    return [k for k in case["R"] if ref.rel_l2(grads[k], case["R"][k]) > ref.bound(case[which][k])]


def test_the_gradient_bound_has_teeth(mutation_case, capsys):
    """The fp32-network restatement stands in for a kernel.  Summed in an order the yardstick has not seen it passes 4x the yardstick
    in every tensor; with one row's dL/dz dropped, with the batch mean taken over n + 1, or with one input_length one short it
    fails in at least one.  The dropped row passes the bound this project used before (4x the all-fp32 restatement's error, whose
    fp32 CTC is a hundred times noisier than the fp32 network): that is why the yardstick changed."""
    c = mutation_case
    n = MUT_N
    run = lambda il=c["il"], **kw: ref.loss_and_grad_kernel_arithmetic(c["w"], c["x"], il, c["labs"], MUT_DIL, **kw)[2]
    right = run(order=[int(i) for i in np.random.default_rng(77).permutation(n)], threads=2)
    assert _rejected(right, c, "yard") == []
    k = next(i for i in range(1, n - 1) if c["il"][i] >= 512 and i != n // 2 and len(c["labs"][i]))

    def drop_row(g):
        g = g.clone()
        g[k, 200] = 0
        return g

    short = list(c["il"])
    short[k] -= 1
    wrong = {"dropped row": run(z_hook=drop_row), "mean over n + 1": run(z_hook=lambda g: g * (n / (n + 1.0))), "input_length - 1": run(il=short)}
    counts = {name: (len(_rejected(g, c, "yard")), len(_rejected(g, c, "old"))) for name, g in wrong.items()}
    with capsys.disabled():
        print("\n[train] tensors rejected of %d (new bound, old bound): " % len(c["R"]) + ", ".join(f"{k} {a}/{b}" for k, (a, b) in counts.items()))
    for name, (new, _) in counts.items():
        assert new >= 1, (name, counts)
    assert counts["dropped row"][1] == 0, counts


def test_the_yardstick_holds_against_itself(mutation_case):
    """the one-thread run, whose reductions are split differently from every multi-thread run, is inside 4x the yardstick taken
    without it"""
    c = mutation_case
    one = ref.loss_and_grad_kernel_arithmetic(c["w"], c["x"], c["il"], c["labs"], MUT_DIL, threads=1)[2]
    assert _rejected(one, c, "yard") == []


def test_threads_are_restored_and_order_is_only_an_order():
    torch = pytest.importorskip("torch")
    from radian_amd import weights
    w = weights.synthetic_weights(seed=33, head_gain=0.3, dilations=(3,))
    x, il, labs = ref.batch_case(34, 3)
    before = torch.get_num_threads()
    l0, g0, _ = ref.loss_and_grad(w, x, il, labs, (3,))
    l1, g1, _ = ref.loss_and_grad(w, x, il, labs, (3,), order=[2, 0, 1], threads=1)
    assert torch.get_num_threads() == before
    assert l1 == pytest.approx(l0, rel=1e-12) and ref.rel_l2(g1, g0) < 1e-12
    seen = []
    ref.loss_and_grad(w, x, il, labs, (3,), order=[2, 0, 1], z_hook=lambda g: (seen.append(g.clone()), g)[1])
    _, gz = ref.ctc_grad_z(ref.logits(w, x, (3,)), il, labs)
    assert np.abs(seen[0].numpy() - gz).max() <= 1e-12 * np.abs(gz).max()   # the hook sees rows in the caller's order


@pytest.mark.parametrize("dilations", [(3,), (1, 512, 5), (2, 1024, 7), (1, 2, 4, 8) * 4], ids=lambda d: "-".join(map(str, d)))
def test_reference_probs_against_the_oracle(oracle, dilations):
    """ref.probs (torch fp64), on which the GPU gradient tests rest, against the C oracle's fp64-accumulating forward on graphs that
    no other test puts through it: one block, a dilation whose taps lie partly and wholly in the padding, 16 blocks.  The oracle
    rounds its rows to float32, so 1e-6 is output rounding (rows are at most 1) with room for an ulp or two"""
    pytest.importorskip("torch")
    from radian_amd import weights
    w = weights.synthetic_weights(seed=35, head_gain=0.3, dilations=dilations)
    x = np.random.default_rng(36).normal(size=(2, 1024)).astype(np.float32)
    got = ref.probs(w, x, dilations)
    exp = oracle.tcn_forward(w, x, dilations=dilations, acc64=True)
    assert np.abs(got - exp).max() <= 1e-6, float(np.abs(got - exp).max())


def test_keras_adam_by_hand():
    w, g = np.float32(0.5), np.float32(-0.02)
    m, v = np.float32(0.0), np.float32(0.0)
    w1, m1, v1 = ref.keras_adam([w], [g], [m], [v], 1, lr=1e-3)
    # t = 1, with TF's float32 constants 1 - beta1, 1 - beta2 (1 - 0.999f = 0.00099998713...):
    # m = (1 - b1) g, v = (1 - b2) g^2, alpha = lr sqrt(1 - b2) / (1 - b1), step = alpha m / (sqrt(v) + eps)
    omb1 = float(np.float32(1) - np.float32(0.9))
    omb2 = float(np.float32(1) - np.float32(0.999))
    alpha = 1e-3 * np.sqrt(omb2) / omb1
    step = alpha * (omb1 * g) / (np.sqrt(omb2 * g * g) + 1e-7)
    assert m1[0] == pytest.approx(omb1 * g, rel=1e-6) and v1[0] == pytest.approx(omb2 * g * g, rel=1e-6)
    assert w1[0] == pytest.approx(w - step, rel=1e-6, abs=1e-9)
    # epsilon goes to sqrt(v), not sqrt(v_hat): with a tiny gradient the step differs from torch.optim.Adam's
    w2, _, _ = ref.keras_adam([w], [np.float32(1e-7)], [m], [v], 1, lr=1e-3)
    torch_style = w - 1e-3 * (1e-7) / (1e-7 + 1e-7)
    keras_style = w - alpha * (omb1 * 1e-7) / (np.sqrt(omb2) * 1e-7 + 1e-7)
    assert w2[0] == pytest.approx(keras_style, rel=1e-6) and abs(w2[0] - torch_style) > 1e-5


def test_stream_is_deterministic_and_covers_each_pass():
    from radian_amd.train import batch_indices, pass_permutation
    n, bs = 37, 8
    seq = np.concatenate([batch_indices(5, n, bs, s) for s in range(20)])
    again = np.concatenate([batch_indices(5, n, bs, s) for s in range(20)])
    assert np.array_equal(seq, again)
    assert not np.array_equal(seq, np.concatenate([batch_indices(6, n, bs, s) for s in range(20)]))
    for p in range(len(seq) // n):
        assert sorted(seq[p * n:(p + 1) * n]) == list(range(n))
        assert np.array_equal(seq[p * n:(p + 1) * n], pass_permutation(5, p, n))
    assert all(len(batch_indices(5, n, bs, s)) == bs for s in range(10))


def test_stream_builds_each_permutation_once():
    """a step costs O(batch): a pass's permutation of all n windows is built once, not once per step"""
    from radian_amd.train import batch_indices, pass_permutation
    pass_permutation.cache_clear()
    n, bs = 3_000_000, 32
    steps = 2 * n // bs + 5                       # three passes, batches crossing both boundaries
    first = [batch_indices(7, n, bs, s) for s in range(0, 200)]
    assert pass_permutation.cache_info().misses == 1
    for s in range(n // bs - 3, steps):
        batch_indices(7, n, bs, s)
    assert pass_permutation.cache_info().misses == 3
    assert np.array_equal(first[0], pass_permutation(7, 0, n)[:bs])
    with pytest.raises(ValueError):
        pass_permutation(7, 0, n)[0] = 1          # shared, read-only


def test_windows_gather_across_shards(tmp_path):
    import _tfrecord_writer as tw
    from radian_amd.train import Windows
    rng = np.random.default_rng(3)
    recs = []
    for f, count in enumerate((5, 1, 7)):
        rs = [(rng.normal(size=1024).astype(np.float32), [int(c) for c in rng.integers(0, 4, size=int(rng.integers(0, 9)))], int(rng.integers(1, 1025)),
               None) for _ in range(count)]
        rs = [(a, b, c, len(b)) for a, b, c, _ in rs]
        tw.write_shard(str(tmp_path / f"s{f}.tfrecords"), rs)
        recs += rs
    data = Windows([str(tmp_path / f"s{f}.tfrecords") for f in range(3)])
    assert len(data) == 13
    idx = np.array([12, 0, 5, 6, 5, 4])
    sig, il, labs = data.batch(idx)
    for k, i in enumerate(idx):
        assert np.array_equal(sig[k], recs[i][0]) and il[k] == recs[i][2] and list(labs[k]) == recs[i][1]


def test_config_refusals_name_the_field():
    from radian_amd.train import ConfigError, DEFAULT_TRAIN, train_settings
    import copy

    def cfg(**mod):
        c = {"train": copy.deepcopy(DEFAULT_TRAIN), "model": {"tcn": {"dropout_rate": 0.0, "use_batch_norm": False}}}
        for path, v in mod.items():
            d = c
            keys = path.split("__")
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = v
        return c

    s = train_settings(cfg())
    assert (s["batch_size"], s["lr"], s["beta_1"], s["beta_2"], s["epsilon"]) == (32, 1e-4, 0.9, 0.999, 1e-7)
    for mod, field in ((dict(train__opt__type="sgd"), "train.opt.type"), (dict(train__opt__type="adagrad"), "train.opt.type"),
                       (dict(train__opt__type="cc_opt"), "train.opt.type"), (dict(train__opt__adam__amsgrad=True), "amsgrad"),
                       (dict(train__opt__adam__clipnorm=1.0), "clipnorm"), (dict(train__opt__adam__clipvalue=0.5), "clipvalue"),
                       (dict(model__tcn__dropout_rate=0.1), "dropout_rate"), (dict(model__tcn__use_batch_norm=True), "use_batch_norm"),
                       (dict(model__tcn__kernel_initializer="glorot_uniform"), "model.tcn.kernel_initializer")):
        with pytest.raises(ConfigError, match=field):
            train_settings(cfg(**mod))


def test_checkpoint_names_and_resume_arithmetic():
    from radian_amd.train import checkpoint_name, epoch_steps
    assert checkpoint_name(1) == "model-01.rdnw" and checkpoint_name(12) == "model-12.rdnw" and checkpoint_name(123) == "model-123.rdnw"
    assert list(epoch_steps(0, 4)) == [0, 1, 2, 3]
    assert list(epoch_steps(2, 4)) == [8, 9, 10, 11]   # -e 2 resumes at step 2 * steps_per_epoch of the same stream


def test_keras_init_distributions():
    from radian_amd import weights
    w = weights.keras_init_weights(3)
    assert w.dtype == np.float32 and w.size == weights.n_params() == 2200581
    assert np.array_equal(w, weights.keras_init_weights(3)) and not np.array_equal(w, weights.keras_init_weights(4))
    o = 0
    for name, shape in weights.tensor_shapes():
        n = int(np.prod(shape))
        t = w[o:o + n]
        o += n
        if name.endswith("bias"):
            assert not t.any()
        elif name.startswith("dense"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            assert np.abs(t).max() <= lim
        else:
            sd = np.sqrt(2.0 / int(np.prod(shape[:-1]))) / 0.87962566103423978
            assert np.abs(t).max() <= 2 * sd + 1e-7
            if n > 10000:
                assert t.std() == pytest.approx(np.sqrt(2.0 / int(np.prod(shape[:-1]))), rel=0.02)   # truncation restores the He stddev
