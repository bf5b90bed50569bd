"""CPU restatement of the training contract of rd_train_* (radian_amd/csrc/train.hip): the graph of
model.py:52-89 in stock PyTorch operators with autograd, Keras's loss chain (softmax -> log(y + 1e-7) -> TF's log-softmax -> CTC,
blank = 4, the batch mean) through torch.nn.functional.ctc_loss, and TF 2.4's Adam in numpy float32; the same graph in the kernel's
own arithmetic (fp32 network, fp64 loss chain) as the yardstick of the gradient tests.  Test infrastructure."""
import itertools

import numpy as np

EPS = 1e-7
BLANK = 4


def _tensors(flat, dilations, dtype):
    import torch
    from radian_amd import weights
    t, o = {}, 0
    for name, shape in weights.tensor_shapes(dilations):
        n = int(np.prod(shape))
        t[name] = torch.tensor(np.asarray(flat[o:o + n], dtype=np.float64).reshape(shape), dtype=dtype, requires_grad=True)
        o += n
    assert o == flat.size
    return t


def _graph(t, x, dilations):
    """the graph as a generator: yields the argument of each ReLU in turn (h1, h2, out of every block as [B, 256, T], then the
    Dense's [B, T, 128]), is sent that ReLU's result, and returns z [B, T, 5] (the last Dense's output)"""
    import torch.nn.functional as F

    def causal(v, kernel, bias, d):
        w = kernel.permute(2, 1, 0)
        return F.conv1d(F.pad(v, ((kernel.shape[0] - 1) * d, 0)), w, bias, dilation=d)

    v = x[:, None, :]
    for b, d in enumerate(dilations):
        p = f"tcn/residual_block_{b}/"
        h = yield causal(v, t[p + "conv1D_0/kernel"], t[p + "conv1D_0/bias"], d)
        h = yield causal(h, t[p + "conv1D_1/kernel"], t[p + "conv1D_1/bias"], d)
        res = causal(v, t[p + "matching_conv1D/kernel"], t[p + "matching_conv1D/bias"], 1) if b == 0 else v
        v = yield res + h
    h = yield v.transpose(1, 2) @ t["dense/kernel"] + t["dense/bias"]
    return h @ t["dense_1/kernel"] + t["dense_1/bias"]


def forward_logits(t, x, dilations, flip=None):
    """z [B, T, 5] of windows x [B, T].  flip: per ReLU (in _graph's order) a boolean tensor of its argument's shape, or None;
    where it is set the unit takes the other side of the ReLU (passes where it would block, blocks where it would pass)"""
    import torch
    g = _graph(t, x, dilations)
    try:
        pre, i = next(g), 0
        while True:
            f = None if flip is None else flip[i]
            pre, i = g.send(torch.relu(pre) if f is None else pre * ((pre > 0) ^ f).to(pre.dtype)), i + 1
    except StopIteration as done:
        return done.value


def relu_candidates(flat, x, dilations):
    """per ReLU a boolean array [B, ...]: the units whose argument in fp64 is nonzero and no further from zero than the largest
    difference between the fp32 and the fp64 argument anywhere in that layer.  An fp32 implementation that sums in another order
    may find such a unit on either side of zero, and the gradient has a jump there: either side is a right answer."""
    import torch
    x = np.asarray(x, dtype=np.float64)
    with torch.no_grad():
        g64 = _graph(_tensors(np.asarray(flat), dilations, torch.float64), torch.as_tensor(x), dilations)
        g32 = _graph(_tensors(np.asarray(flat), dilations, torch.float32), torch.as_tensor(x, dtype=torch.float32), dilations)
        out = []
        try:
            a, b = next(g64), next(g32)
            while True:
                tau = (b.double() - a).abs().max()
                out.append(((a.abs() <= tau) & (a != 0)).numpy())
                a, b = g64.send(torch.relu(a)), g32.send(torch.relu(b))
        except StopIteration:
            return out


def keras_ctc_mean_of_rows(y, input_len, labels):
    """Keras ctc_batch_cost on softmax rows y [B, T, 5], infeasible windows counted as zero, summed and divided by the batch size"""
    import torch
    import torch.nn.functional as F
    lp = torch.log_softmax(torch.log(y + EPS), dim=-1)
    n = y.shape[0]
    tg = [torch.as_tensor(np.asarray(l, dtype=np.int64)) for l in labels]
    flat = torch.cat(tg) if sum(len(a) for a in tg) else torch.zeros(0, dtype=torch.int64)
    loss = F.ctc_loss(lp.transpose(0, 1), flat, torch.as_tensor(np.asarray(input_len, dtype=np.int64)),
                      torch.as_tensor([len(a) for a in tg], dtype=torch.int64), blank=BLANK, reduction="sum", zero_infinity=True)
    return loss / n


def keras_ctc_mean(z, input_len, labels):
    """the same on logits z, the softmax in z's own type"""
    import torch
    return keras_ctc_mean_of_rows(torch.softmax(z, dim=-1), input_len, labels)


def loss_and_grad(flat, x, input_len, labels, dilations, dtype=None, ctc64=False, order=None, threads=None, z_hook=None, flip=None):
    """(mean loss, flat gradient in load_weights order, {name: grad}) by autograd.
    dtype   torch.float64 (default) or float32: the type of the tensors, the input and forward_logits
    ctc64   the softmax rows y = softmax(z) in dtype, then y.double() into the loss chain.  With dtype float32 this is train.hip's
            arithmetic: an fp32 network and fp32 rows (head_fwd_kernel), the CTC in fp64 (ctc_logp_kernel, ctc_ab_kernel, ctc_grad_kernel)
    order   a permutation of the batch: the windows are summed in that order (the gradient is the same sum in another order)
    threads torch.set_num_threads for the call (restored): another split of every reduction
    z_hook  a function of dL/dz [B, T, 5] (rows in the caller's order) that returns its replacement: seeded faults for the tests
    flip    relu_candidates' arrays (windows in the caller's order): those units take the other side of their ReLU"""
    import torch
    from radian_amd import weights
    dtype = dtype or torch.float64
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    order = np.arange(n) if order is None else np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(n))
    before = torch.get_num_threads()
    if threads:
        torch.set_num_threads(int(threads))
    try:
        t = _tensors(np.asarray(flat), dilations, dtype)
        z = forward_logits(t, torch.as_tensor(x[order], dtype=dtype), dilations,
                           None if flip is None else [None if f is None else torch.as_tensor(np.asarray(f)[order]) for f in flip])
        if z_hook is not None:
            inv = torch.as_tensor(np.argsort(order))
            fwd = torch.as_tensor(order)
            z.register_hook(lambda g: z_hook(g[inv])[fwd])
        il = [input_len[i] for i in order]
        labs = [labels[i] for i in order]
        if ctc64:
            loss = keras_ctc_mean_of_rows(torch.softmax(z, dim=-1).double(), il, labs)
        else:
            loss = keras_ctc_mean(z, il, labs)
        loss.backward()
    finally:
        torch.set_num_threads(before)
    grads = {k: v.grad.detach().to(torch.float64).numpy().ravel() for k, v in t.items()}
    return float(loss.detach()), np.concatenate([grads[k] for k, _ in weights.tensor_shapes(dilations)]), grads


def loss_and_grad_kernel_arithmetic(flat, x, input_len, labels, dilations, **kw):
    """loss_and_grad in the arithmetic of train.hip: fp32 network and softmax rows, fp64 loss chain"""
    import torch
    return loss_and_grad(flat, x, input_len, labels, dilations, dtype=torch.float32, ctc64=True, **kw)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def summation_variants(n, seed=0, one_thread=True, flip=None):
    """the variants the yardstick takes its maximum over: the batch as given, reversed, in a seeded permutation, on one thread
    (orders that coincide at a small batch are listed once), and with relu_candidates' units `flip` on the other side"""
    orders = [tuple(range(n)), tuple(range(n))[::-1], tuple(int(i) for i in np.random.default_rng(seed).permutation(n))]
    out = [dict(order=list(o)) for o in dict.fromkeys(orders)]
    if one_thread:
        out.append(dict(threads=1))
    if flip is not None:
        # restates the ReLU masks of train.hip (gemm_kernel's epilogues `p.aux[o] > 0.f`, head_bwd_kernel's `h3[i] > 0.f`): they are
        # taken from fp32 sums in the MFMA's own order, so a unit within rounding of zero can fall on the other side than torch's
        out.append(dict(flip=flip))
    return out


def gradient_yardstick(flat, x, input_len, labels, dilations, variants, ref_grads=None):
    """{tensor name: the largest relative L2 error, against the fp64 loss_and_grad, of loss_and_grad_kernel_arithmetic over the
    variants (keyword sets: order, threads, flip)}.  What fp32 summation in one order or another costs a correct implementation of the
    kernel's arithmetic; ref_grads: loss_and_grad's {name: grad} when the caller has it already."""
    if ref_grads is None:
        ref_grads = loss_and_grad(flat, x, input_len, labels, dilations)[2]
    worst = {k: 0.0 for k in ref_grads}
    for kw in variants:
        g = loss_and_grad_kernel_arithmetic(flat, x, input_len, labels, dilations, **kw)[2]
        for k in worst:
            worst[k] = max(worst[k], rel_l2(g[k], ref_grads[k]))
    return worst


def bound(yardstick):
    """the project's rule: an implementation may be 4x as far from fp64 as the yardstick, which is floored at 1e-7"""
    return 4 * max(yardstick, 1e-7)


LENGTHS = (1024, 900, 512, 300, 64)


def batch_case(seed, n, special=False):
    """(x [n, 1024] float32, input_len, labels): input lengths drawn from LENGTHS, random labels of at most min(len // 3, 255).
    special (n >= 3): window 0 has no label, window n // 2 has 255 labels on 1024 rows, and window n - 1 has no CTC path
    (40 equal labels need 79 rows, it has 64)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 1024)).astype(np.float32)
    il = [int(v) for v in rng.choice(LENGTHS, size=n)]
    labs = [rng.integers(0, 4, size=int(rng.integers(0, min(m // 3, 255) + 1))) for m in il]
    if special:
        assert n >= 3
        labs[0] = np.zeros(0, dtype=np.int64)
        il[n // 2], labs[n // 2] = 1024, rng.integers(0, 4, size=255)
        il[n - 1], labs[n - 1] = 64, np.ones(40, dtype=np.int64)
    return x, il, labs


def probs(flat, x, dilations):
    import torch
    t = _tensors(np.asarray(flat), dilations, torch.float64)
    with torch.no_grad():
        return torch.softmax(forward_logits(t, torch.as_tensor(np.asarray(x, dtype=np.float64)), dilations), -1).numpy()


def logits(flat, x, dilations):
    import torch
    t = _tensors(np.asarray(flat), dilations, torch.float64)
    with torch.no_grad():
        return forward_logits(t, torch.as_tensor(np.asarray(x, dtype=np.float64)), dilations).numpy()


def ctc_grad_z(z, input_len, labels):
    """(mean loss, dL/dz [B, T, 5]) of logits z by autograd, fp64"""
    import torch
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    loss = keras_ctc_mean(zt, input_len, labels)
    loss.backward()
    return float(loss.detach()), zt.grad.numpy()


def brute_force_loss(z, n, label):
    """-log sum over every path of the first n rows that collapses to label of prod p; fp64, small n only"""
    y = np.exp(z - z.max(-1, keepdims=True))
    y /= y.sum(-1, keepdims=True)
    q = y[:n] + EPS
    p = q / q.sum(-1, keepdims=True)
    total = 0.0
    for path in itertools.product(range(5), repeat=n):
        out, prev = [], None
        for c in path:
            if c != BLANK and c != prev:
                out.append(c)
            prev = c
        if out == list(label):
            total += float(np.prod([p[t, c] for t, c in enumerate(path)]))
    return -np.log(total) if total > 0 else np.inf


def keras_adam(w, g, m, v, t, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7):
    """TF 2.4 ApplyAdam in float32, t counted from 1: (w, m, v) after one step"""
    f = np.float32
    w, g, m, v = (np.asarray(a, dtype=f) for a in (w, g, m, v))
    b1, b2, lr_, eps = f(beta1), f(beta2), f(lr), f(epsilon)
    b1p, b2p = f(b1 ** f(t)), f(b2 ** f(t))
    alpha = f(lr_ * np.sqrt(f(1) - b2p) / (f(1) - b1p))
    m = m + (g - m) * (f(1) - b1)
    v = v + (g * g - v) * (f(1) - b2)
    w = w - (m * alpha) / (np.sqrt(v) + eps)
    return w, m, v
