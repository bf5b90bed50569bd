"""CPU restatement of the training contract of rd_train_* (radian_amd/csrc/train.hip): the graph of
model.py:52-89 in stock PyTorch operators with autograd, Keras's loss chain (softmax -> log(y + 1e-7) -> TF's log-softmax -> CTC,
blank = 4, the batch mean) through torch.nn.functional.ctc_loss, and TF 2.4's Adam in numpy float32.  Test infrastructure."""
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


def forward_logits(t, x, dilations):
    """z [B, T, 5] (the last Dense's output) of windows x [B, T]"""
    import torch
    import torch.nn.functional as F

    def causal(v, kernel, bias, d):
        w = kernel.permute(2, 1, 0)
        return F.conv1d(F.pad(v, ((kernel.shape[0] - 1) * d, 0)), w, bias, dilation=d)

    v = x[:, None, :]
    for b, d in enumerate(dilations):
        p = f"tcn/residual_block_{b}/"
        h = torch.relu(causal(v, t[p + "conv1D_0/kernel"], t[p + "conv1D_0/bias"], d))
        h = torch.relu(causal(h, t[p + "conv1D_1/kernel"], t[p + "conv1D_1/bias"], d))
        res = causal(v, t[p + "matching_conv1D/kernel"], t[p + "matching_conv1D/bias"], 1) if b == 0 else v
        v = torch.relu(res + h)
    h = torch.relu(v.transpose(1, 2) @ t["dense/kernel"] + t["dense/bias"])
    return h @ t["dense_1/kernel"] + t["dense_1/bias"]


def keras_ctc_mean(z, input_len, labels):
    """Keras ctc_batch_cost on softmax(z), infeasible windows counted as zero, summed and divided by the batch size"""
    import torch
    import torch.nn.functional as F
    y = torch.softmax(z, dim=-1)
    lp = torch.log_softmax(torch.log(y + EPS), dim=-1)
    n = z.shape[0]
    tg = [torch.as_tensor(np.asarray(l, dtype=np.int64)) for l in labels]
    flat = torch.cat(tg) if sum(len(a) for a in tg) else torch.zeros(0, dtype=torch.int64)
    loss = F.ctc_loss(lp.transpose(0, 1), flat, torch.as_tensor(np.asarray(input_len, dtype=np.int64)),
                      torch.as_tensor([len(a) for a in tg], dtype=torch.int64), blank=BLANK, reduction="sum", zero_infinity=True)
    return loss / n


def loss_and_grad(flat, x, input_len, labels, dilations, dtype=None):
    """(mean loss, flat gradient in load_weights order, {name: grad}) by autograd; dtype torch.float64 (default) or float32"""
    import torch
    dtype = dtype or torch.float64
    t = _tensors(np.asarray(flat), dilations, dtype)
    z = forward_logits(t, torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dtype), dilations)
    loss = keras_ctc_mean(z, input_len, labels)
    loss.backward()
    grads = {k: v.grad.detach().to(torch.float64).numpy().ravel() for k, v in t.items()}
    from radian_amd import weights
    return float(loss.detach()), np.concatenate([grads[k] for k, _ in weights.tensor_shapes(dilations)]), grads


def probs(flat, x, dilations):
    import torch
    t = _tensors(np.asarray(flat), dilations, torch.float64)
    with torch.no_grad():
        return torch.softmax(forward_logits(t, torch.as_tensor(np.asarray(x, dtype=np.float64)), dilations), -1).numpy()


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
