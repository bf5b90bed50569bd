"""A plain NumPy float64 restatement of the TCN forward (the graph in the header of radian_amd/csrc/forward.hip), the centred
log-ratio metric, the CPU-float32 yardstick, and a catalogue of named faults modelled on how the HIP kernels can go wrong.

It shares no code with the library or with oracle/radian_oracle.c: the weights come as the flat float32 array in
`weights.tensor_shapes` order, every product is a float64 matmul, and the values the kernels STORE between layers (the mid
activation of a block, the block's output, the Dense(128) rows) are rounded to float32 -- in the split modes to what those modes
carry (f16x3: hi + lo halves, 22 bits; bf16x3: hi + mid + lo, every float32 bit).

  mode "exact"   a . w, operands float32
  mode "f16x3"   hi = f16(v), lo = f16(v - hi); a . w = ah.wh + ah.wl + al.wh; conv / Dense(128) kernels scaled per tensor by the
                 power of two that brings max|w| into [512, 1024) before the split (model.hip split_scale), the sum scaled back
  mode "bf16x3"  hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid); a . w = ah.bh + (ah.bm + am.bh) + (ah.bl + am.bm + al.bh)
In every mode block 0's first conv (one input channel), the 1x1 match conv and Dense(5) are plain float32 operands (the kernels
compute them on the vector unit), and the residual is added to the carried value of the block input.

Faults (`catalogue`) change one thing in one layer; `logits64(..., fault=f, cache=c)` re-evaluates only the windows the fault touches,
from the fault's block on, out of the block inputs a clean run left in `c`."""
import numpy as np

C, K, H, NCLS = 256, 3, 128, 5
MODES = ("exact", "f16x3", "bf16x3")
P_MIN = 2.0 ** -10          # smallest reference probability a soft-head case may hold


# ---------------------------------------------------------------------------------------------------------------- number formats
def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _bf16(v32):
    """float32 -> nearest bf16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _split(v64, mode, rounded=True):
    """the terms a mode carries for a value: tuple of float64 arrays whose sum is the carried value"""
    if not rounded:
        return (np.asarray(v64, dtype=np.float64),)
    v = _f32(v64)
    if mode == "exact":
        return (v.astype(np.float64),)
    if mode == "f16x3":
        hi = v.astype(np.float16).astype(np.float32)
        lo = (v - hi).astype(np.float16)
        return (hi.astype(np.float64), lo.astype(np.float64))
    if mode == "bf16x3":
        hi = _bf16(v)
        r1 = v - hi
        mid = _bf16(r1)
        lo = _bf16(r1 - mid)
        return (hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64))
    raise ValueError(mode)


def _round_bits(v, bits=16):
    """v rounded to `bits` significant bits (a split operand that lost its low term)"""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(np.rint(m * 2.0 ** bits) / 2.0 ** bits, e)


def _weight_terms(w32, mode, lo16=False):
    """(terms, inv_scale) of a conv / Dense(128) kernel"""
    w = np.asarray(w32, dtype=np.float32)
    if lo16:
        return (_round_bits(w),), 1.0
    if mode == "f16x3":
        mx = float(np.abs(w).max())
        sc = 1.0
        if mx > 0 and np.isfinite(mx):
            sc = 2.0 ** (10 - int(np.frexp(mx)[1]))
        return _split(w.astype(np.float64) * sc, mode), 1.0 / sc
    return _split(w, mode), 1.0


def _dot(a, w):
    """the products a mode keeps, summed in float64: a, w = term tuples, a [..., n] . w [n, m]"""
    lead = a[0].shape[:-1]
    a = tuple(np.ascontiguousarray(t).reshape(-1, t.shape[-1]) for t in a)      # one matrix product for all windows
    if len(a) == 1 or len(w) == 1:
        out = _total(a) @ _total(w)
    elif len(a) == 2:
        out = a[0] @ (w[0] + w[1]) + a[1] @ w[0]
    else:
        out = a[0] @ (w[0] + w[1] + w[2]) + a[1] @ (w[0] + w[1]) + a[2] @ w[0]
    return out.reshape(lead + (out.shape[-1],))


# ---------------------------------------------------------------------------------------------------------------- faults
class Fault:
    """One thing wrong in one place.  kind:
      drop   tap `tap`, input channels `ci`, left out of the rows `rows(T)`           (conv `conv` of block `block`)
      bias   the bias left out for output channels `co` of the rows                    (conv)
      pad    the causal padding read as the segment's first row instead of zero       (conv)
      elem   one output element (row `rows(T)[0]`, the channel with the largest pre-activation) zeroed   (conv)
      lo16   both operands keep 16 significant bits                                   (conv; block None = every conv and Dense(128))
      nores  the residual (identity, or block 0's match conv) not added on the rows   (block)
      swap   Dense(5) outputs 1 and 2 exchanged on the rows                           (head)
    window: None = every window, k = the window with the k-th largest valid length.  structural: not a precision fault.
    min_rows: kept rows a case needs before the fault's distance means anything (precision faults: an rms over a handful of rows)."""

    def __init__(self, name, kind, block=None, conv=None, rows=None, tap=None, ci=slice(None), co=slice(None), window=None, structural=True,
                 min_rows=0):
        self.name, self.kind, self.block, self.conv, self.rows = name, kind, block, conv, rows
        self.tap, self.ci, self.co, self.window, self.structural, self.min_rows = tap, ci, co, window, structural, min_rows

    def __repr__(self):
        return self.name

    def rows_in(self, T, valid):
        """the rows of a window of T rows (valid of them kept) the fault changes first, as an index array"""
        r = np.arange(T) if self.rows is None else np.asarray(self.rows(T, valid), dtype=np.int64)
        return r[(r >= 0) & (r < T)]


def _every(period, phase, lo=0):
    return lambda T, valid: np.array([t for t in range(phase, T, period) if t >= lo], dtype=np.int64)


def _span(a, b):
    return lambda T, valid: np.arange(a, min(b, T))


def catalogue(dilations):
    """the named faults for a model with these dilations (tiles are 128 rows, sub-tiles 32, K-chunks 16 channels x one tap)"""
    nb = len(dilations)
    last, mid, second = nb - 1, nb // 2, min(1, nb - 1)
    d_last = dilations[last]
    return [
        Fault("tap_dropped_first_row_of_every_tile", "drop", last, 0, _every(128, 0, lo=d_last), tap=1),
        Fault("tap_dropped_last_row_of_every_tile", "drop", mid, 1, _every(128, 127), tap=0),
        Fault("tap_dropped_row_31_of_a_subtile", "drop", second, 0, _span(31, 32), tap=1, window=0),
        Fault("tap_dropped_row_32_of_a_subtile", "drop", second, 1, _span(32, 33), tap=0, window=0),
        Fault("k_chunk_lost_for_a_subtile", "drop", mid, 0, _span(32, 64), tap=2, ci=slice(80, 96), window=1),
        Fault("k_chunk_lost_for_a_tile", "drop", last, 1, _span(0, 128), tap=2, ci=slice(144, 160), window=2),
        Fault("padding_read_as_first_row_block_0", "pad", 0, 0),
        Fault("padding_read_as_first_row_last_block", "pad", last, 0),
        Fault("one_output_element_zeroed", "elem", mid, 1, lambda T, valid: np.array([min(valid - 1, 40)]), window=0),
        Fault("bias_missing_channels_192_255_of_a_tile", "bias", second, 1, _span(0, 128), co=slice(192, 256), window=1),
        Fault("residual_add_skipped_for_a_subtile", "nores", max(mid, 1), None, _span(32, 64), window=2),
        Fault("match_conv_skipped_for_a_tile", "nores", 0, None, _span(0, 128), window=0),
        Fault("low_term_dropped_in_one_conv", "lo16", mid, 1, structural=False, min_rows=90),
        Fault("low_term_dropped_in_every_layer", "lo16", None, None, structural=False),
        Fault("dense5_outputs_swapped_on_a_row_class", "swap", nb, None, _every(32, 31)),
    ]


def fault_window(fault, valid):
    """index of the window a one-window fault touches: the fault.window-th by valid length, longest first (stable)"""
    order = np.argsort(-np.asarray(valid), kind="stable")
    return int(order[fault.window])


def fault_reaches(fault, T, valid):
    """whether the fault changes a row the comparison keeps"""
    valid = np.asarray(valid)
    ws = range(len(valid)) if fault.window is None else [fault_window(fault, valid)]
    if int(valid.sum()) < fault.min_rows:
        return False
    if fault.kind in ("pad", "lo16"):
        return True
    return any((fault.rows_in(T, int(valid[w])) < valid[w]).any() for w in ws)


# ---------------------------------------------------------------------------------------------------------------- the graph
def _tensors(flat, dilations):
    from radian_amd import weights
    t, o = {}, 0
    for name, shape in weights.tensor_shapes(dilations):
        n = int(np.prod(shape))
        t[name] = np.asarray(flat[o:o + n], dtype=np.float32).reshape(shape)
        o += n
    assert o == flat.size
    return t


def _total(terms):
    return terms[0] if len(terms) == 1 else sum(terms[1:], terms[0])


def _taps(a, d, pad_first):
    """a [B, T, c] -> [B, T, 3 c]: columns j c .. of row t hold row t - (K - 1 - j) d, tap j's input; rows before the segment are zero
    (or, the `pad` fault, the segment's first row)"""
    B, T, c = a.shape
    X = np.zeros((B, T, K * c))
    for j in range(K):
        s = (K - 1 - j) * d
        if s < T:
            X[:, s:, j * c:(j + 1) * c] = a[:, :T - s]
        if pad_first and s > 0:
            X[:, :min(s, T), j * c:(j + 1) * c] = a[:, :1]
    return X


def _conv(a, kernel, bias, d, mode, f, T, valid):
    """causal dilated conv of the term tuple a ([B, T, cin] each) -> float64 pre-activations [B, T, 256]: out[t] = b + sum_j W[j] . a[t -
    (K - 1 - j) d] as ONE product over (tap, channel); f = the fault of THIS conv"""
    kind = f.kind if f is not None else None
    cin = kernel.shape[1]
    plain = cin == 1                                  # block 0's first conv: float32 operands on the vector unit in every mode
    lo16 = kind == "lo16"
    if lo16:
        a = (_round_bits(_total(a)),)
    w, inv = _weight_terms(kernel.reshape(K * cin, C), "exact" if plain else mode, lo16)
    xs = tuple(_taps(t, d, kind == "pad") for t in a)
    out = _dot(xs, w)
    if inv != 1.0:
        out *= inv
    rows = f.rows_in(T, valid) if kind in ("drop", "bias", "elem") else None
    if kind == "drop" and len(rows):
        cols = np.arange(f.tap * cin, (f.tap + 1) * cin)[f.ci]
        out[:, rows] -= _dot(tuple(t[:, rows][:, :, cols] for t in xs), tuple(t[cols] for t in w)) * inv
    out += bias.astype(np.float64)
    if kind == "bias" and len(rows):
        sub = np.zeros(C)
        sub[f.co] = bias[f.co]
        out[:, rows] -= sub
    if kind == "elem":
        r = int(rows[0])
        c = int(np.argmax(out[0, r]))
        assert out[0, r, c] > 0, "the zeroed element must have a positive pre-activation"
        out[0, r, c] = 0.0
    return out


def _blocks(t, x, v, dilations, mode, rounded, fault, first_block, cache, valid):
    """blocks first_block.. and the head: v = term tuple of the block input ([B, T, 256]; for block 0 the raw samples [B, T, 1])"""
    T = x.shape[1]
    nb = len(dilations)
    relu = lambda z: np.maximum(z, 0.0)
    every = fault is not None and fault.kind == "lo16" and fault.block is None

    def here(b, conv):
        if fault is None:
            return None
        if every and conv is not None:
            return fault
        return fault if (fault.block == b and fault.conv == conv) else None

    for b in range(first_block, nb):
        d = dilations[b]
        p = f"tcn/residual_block_{b}/"
        if cache is not None:
            cache["block", b] = v
        x1 = _split(relu(_conv(v, t[p + "conv1D_0/kernel"], t[p + "conv1D_0/bias"], d, mode, here(b, 0), T, valid)), mode, rounded)
        x1 = relu(_conv(x1, t[p + "conv1D_1/kernel"], t[p + "conv1D_1/bias"], d, mode, here(b, 1), T, valid))
        if b == 0:
            res = x[:, :, None].astype(np.float64) * t[p + "matching_conv1D/kernel"].reshape(C).astype(np.float64) \
                + t[p + "matching_conv1D/bias"].astype(np.float64)
        else:
            res = _total(v)
        f = here(b, None)
        if f is not None and f.kind == "nores":
            res = res.copy()
            res[:, f.rows_in(T, valid)] = 0.0
        v = _split(relu(res + x1), mode, rounded)
    if cache is not None:
        cache["block", nb] = v
    lo16 = every
    if lo16:
        v = (_round_bits(_total(v)),)
    w1, inv = _weight_terms(t["dense/kernel"], mode, lo16)
    h = relu(_dot(v, w1) * inv + t["dense/bias"].astype(np.float64))
    if rounded:
        h = _f32(h).astype(np.float64)
    z = h @ t["dense_1/kernel"].astype(np.float64) + t["dense_1/bias"].astype(np.float64)
    if fault is not None and fault.kind == "swap":
        r = fault.rows_in(T, valid)
        z[:, r, 1], z[:, r, 2] = z[:, r, 2].copy(), z[:, r, 1].copy()
    return z


def logits64(flat, x, dilations, mode="exact", fault=None, rounded=True, cache=None, valid=None):
    """[B, T] float32 windows -> [B, T, 5] float64 logits, every window causally zero-padded at its own start.
    rounded=False keeps float64 between layers (exact mode only).  cache: a dict a clean run fills with its block inputs and logits and
    a faulted run restarts from.  valid [B]: rows of each window the comparison keeps (only used to place one-window faults)."""
    if mode not in MODES:
        raise ValueError(mode)
    assert rounded or mode == "exact"
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, T = x.shape
    valid = np.full(B, T, dtype=np.int64) if valid is None else np.asarray(valid, dtype=np.int64)
    t = _tensors(np.asarray(flat), dilations)
    if fault is None:
        z = _blocks(t, x, (x[:, :, None].astype(np.float64),), dilations, mode, rounded, None, 0, cache, int(valid.max()))
        if cache is not None:
            cache["logits"] = z
        return z
    ws = np.arange(B) if fault.window is None else np.array([fault_window(fault, valid)])
    first = 0 if fault.block is None else min(fault.block, len(dilations))
    if cache is not None and "logits" in cache:
        z = cache["logits"].copy()
        v = tuple(term[ws] for term in cache["block", first])
    else:
        z = None if len(ws) == B else logits64(flat, x, dilations, mode, None, rounded)
        v, first = (x[ws][:, :, None].astype(np.float64),), 0
    zw = _blocks(t, x[ws], v, dilations, mode, rounded, fault, first, None, int(valid[ws].min()) if fault.window is not None else T)
    if z is None:
        return zw
    z[ws] = zw
    return z


# ---------------------------------------------------------------------------------------------------------------- the metric
def softmax64(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def clr(p):
    """centred log-ratio of probability rows: u_c = ln p_c - mean_c ln p_c (= logit - row mean), float64"""
    lp = np.log(np.asarray(p, dtype=np.float64))
    return lp - lp.mean(axis=-1, keepdims=True)


def keep_mask(B, T, valid=None):
    """[B, T] bool: the rows a comparison keeps"""
    valid = np.full(B, T) if valid is None else np.asarray(valid)
    return np.arange(T)[None, :] < valid[:, None]


def distance(p, expected_clr, valid=None):
    """(max, rms) of |clr(p) - E| over the kept rows"""
    B, T = expected_clr.shape[:2]
    keep = keep_mask(B, T, valid)
    d = clr(np.asarray(p)[keep]) - expected_clr[keep]
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def yardstick(oracle, flat, x, dilations, valid=None, ref=None):
    """(max, rms) of |clr(oracle.tcn_forward) - clr(softmax(logits64))|: what a plain float32 CPU forward of the same graph differs by
    from the float64 statement, on this input.  ref = the exact-mode logits64 of the same input where the caller has them."""
    z = logits64(flat, x, dilations) if ref is None else ref
    p32 = oracle.tcn_forward(np.asarray(flat), np.ascontiguousarray(x, dtype=np.float32), dilations=tuple(dilations))
    return distance(p32, clr(softmax64(z)), valid)


def soft_weights(seed, dilations):
    """He-normal weights with the last Dense kernel scaled by 0.05: logit spans of a few units, no saturated class"""
    from radian_amd import weights
    return weights.synthetic_weights(seed=seed, dilations=tuple(dilations), head_gain=0.05)


# ---------------------------------------------------------------------------------------------------------------- the cases
DEFAULT = (1, 2, 4, 8, 16, 32)
WEIGHT_SETS = ((1234, DEFAULT), (77, DEFAULT), (3, (2, 4, 1)), (3, (16, 1)))      # (seed, dilations)
WINDOW_T = (1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300)
READ_LENGTHS = (1, 33, 129, 700, 1024, 1500, 2100)
STREAM_GEOMETRIES = ((1024, 512), (300, 77))


def window_case(T):
    """three windows of T samples: one starts with 40 zeros, one is zero from two thirds on"""
    rng = np.random.default_rng(1000 + T)
    x = np.clip(rng.normal(size=(3, T)), -4, 4).astype(np.float32)
    x[1, :40] = 0.0
    x[2, (2 * T) // 3:] = 0.0
    return x


def reads_case():
    rng = np.random.default_rng(2024)
    return [np.clip(rng.normal(size=n), -4, 4).astype(np.float32) for n in READ_LENGTHS]


def read_windows(sig, chunk, step):
    """the windows of one read as the reference cuts them -- every full window at multiples of step, then one zero-padded window with
    what is left (always present) -- and the rows of each the pad trim keeps"""
    n = len(sig)
    nw = (0 if n < chunk else (n - chunk) // step + 1) + 1
    padded = np.zeros((nw - 1) * step + chunk, dtype=np.float32)
    padded[:n] = sig
    win = np.stack([padded[i * step:i * step + chunk] for i in range(nw)])
    valid = np.array([min(chunk, n - i * step) for i in range(nw)], dtype=np.int64)
    return win, valid


def stream_case(chunk, step):
    """(reads, windows [nW, chunk], valid [nW], windows per read)"""
    reads = reads_case()
    cut = [read_windows(s, chunk, step) for s in reads]
    return reads, np.concatenate([c[0] for c in cut]), np.concatenate([c[1] for c in cut]), [len(c[1]) for c in cut]


def cases():
    """[(name, x [B, T], valid [B])]: every input the GPU test compares"""
    out = [(f"windows_T{T}", window_case(T), np.full(3, T, dtype=np.int64)) for T in WINDOW_T]
    for chunk, step in STREAM_GEOMETRIES:
        _, win, valid, _ = stream_case(chunk, step)
        out.append((f"reads_{chunk}_{step}", win, valid))
    return out
