"""Packed window heads (rd_set_head_pack): the chunk-mode streamed forward with its window heads run as packed row classes
that leave out the conv taps lying in the window's zero left-padding must be BIT-IDENTICAL to the same forward with head tiles, and to the
windowed forward -- a left-out product is fma(0, w, acc)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK, STEP = 1024, 512


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend, weights
    b = Backend(0)
    b.load_weights(weights.synthetic_weights(seed=1234))
    yield b
    b.close()


def _reads(rng, lengths):
    return [np.clip(rng.normal(size=n), -4, 4).astype(np.float32) for n in lengths]


def _windowed(be, sig, chunk, step):
    """the windowed forward of one read, rows behind a window's valid length zeroed as forward_reads leaves them"""
    from radian_amd.preprocess import get_windows
    w, pad = get_windows(sig, chunk, step)
    p = be.forward(w.astype(np.float32))
    if pad > 0:
        p[-1, chunk - pad:] = 0
    return p


def _packed_tiles(chunk, step, lengths):
    """packed workgroup tiles of one forward, from the class rule: per conv layer behind block 0, ceil(heads x L / 128) for
    L = h - 2d, d, d (h = the layer's head length, capped at the chunk length)"""
    heads = sum(max(0, (n - chunk) // step + 1 if n >= chunk else 0) for n in lengths)
    for n in lengths:   # a last window without rows has no head
        if n >= chunk and (n - chunk) % step == 0 and chunk - step <= 0:
            heads -= 1
    if heads == 0:
        return 0
    tiles, H = 0, 4
    for d in (2, 4, 8, 16, 32):
        for h in (H + 2 * d, H + 4 * d):
            h = min(h, chunk)
            for L in (h - min(2 * d, h), min(2 * d, h) - min(d, h), min(d, h)):
                tiles += -(-heads * L // 128)
        H += 4 * d
    return tiles


def _both(be, sigs, chunk, step):
    """forward_reads with packed heads and with head tiles; the packed forward must have launched the packed tiles the class rule gives"""
    be.set_head_pack(1)
    assert be.head_pack_active()
    on = be.forward_reads(sigs, chunk, step)
    assert be.head_pack_tiles() == _packed_tiles(chunk, step, [len(s) for s in sigs])
    be.set_head_pack(0)
    assert not be.head_pack_active()
    off = be.forward_reads(sigs, chunk, step)
    assert be.head_pack_tiles() == 0
    be.set_head_pack(1)
    return on, off


GEOMETRIES = {
    "two_reads": (CHUNK, STEP, [1536, 2049]),
    "short_last_window": (CHUNK, STEP, [CHUNK + STEP + 5]),              # last window shorter than the 252-row halo
    "three_heads": (CHUNK, STEP, [CHUNK + 2 * STEP]),                    # class A (d rows per head) straddles DMA pieces and tiles
    "five_heads": (CHUNK, STEP, [CHUNK + STEP, CHUNK + 2 * STEP]),
    "four_heads": (CHUNK, STEP, [CHUNK + 3 * STEP]),                     # classes A and B of d = 32 fill one tile exactly
    "seven_heads": (CHUNK, STEP, [CHUNK + 2 * STEP, CHUNK + 3 * STEP + 100]),
    "step_is_chunk": (CHUNK, CHUNK, [3 * CHUNK + 40, CHUNK + 1]),
    "step_772": (CHUNK, 772, [4000, 1800]),
    "step_773": (CHUNK, 773, [4000, 1800]),
    "heads_longer_than_step": (300, 7, [420, 331]),
    "one_window_reads": (CHUNK, STEP, [1000, 37, 1023, 1]),              # no heads: zero packed tiles
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_packed_equals_unpacked_and_windowed(be, name):
    chunk, step, lengths = GEOMETRIES[name]
    rng = np.random.default_rng(sum(lengths) + step)
    sigs = _reads(rng, lengths)
    on, off = _both(be, sigs, chunk, step)
    for r, sig in enumerate(sigs):
        assert on[r].shape == off[r].shape
        assert np.array_equal(on[r], off[r]), (name, r)
        assert np.array_equal(on[r], _windowed(be, sig, chunk, step)), (name, r)


def _poke(flat, name, index, value):
    from radian_amd import weights
    out = flat.copy()
    o = 0
    for n, shape in weights.tensor_shapes():
        size = int(np.prod(shape))
        if n == name:
            out[o + index] = value
            return out
        o += size
    raise KeyError(name)


@pytest.mark.parametrize("case", ["inf_kernel", "neg_zero_bias"])
def test_bad_weights_fall_back_to_head_tiles(case):
    """one inf in a block-3 conv kernel / one -0.0 conv bias: a skipped product would not be a no-op, so the context does not pack"""
    from radian_amd import Backend, weights
    flat = weights.synthetic_weights(seed=1234)
    if case == "inf_kernel":
        bad = _poke(flat, "tcn/residual_block_3/conv1D_1/kernel", 12345, np.float32(np.inf))
    else:
        bad = _poke(flat, "tcn/residual_block_2/conv1D_0/bias", 17, np.float32(-0.0))
        assert (bad == 0).sum() == 1 and np.signbit(bad[bad == 0]).all()
    rng = np.random.default_rng(5)
    sigs = _reads(rng, [1536, 2049])
    be = Backend(0)
    try:
        be.load_weights(bad)
        assert not be.head_pack_active()          # set_head_pack is still 1: the weights turn the packed path off
        got = be.forward_reads(sigs, CHUNK, STEP)
        assert be.head_pack_tiles() == 0
        be.set_head_pack(0)
        ref = be.forward_reads(sigs, CHUNK, STEP)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r, equal_nan=True)
        be.set_head_pack(1)
        be.load_weights(flat)                     # good weights again: packed
        assert be.head_pack_active()
        be.forward_reads(sigs, CHUNK, STEP)
        assert be.head_pack_tiles() > 0
    finally:
        be.close()


def test_other_precisions_and_shapes_do_not_pack(be):
    try:
        be.set_precision("f16x3")
        assert not be.head_pack_active()
        be.set_precision("fp32")
        be.set_conv_shape(1)
        assert not be.head_pack_active()
    finally:
        be.set_precision("fp32")
        be.set_conv_shape(0)
    assert be.head_pack_active()


def test_pipeline_labels_with_and_without_packing(be):
    """rd_pipe_submit_reads on two lanes: one 8-read batch, labels with packing on == off"""
    rng = np.random.default_rng(11)
    n_reads, N, W = 8, 2048, 10
    batch = np.stack(_reads(rng, [N] * n_reads))
    read_off = np.arange(n_reads + 1, dtype=np.int64) * N
    nwin = n_reads * be.count_windows(N, CHUNK, STEP)
    d = be.dev_alloc(batch.nbytes)
    be.h2d(d, batch)
    res = {}
    try:
        be.pipe_set_lanes(2)
        for on in (1, 0):
            be.set_head_pack(on)
            outs = [(np.zeros((nwin, CHUNK), dtype=np.uint8), np.full(nwin, -1, dtype=np.int32)) for _ in range(2)]   # one batch on each lane
            for lab, ln in outs:
                be.pipe_submit_reads(d, read_off, n_reads, CHUNK, STEP, W, lab, ln)
            be.pipe_flush()
            res[on] = outs
    finally:
        be.set_head_pack(1)
        be.pipe_flush()
        be.dev_free(d)
    for k in range(2):
        assert (res[1][k][1] >= 0).all()
        assert np.array_equal(res[1][k][1], res[0][k][1]) and np.array_equal(res[1][k][0], res[0][k][0])
    assert np.array_equal(res[1][0][0], res[1][1][0])
