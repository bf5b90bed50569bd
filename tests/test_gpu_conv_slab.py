"""Slab tiles of the exact-fp32 conv launches behind block 0 (rd_set_conv_slab): a workgroup tile that lies wholly inside one
segment stages the 128 + 2 d input rows its three taps share once per channel slice instead of 128 shifted rows per tap.  Products and their
order are unchanged, so every output must be BIT-IDENTICAL (compared as uint32, not under IEEE equality) with the switch on and off.  Every
case also holds the forward's slab-tile count (rd_conv_slab_tiles) to the count the tile rule gives for its lists -- zero where no tile can
qualify -- so no case passes without the path having run.

The expected count: a layer's list is the 32-row sub-tiles of its segments in order, cut into workgroup tiles of four; a tile is a slab tile
when its four sub-tiles are consecutive pieces of one segment and t0 + 128 <= the segment's length.  Every conv launch behind block 0 whose
dilation is <= 32 runs the list (two per block).  Head tiles never qualify for the models here: a head's residual rows switch to the read's
stream after the halo in front of its block, which stays below 128 rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _forward_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WSETS = ((1234, R.DEFAULT), (3, (2, 4, 1)), (3, (16, 1)))      # (2, 4, 1): slot keys differ per tap, order not monotone
WSET_IDS = ["seed%d_d%s" % (s, "_".join(map(str, d))) for s, d in WSETS]
WINDOW_T = (127, 128, 129, 256, 300)
READ_LENGTHS = (128, 129, 255, 256, 257, 1500, 2100)
GEOMETRIES = ((1024, 512), (300, 77))


def _slab_launches(dilations):
    return 2 * sum(1 for d in dilations[1:] if d <= 32)


def _list_slab_tiles(seg_lens):
    """slab tiles of a list that holds these segments' sub-tiles in order (whatever follows them in the list cannot complete a slab tile)"""
    subs = [(s, t0, n) for s, n in enumerate(seg_lens) for t0 in range(0, n, 32)]
    tiles = 0
    for k in range(0, len(subs) - 3, 4):
        s, t0, n = subs[k]
        if all(subs[k + j][0] == s for j in range(4)) and t0 + 128 <= n:
            tiles += 1
    return tiles


def test_tile_rule_of_the_test():
    """the rule above on the window lengths the cases turn on"""
    assert _list_slab_tiles([127] * 3) == 0
    assert _list_slab_tiles([128]) == 1 and _list_slab_tiles([128] * 3) == 3
    assert _list_slab_tiles([300]) == 2          # t0 = 0 and t0 = 128; [256, 300) is a partial tile
    assert _list_slab_tiles([300] * 3) == 5      # windows share tiles: window 1's tiles start at t0 = 64 (one interior) and 192


@pytest.fixture(scope="module")
def backends():
    """one context per weight set, opened on first use; the switch is put back to what the context came with"""
    from radian_amd import Backend
    open_ = {}

    def get(wi):
        if wi not in open_:
            b = Backend(0)
            b.load_weights(R.soft_weights(*WSETS[wi]), WSETS[wi][1])
            open_[wi] = (b, b.conv_slab_active())
        return open_[wi][0]
    try:
        yield get
    finally:
        for b, was in open_.values():
            b.set_conv_slab(was)
            b.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _on_off(be, run, expect_tiles):
    """run() with the switch on, then off: the outputs of both, the counts checked"""
    was = be.conv_slab_active()
    try:
        be.set_conv_slab(1)
        assert be.conv_slab_active()
        on = run()
        n_on = be.conv_slab_tiles()
        be.set_conv_slab(0)
        assert not be.conv_slab_active()
        off = run()
        n_off = be.conv_slab_tiles()
    finally:
        be.set_conv_slab(was)
    print(f"slab tiles: {n_on} with the switch on (expected {expect_tiles}), {n_off} off")
    assert n_off == 0
    assert n_on == expect_tiles
    return on, off


def _signals(seed, lengths):
    rng = np.random.default_rng(seed)
    return [np.clip(rng.normal(size=n), -4, 4).astype(np.float32) for n in lengths]


@pytest.mark.parametrize("T", WINDOW_T)
@pytest.mark.parametrize("wi", range(len(WSETS)), ids=WSET_IDS)
def test_windowed_forward_bits(backends, wi, T):
    """three windows of T rows: none at T = 127; at T = 128 one per window, t0 = 0, the whole halo in the padding; at T = 300 tiles at
    t0 = 64 and 128 whose halo of 2 x 32 rows lies inside the window"""
    be = backends(wi)
    x = np.stack(_signals(500 + T, [T] * 3))
    expect = _list_slab_tiles([T] * 3) * _slab_launches(WSETS[wi][1])
    assert (expect == 0) == (T == 127)
    on, off = _on_off(be, lambda: be.forward(x), expect)
    assert np.array_equal(_bits(on), _bits(off))


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["%d_%d" % g for g in GEOMETRIES])
@pytest.mark.parametrize("wi", range(len(WSETS)), ids=WSET_IDS)
def test_streamed_forward_bits(backends, wi, geom):
    """ragged reads, chunk plan: slab tiles, a read's last partial tile, the mixed tile, head tiles / packed classes in one launch"""
    be = backends(wi)
    chunk, step = geom
    sigs = _signals(77, READ_LENGTHS)
    expect = _list_slab_tiles(READ_LENGTHS) * _slab_launches(WSETS[wi][1])
    assert expect > 0
    on, off = _on_off(be, lambda: be.forward_reads(sigs, chunk, step), expect)
    for a, b in zip(on, off):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("fuse", (0, 1))
@pytest.mark.parametrize("pack", (0, 1))
def test_switch_combinations_bits(backends, fuse, pack):
    """first-conv fusion x head packing on the (300, 77) reads: with head tiles in the list the count stays the stream tiles'"""
    be = backends(0)
    sigs = _signals(78, READ_LENGTHS)
    expect = _list_slab_tiles(READ_LENGTHS) * _slab_launches(WSETS[0][1])
    try:
        be.set_conv_fuse(fuse)
        be.set_head_pack(pack)
        on, off = _on_off(be, lambda: be.forward_reads(sigs, 300, 77), expect)
        assert (be.head_pack_tiles() > 0) == bool(pack)
    finally:
        be.set_conv_fuse(1)
        be.set_head_pack(1)
    for a, b in zip(on, off):
        assert np.array_equal(_bits(a), _bits(b))


def test_global_plan_labels(backends):
    """the global plan (one stream per read, one list for every layer) through the same two kernels.  No entry point hands back a global-mode
    forward's rows, so the labels of its beam search are compared"""
    be = backends(0)
    sigs = _signals(79, READ_LENGTHS)
    expect = _list_slab_tiles(READ_LENGTHS) * _slab_launches(WSETS[0][1])
    on, off = _on_off(be, lambda: be.basecall_reads_global(sigs, 1024, 512, 6, False), expect)
    assert len(on) == len(off) == len(sigs)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


def test_other_precisions_and_shapes_have_no_slab_path(backends):
    be = backends(0)
    was = be.conv_slab_active()
    try:
        be.set_conv_slab(1)
        be.set_precision("f16x3")
        assert not be.conv_slab_active()
        be.set_precision("fp32")
        be.set_conv_shape(1)
        assert not be.conv_slab_active()
        be.forward(np.stack(_signals(80, [256] * 2)))
        assert be.conv_slab_tiles() == 0
    finally:
        be.set_precision("fp32")
        be.set_conv_shape(0)
        be.set_conv_slab(was)


def test_pipelined_chunk_step_labels(backends):
    """one pipelined chunk step (rd_pipe_submit_reads): 4 reads x 2100 samples, beam 10 -- labels and lengths with the switch on == off"""
    be = backends(0)
    chunk, step, W = 1024, 512, 10
    n_reads, N = 4, 2100
    batch = np.stack(_signals(81, [N] * n_reads))
    read_off = np.arange(n_reads + 1, dtype=np.int64) * N
    nwin = n_reads * be.count_windows(N, chunk, step)
    d = be.dev_alloc(batch.nbytes)
    be.h2d(d, batch)

    def run():
        lab, ln = np.zeros((nwin, chunk), dtype=np.uint8), np.full(nwin, -1, dtype=np.int32)
        be.pipe_submit_reads(d, read_off, n_reads, chunk, step, W, lab, ln)
        be.pipe_flush()
        return lab, ln
    try:
        expect = _list_slab_tiles([N] * n_reads) * _slab_launches(WSETS[0][1])
        (lab1, ln1), (lab0, ln0) = _on_off(be, run, expect)
    finally:
        be.pipe_flush()
        be.dev_free(d)
    assert (ln1 >= 0).all()
    assert np.array_equal(ln1, ln0) and np.array_equal(lab1, lab0)
