"""GPU check of the workspace the budgeted entry points share (rd_ctx::ws_align, sized by DevBuf::reserve_exact to the largest launch under
the caller's budget): one Backend runs align under a tiny budget, ctc_align under a larger one, map_batch, then align again, so that the
block is allocated, regrown twice by other entry points and reused while larger than needed.  Every result equals the same call on a
fresh Backend.  The same for the blocks the stages own (ws_polya, ws_segment, ws_site, ws_sim, ws_eval, ..., each described once by its
stage's layout function and carved by csrc/carve.h): small inputs, inputs some twenty times larger, the small ones again.  (What the
entry points compute is checked in their own files; the cutter's properties in tests/asan_budget.cpp, the carver's in tests/asan_carve.cpp.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same_align(a, b):
    return np.array_equal(a.score, b.score) and np.array_equal(a.counts, b.counts) and np.array_equal(a.status, b.status) and a.ops == b.ops


def _same_ctc(a, b):
    return (np.array_equal(a.score, b.score) and np.array_equal(a.status, b.status)
            and all(np.array_equal(x, y) for f in ("first_step", "last_step", "qual") for x, y in zip(getattr(a, f), getattr(b, f))))


def test_shared_workspace_grows_and_is_reused_across_entry_points():
    from radian_amd import Backend
    from radian_amd.backend import ALIGN_OK, CTCALIGN_OK, MAP_OK, align_workspace_bytes, ctc_align_workspace_bytes
    rng = np.random.default_rng(31)
    codes = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    text = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[codes(n)])
    # align: five pairs of a few dozen characters; the budget holds the largest pair alone, so the pairs take several launches
    refs = [text(n) for n in (30, 45, 17, 60, 38)]
    reads = [refs[0], text(41), text(20), text(55), refs[4][3:30]]
    align_budget = max(align_workspace_bytes(len(a), len(b)) for a, b in zip(refs, reads))
    align = lambda be: be.align(refs, reads, budget_bytes=align_budget, with_ops=True)
    # ctc_align: three sequences of a few dozen rows in one launch, which is larger than any launch of the align call
    T, labs = [40, 25, 33], [list(codes(12)), list(codes(7)), list(codes(10))]
    rows = rng.dirichlet([0.5] * 5, size=sum(T)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(T)[:-1]])
    ctc_budget = sum(ctc_align_workspace_bytes(t, len(l)) for t, l in zip(T, labs))
    assert ctc_budget > align_budget
    ctc = lambda be: be.ctc_align(rows, off, T, labs, budget_bytes=ctc_budget)
    # map_batch: two transcripts, three reads cut from them; a launch's workspace is above 1 MiB whatever its anchors
    transcripts = [codes(400), codes(500)]
    map_reads = [transcripts[0][50:170].copy(), transcripts[1][300:420].copy(), codes(90)]
    t_off = np.array([0, 400, 900], dtype=np.int64)

    def mapped(be):
        be.map_index(np.concatenate(transcripts), t_off)
        return be.map_batch(map_reads)

    def fresh(call):
        be = Backend(0)
        try:
            return call(be)
        finally:
            be.close()

    exp_align, exp_ctc, exp_map = fresh(align), fresh(ctc), fresh(mapped)
    assert (exp_align.status == ALIGN_OK).all() and (exp_ctc.status == CTCALIGN_OK).all() and list(exp_map.status[:2]) == [MAP_OK, MAP_OK]
    assert list(exp_map.t[:2]) == [0, 1]
    be = Backend(0)
    try:
        assert _same_align(align(be), exp_align), "align on a new context"
        assert _same_ctc(ctc(be), exp_ctc), "ctc_align after align's smaller workspace"
        got = mapped(be)
        assert np.array_equal(got.status, exp_map.status) and np.array_equal(got.hits, exp_map.hits), "map_batch after ctc_align's smaller workspace"
        assert _same_align(align(be), exp_align), "align inside map_batch's larger workspace"
        assert _same_ctc(ctc(be), exp_ctc), "ctc_align inside map_batch's larger workspace"
    finally:
        be.close()


def _same(a, b):
    """field by field: arrays, lists and dicts of them, and the result classes' slots"""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if hasattr(a, "__slots__"):
        return type(a) is type(b) and all(_same(getattr(a, f), getattr(b, f)) for f in a.__slots__)
    return a == b


def test_stage_owned_blocks_regrow_and_are_carved_inside_larger_ones():
    """polya_segment, segment, site_compare, site_split, sim_signal and eventalign on one Backend: on a small input (reads of 300 samples,
    one of them empty; a dozen sites of 5 to 40 events; sequences of 20 to 60 bases), on one some twenty times larger (6000 samples: several
    tiles, windows' blocks and chunks, so every block of every stage regrows and its arrays move), then on the small one again, whose
    carve then runs inside a block larger than it needs.  Every result equals, field by field, the same call on a fresh Backend."""
    import _eventalign_cases as ea
    from radian_amd import Backend
    from radian_amd.backend import PolyaParams, SegmentParams, SimModel
    from radian_amd.simulate import dwell_cdf, standin_tables
    rng = np.random.default_rng(47)
    sim_model = SimModel(5, *standin_tables(5, 7), dwell_cdf(0.2))
    eval_model = ea.backend_model()

    def inputs(T, scale):
        """three reads of T samples and an empty one; 12 sites of 5 .. 40 events times scale; four sequences of 20 .. 60 bases times scale"""
        g = {}
        quiet = lambda n: rng.integers(-3, 4, n)
        g["raws"] = [np.concatenate([rng.integers(-400, 400, T - T // 3), 100 + quiet(T // 3)]).astype(np.int16), np.zeros(0, np.int16),
                     rng.integers(-900, 900, T).astype(np.int16), np.concatenate([quiet(T // 2) - 200, rng.integers(-400, 400, T - T // 2)]).astype(np.int16)]
        per_site = rng.integers(5, 41, 12) * scale
        g["site"] = np.repeat(rng.choice(40, 12, replace=False).astype(np.uint32), per_site)
        g["cond"] = rng.integers(0, 2, g["site"].size).astype(np.uint8)
        g["value"] = (rng.normal(0, 300, g["site"].size) + 250 * g["cond"]).astype(np.int16)
        g["seqs"] = [rng.integers(0, 4, int(n) * scale).astype(np.uint8) for n in rng.integers(20, 61, 4)]
        g["keys"] = rng.integers(0, 2 ** 32, (4, 2), dtype=np.uint64).astype(np.uint32)
        L = [int(n) for n in rng.integers(20, 61, 3) * (scale if scale == 1 else scale // 4)]   # (the bases of a read stay under its samples)
        g["ea_seqs"] = [rng.integers(0, 4, L[0]).astype(np.uint8), rng.integers(0, 4, L[1]).astype(np.uint8), rng.integers(0, 4, L[2]).astype(np.uint8)]
        g["ea_raws"] = [ea.signal(rng, g["ea_seqs"][0], T, T // 10, T // 10), np.zeros(0, np.int16), ea.signal(rng, g["ea_seqs"][2], T, 5, 5)]
        return g

    def calls(be, g):
        return [be.polya_segment(g["raws"], PolyaParams(min_samples=64)),
                be.segment(g["raws"], SegmentParams(), [(0, len(x)) for x in g["raws"]]),
                be.site_compare(g["site"], g["cond"], g["value"], 40),
                be.site_split(g["site"], g["cond"], g["value"], 40, min_frac_q16=3277),
                be.sim_signal(g["seqs"], sim_model, 30, 2048, 307, 600, 91091, g["keys"]),
                be.eventalign(g["ea_raws"], g["ea_seqs"], eval_model)]

    names = ("polya_segment", "segment", "site_compare", "site_split", "sim_signal", "eventalign")
    small, large = inputs(300, 1), inputs(6000, 20)
    expected = {}
    for tag, g in (("small", small), ("large", large)):
        be = Backend(0)
        try:
            expected[tag] = calls(be, g)
        finally:
            be.close()
    # the inputs do what they are for: every stage has something to find, and the empty read is reported as such
    for tag in ("small", "large"):
        pa, sg, sc, ss, sim, ev = expected[tag]
        assert pa.status[0] == 0 and pa.status[1] != 0 and sg.n_events[0] > 1 and sg.n_events[1] == 0 and sg.status[1] != 0, tag
        assert len(sc.out_site) == 12 and len(ss.out_site) == 12 and (sc.status == 0).all(), tag
        assert all(len(r) > 0 for r in sim.raw) and (sim.status == 0).all(), tag
        assert ev.status[0] == 0 and ev.status[1] != 0 and ev.status[2] == 0, tag
    be = Backend(0)
    try:
        for tag, g in (("small", small), ("large", large), ("small", small)):
            for name, got, exp in zip(names, calls(be, g), expected[tag]):
                assert _same(got, exp), f"{name} on the {tag} input differs from a fresh context's"
    finally:
        be.close()
