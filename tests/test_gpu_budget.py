"""GPU check of the workspace the budgeted entry points share (rd_ctx::ws_align, sized by DevBuf::reserve_exact to the largest launch under
the caller's budget): one Backend runs align under a tiny budget, ctc_align under a larger one, map_batch, then align again, so that the
block is allocated, regrown twice by other entry points and reused while larger than needed.  Every result equals the same call on a
fresh Backend.  (What the entry points compute is checked in their own files; the cutter's properties in tests/asan_budget.cpp.)"""
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
