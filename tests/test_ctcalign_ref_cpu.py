"""No GPU: the forced-alignment reference of the GPU tests (tests/_ctcalign_ref.py) on cases that can be checked by hand, and its
vectorised form against the plain one."""
import math

import numpy as np
import pytest

import _ctcalign_ref as ref


def test_uniform_rows_take_the_tie_break_path():
    """every path scores 6 log 0.2; strict-greater in the order s, s-1, s-2 keeps the traceback in its state as long as it can, so the
    labels sit in the first rows"""
    r = ref.align(np.full((6, 5), 0.2), [0, 1, 2])
    assert r.status == ref.OK
    assert r.first_step == [0, 1, 2] and r.last_step == [0, 1, 2]
    assert abs(r.score - 6 * math.log(0.2)) < 1e-13
    v = 0.0
    for t in range(6):   # the score is the left-to-right sum of the rows' logs
        v = math.log(0.2) + v if t else math.log(0.2)
    assert r.score == v
    assert r.qual == [0, 0, 0]   # e = 0.8: above every threshold


def test_repeat_needs_a_blank():
    r = ref.align(np.full((2, 5), 0.2), [0, 0])
    assert r.status == ref.NO_PATH and r.score == ref.NEG
    assert r.first_step == [-1, -1] and r.last_step == [-1, -1] and r.qual == [0, 0]
    r = ref.align(np.full((3, 5), 0.2), [0, 0])
    assert r.status == ref.OK and r.first_step == [0, 2] and r.last_step == [0, 2]


def test_more_labels_than_rows_is_no_path():
    r = ref.align(np.full((3, 5), 0.2), [0, 1, 2, 3])
    assert r.status == ref.NO_PATH and r.score == ref.NEG


def test_no_labels_is_the_all_blank_path():
    P = np.array([[0.1, 0.1, 0.1, 0.1, 0.6], [0.2, 0.2, 0.2, 0.2, 0.2], [0.0, 0.0, 0.0, 0.5, 0.5]])
    r = ref.align(P, [])
    assert r.status == ref.OK and r.first_step == [] and r.qual == []
    assert r.score == math.log(0.5) + (math.log(0.2) + math.log(0.6))
    with pytest.raises(ValueError):
        ref.align(np.zeros((0, 5)), [])


def test_quality_thresholds_and_exact_one():
    # a certain base: e = 0 -> 50; a zero anywhere on the only path -> no path
    P = np.array([[0.0, 1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]])
    r = ref.align(P, [1])
    assert r.status == ref.OK and r.qual == [50] and r.score == 0.0 and r.first_step == [0]
    assert ref.align(P, [2]).status == ref.NO_PATH
    # p = 0.9 -> e = 0.1 (to an ulp or so): Q9 or Q10 by the comparison, never beyond
    P = np.array([[0.02, 0.9, 0.02, 0.02, 0.04]])
    r = ref.align(P, [1])
    assert r.qual[0] == sum(1 for k in range(1, 51) if 1.0 - 0.9 <= 10.0 ** (-k / 10)) and r.qual[0] in (9, 10)
    # the quality takes the best row of the base's stay
    P = np.array([[0.5, 0.1, 0.1, 0.1, 0.2], [0.99, 0.0, 0.0, 0.0, 0.01], [0.0, 0.0, 0.0, 0.0, 1.0]])
    r = ref.align(P, [0])
    assert (r.first_step, r.last_step) == ([0], [1]) and r.qual == [sum(1 for k in range(1, 51) if 1.0 - 0.99 <= 10.0 ** (-k / 10))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vectorised_form_is_the_plain_one(dtype):
    rng = np.random.default_rng(7)
    worst = 1.0
    for T, L in [(1, 0), (1, 1), (2, 2), (3, 2), (9, 0), (40, 17), (74, 33), (40, 40), (30, 31)]:
        lab = [int(c) for c in rng.integers(0, 4, L)]
        if T == L:
            lab = [(i * 3 + 1) % 4 for i in range(L)]   # repeat-free: every row an emission
        P = ref.peaky(T, lab, rng, dtype)
        if L == 17:
            P[5] = 0.0   # a dead row
            P[5, 4] = 1.0
        a, b = ref.align(P, lab), ref.align_fast(P, lab)
        assert (a.status, a.first_step, a.last_step, a.qual) == (b.status, b.first_step, b.last_step, b.qual)
        assert a.score == b.score and a.margin == b.margin
        worst = min(worst, a.margin)
    assert worst > 1e-9
    for P, lab in [(np.full((12, 5), 0.2, dtype=dtype), [0, 0, 1, 1, 2]), (np.repeat(ref.peaky(9, [1, 2, 2], rng, dtype), 2, axis=0), [1, 2, 2])]:
        a, b = ref.align(P, lab), ref.align_fast(P, lab)
        assert a.status == ref.OK and (a.first_step, a.last_step, a.qual, a.score) == (b.first_step, b.last_step, b.qual, b.score)


def test_workspace_formula():
    assert ref.workspace_bytes(1, 0) == 256 * 3
    assert ref.workspace_bytes(1600, 1500) == 64 * 1600 + 4 * 1600 * 188 + 16 * 1600
