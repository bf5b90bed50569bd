"""GPU checks of the forced CTC alignment (rd_ctc_align_batch / Backend.ctc_align) against the plain-Python restatement of its
contract (tests/_ctcalign_ref.py).  Everything is compared for EXACT equality: steps, qualities, status and the score's bits.

Sizes follow the kernel (radian_amd/csrc/ctcalign.hip): a thread owns 16 states, a wave 1024 (at most that many: one wave, no barrier:
L <= 511), a workgroup pass 4096 (L <= 2047); more states are swept band after band (L = 2048: the band edge falls between the two
end states; L = 2100)."""
import numpy as np
import pytest

import _ctcalign_ref as ref

pytestmark = pytest.mark.gpu

SMALL_L = [0, 1, 2, 31, 32, 33, 127, 128, 129, 511, 512]
BIG = [(2048, 2100), (2100, 2200)]   # (L, T), repeat-free labels


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same(res, i, r):
    assert int(res.status[i]) == r.status, (i, int(res.status[i]), r.status)
    assert _bits(res.score[i]) == _bits(r.score), (i, float(res.score[i]), r.score)
    assert res.first_step[i].tolist() == r.first_step, i
    assert res.last_step[i].tolist() == r.last_step, i
    assert res.qual[i].tolist() == r.qual, i


def _repeat_free(L, start=1):
    return [(start + 3 * i) % 4 for i in range(L)]   # consecutive labels differ by 3 mod 4


def _pack(mats, rng, dtype):
    """sequences in shuffled order with rows of another sequence's making between them -> (rows, seq_off, seq_len)"""
    order = rng.permutation(len(mats))
    off = np.zeros(len(mats), dtype=np.int64)
    parts, at = [], 0
    for k in order:
        gap = int(rng.integers(1, 4))
        parts.append(np.full((gap, 5), 0.2, dtype=dtype))
        at += gap
        off[k] = at
        parts.append(mats[k])
        at += mats[k].shape[0]
    return np.ascontiguousarray(np.concatenate(parts)), off, np.array([m.shape[0] for m in mats], dtype=np.int32)


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def batch(request):
    """the seeded peaky batch and its reference results, computed once per input type"""
    dtype = request.param
    rng = np.random.default_rng(20 if dtype == np.float32 else 21)
    labs, mats = [], []
    for L in SMALL_L:
        labs.append([int(c) for c in rng.integers(0, 4, L)])
        mats.append(ref.peaky(2 * L + 8, labs[-1], rng, dtype))
    for L, T in BIG:
        labs.append(_repeat_free(L))
        mats.append(ref.peaky(T, labs[-1], rng, dtype))
    exp = [ref.align(m, l) if len(l) <= 33 else ref.align_fast(m, l) for m, l in zip(mats, labs)]
    rows, off, ln = _pack(mats, rng, dtype)
    return {"labs": labs, "mats": mats, "exp": exp, "rows": rows, "off": off, "len": ln}


def test_batch_equals_reference(be, batch):
    exp = batch["exp"]
    assert all(r.status == ref.OK for r in exp)
    assert min(r.margin for r in exp) > 1e-9   # no quality of these inputs hangs on the last bit of a threshold
    res = be.ctc_align(batch["rows"], batch["off"], batch["len"], batch["labs"])
    for i, r in enumerate(exp):
        _same(res, i, r)
    # a path stays in a label's state from first_step to last_step, and the labels follow each other
    for i in range(len(exp)):
        f, l = res.first_step[i], res.last_step[i]
        assert (f <= l).all() and (l[:-1] < f[1:]).all() and (len(f) == 0 or (f[0] >= 0 and l[-1] < batch["len"][i]))


def test_one_sequence_per_call_and_several_launches_give_the_same(be, batch):
    from radian_amd.backend import ctc_align_workspace_bytes
    exp, labs, mats = batch["exp"], batch["labs"], batch["mats"]
    for i, r in enumerate(exp):
        one = be.ctc_align(mats[i], [0], [mats[i].shape[0]], [labs[i]])
        _same(one, 0, r)
    need = [ref.workspace_bytes(m.shape[0], len(l)) for m, l in zip(mats, labs)]
    assert need == [ctc_align_workspace_bytes(m.shape[0], len(l)) for m, l in zip(mats, labs)]
    budget = max(need) + 4096   # the largest alone, or a few of the others: at least three launches
    assert sum(need) > 2 * budget
    res = be.ctc_align(batch["rows"], batch["off"], batch["len"], labs, budget_bytes=budget)
    for i, r in enumerate(exp):
        _same(res, i, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_tight_cases(be, dtype):
    rng = np.random.default_rng(5)
    cases = []
    for L in (1, 7, 64, 600):                       # T = L, repeat-free: every row is an emission
        cases.append((ref.peaky(L, _repeat_free(L), rng, dtype), _repeat_free(L)))
    cases.append((ref.peaky(2048, _repeat_free(2048), rng, dtype), _repeat_free(2048)))   # ... with the last state alone in a band no row reaches
    cases.append((ref.peaky(1, [], rng, dtype), []))                                       # T = 1
    cases.append((ref.peaky(1, [2], rng, dtype), [2]))
    cases.append((ref.peaky(3, [0, 0], rng, dtype), [0, 0]))                               # a repeat with no row to spare
    cases.append((ref.peaky(4, [0, 0], rng, dtype), [0, 0]))                               # ... with exactly one
    cases.append((ref.peaky(9, [1, 1, 1, 2, 2], rng, dtype), [1, 1, 1, 2, 2]))             # three repeats: 8 rows at least, one to spare
    cases.append((ref.peaky(2, [3, 3], rng, dtype), [3, 3]))                               # no room for the blank
    cases.append((ref.peaky(5, _repeat_free(6), rng, dtype), _repeat_free(6)))             # L > T
    cases.append((ref.peaky(40, _repeat_free(700), rng, dtype), _repeat_free(700)))        # L > T, beyond one wave
    exp = [ref.align_fast(m, l) for m, l in cases]
    assert [r.status for r in exp] == [ref.OK] * 10 + [ref.NO_PATH] * 3
    assert min(r.margin for r in exp) > 1e-9
    rows, off, ln = _pack([m for m, _ in cases], rng, dtype)
    res = be.ctc_align(rows, off, ln, [l for _, l in cases])
    for i, r in enumerate(exp):
        _same(res, i, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ties_take_the_contracts_path(be, dtype):
    rng = np.random.default_rng(9)
    cases = [(np.full((6, 5), 0.2, dtype=dtype), [0, 1, 2]),
             (np.full((40, 5), 0.2, dtype=dtype), [0, 0, 1, 1, 2, 3, 3]),
             (np.full((1300, 5), 0.2, dtype=dtype), [int(c) for c in rng.integers(0, 4, 600)])]
    for L in (3, 50, 600):                          # every row twice: each label has two equally good rows
        lab = [int(c) for c in rng.integers(0, 4, L)]
        cases.append((np.ascontiguousarray(np.repeat(ref.peaky(2 * L + 8, lab, rng, dtype), 2, axis=0)), lab))
    exp = [ref.align(m, l) if len(l) <= 7 else ref.align_fast(m, l) for m, l in cases]
    assert exp[0].first_step == [0, 1, 2] and all(r.status == ref.OK for r in exp)
    assert min(r.margin for r in exp) > 1e-9
    rows, off, ln = _pack([m for m, _ in cases], rng, dtype)
    res = be.ctc_align(rows, off, ln, [l for _, l in cases])
    for i, r in enumerate(exp):
        _same(res, i, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_exact_zeros_and_ones_and_no_path_beside_good_neighbours(be, dtype):
    rng = np.random.default_rng(13)
    lab = [int(c) for c in rng.integers(0, 4, 40)]
    good = ref.peaky(88, lab, rng, dtype)
    hard = good.copy()                               # one-hot rows along the best path: log 1 = 0, e = 0 -> Q50; zeros elsewhere
    r0 = ref.align(good, lab)
    for i in (0, 5, 39):
        t = r0.first_step[i]
        hard[t] = 0.0
        hard[t, lab[i]] = 1.0
    dead = good.copy()                               # a row of zeros: every path dies there
    dead[44] = 0.0
    blocked = ref.peaky(3, [1, 1], rng, dtype)       # the only path is A - A; its blank has probability 0
    blocked[1, 4] = 0.0
    cases = [(good, lab), (hard, lab), (dead, lab), (blocked, [1, 1]), (good, lab)]
    exp = [ref.align(m, l) for m, l in cases]
    assert [r.status for r in exp] == [ref.OK, ref.OK, ref.NO_PATH, ref.NO_PATH, ref.OK]
    assert [exp[1].qual[i] for i in (0, 5, 39)] == [50, 50, 50]
    assert min(r.margin for r in exp) > 1e-9
    rows, off, ln = _pack([m for m, _ in cases], rng, dtype)
    res = be.ctc_align(rows, off, ln, [l for _, l in cases])
    for i, r in enumerate(exp):
        _same(res, i, r)
    assert res.first_step[2].tolist() == [-1] * 40 and res.last_step[2].tolist() == [-1] * 40 and res.qual[2].tolist() == [0] * 40


def test_a_sequence_over_the_budget_alone(be):
    from radian_amd import RadianHipError
    from radian_amd.backend import CTCALIGN_TOO_LARGE
    rng = np.random.default_rng(17)
    shapes = [(30, 68), (300, 608), (31, 70)]        # (L, T)
    labs = [[int(c) for c in rng.integers(0, 4, L)] for L, _ in shapes]
    mats = [ref.peaky(T, l, rng, np.float32) for (_, T), l in zip(shapes, labs)]
    exp = [ref.align_fast(m, l) for m, l in zip(mats, labs)]
    need = [ref.workspace_bytes(T, L) for L, T in shapes]
    budget = need[1] - 1                             # from the documented formula: one byte short for the middle sequence
    assert budget > need[0] + need[2]
    rows, off, ln = _pack(mats, rng, np.float32)
    with pytest.raises(RadianHipError, match="RD_CTCALIGN_TOO_LARGE"):
        be.ctc_align(rows, off, ln, labs, budget_bytes=budget)
    res = be.ctc_align(rows, off, ln, labs, budget_bytes=budget, allow_too_large=True)
    assert int(res.status[1]) == CTCALIGN_TOO_LARGE
    assert res.first_step[1].tolist() == [-1] * 300 and res.qual[1].tolist() == [0] * 300
    _same(res, 0, exp[0])
    _same(res, 2, exp[2])
    res = be.ctc_align(rows, off, ln, labs, budget_bytes=need[1])   # exactly enough
    for i, r in enumerate(exp):
        _same(res, i, r)


def test_argument_errors(be):
    from radian_amd import RadianHipError
    P = np.full((4, 5), 0.2, dtype=np.float32)
    with pytest.raises(RadianHipError, match="at least one"):
        be.ctc_align(P, [0], [0], [[]])              # T = 0
    with pytest.raises(RadianHipError, match="0..3"):
        be.ctc_align(P, [0], [4], [[0, 4]])          # a blank among the labels
    assert be.ctc_align(P, [], [], []).score.shape == (0,)
