"""No-GPU checks of the CPU restatement of the model-evaluation contract (tests/_ctc_ref.py) that the GPU tests hold rd_ctc_* to:
brute force over every path for short windows, torch's CTC loss in fp64 for long ones, and hand cases of the greedy decode and
the edit distance."""
import itertools
import math

import numpy as np
import pytest

import _ctc_ref as ref


def _collapse(path):
    out, prev = [], None
    for c in path:
        if c != ref.BLANK and c != prev:
            out.append(c)
        prev = c
    return out


def _brute(y, n, label):
    p = np.exp(ref.log_probs(y[:n]))
    tot = 0.0
    for path in itertools.product(range(5), repeat=n):
        if _collapse(path) == list(label):
            tot += math.prod(p[t, c] for t, c in enumerate(path))
    return -math.log(tot) if tot > 0 else math.inf


def _labels_up_to(k):
    for L in range(k + 1):
        yield from itertools.product(range(4), repeat=L)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_loss_equals_brute_force_over_every_path(T):
    rng = np.random.default_rng(T)
    labels = list(_labels_up_to(3)) if T <= 5 else [l for l in _labels_up_to(3) if len(l) <= 1 or rng.random() < 0.25]
    for label in labels:
        y = rng.dirichlet([0.7] * 5, size=T).astype(np.float32)
        n = int(rng.integers(1, T + 1))
        got = ref.ctc_loss(y, n, label)
        exp = _brute(y, n, label)
        assert bool(ref.infeasible(label, n)) == math.isinf(exp), (label, n)
        if math.isinf(exp):
            assert math.isinf(got) and got > 0
        else:
            assert got == pytest.approx(exp, rel=1e-12, abs=0), (label, n)


def test_loss_equals_torch_ctc_loss_in_fp64():
    import torch
    rng = np.random.default_rng(7)
    shapes = [(1024, 255), (1024, 63), (1024, 25), (600, 0), (1, 0), (1, 1), (513, 200), (1024, 1), (64, 31)]
    shapes += [(int(rng.integers(1, 1025)), int(rng.integers(0, 256))) for _ in range(12)]
    for T, L in shapes:
        y = rng.dirichlet([0.5] * 5, size=1024).astype(np.float32)
        label = rng.integers(0, 4, size=L)
        if rng.random() < 0.3 and L > 4:
            label[1:4] = label[0]    # repeats
        got = ref.ctc_loss(y, T, label)
        lp = torch.from_numpy(ref.log_probs(y)[:T]).unsqueeze(1)                    # [T, 1, 5]
        tgt = torch.from_numpy(label.astype(np.int64)).unsqueeze(0) if L else torch.zeros((1, 1), dtype=torch.int64)
        exp = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([L]), blank=4, reduction="none",
                                           zero_infinity=False).item()
        if ref.infeasible(label, T):
            assert math.isinf(got) and math.isinf(exp), (T, L)
        else:
            assert got == pytest.approx(exp, rel=1e-10, abs=0), (T, L)


def test_infeasible_rule():
    assert not ref.infeasible([0, 1, 2], 3)
    assert ref.infeasible([0, 0], 2)            # a blank must separate the repeat
    assert not ref.infeasible([0, 0], 3)
    assert ref.infeasible([1, 1, 1], 4) and not ref.infeasible([1, 1, 1], 5)
    assert not ref.infeasible([], 1)


def _rows(classes, peak=0.9):
    y = np.full((len(classes), 5), (1 - peak) / 4, dtype=np.float32)
    for t, c in enumerate(classes):
        y[t, c] = peak
    return y


def test_greedy_hand_cases():
    assert ref.greedy(_rows([4, 0, 0, 4, 0, 1, 1, 2, 4]), 9) == [0, 0, 1, 2]
    assert ref.greedy(_rows([4, 0, 0, 4, 0, 1, 1, 2, 4]), 3) == [0]
    assert ref.greedy(_rows([4, 4, 4]), 3) == []
    assert ref.greedy(_rows([3, 3, 3]), 3) == [3]
    tie = np.array([[0.2, 0.2, 0.2, 0.2, 0.2], [0.1, 0.4, 0.4, 0.05, 0.05], [0.0, 0.0, 0.0, 0.5, 0.5]], dtype=np.float32)
    assert ref.greedy(tie, 3) == [0, 1, 3]      # exact ties: the lowest class wins


def test_edit_distance_hand_cases():
    assert ref.levenshtein([], []) == 0
    assert ref.levenshtein([0, 1, 2], []) == 3
    assert ref.levenshtein([], [3, 3]) == 2
    assert ref.levenshtein([0, 1, 2, 3], [0, 1, 2, 3]) == 0
    assert ref.levenshtein([0, 1, 2, 3], [0, 2, 3]) == 1
    assert ref.levenshtein([0, 1, 2, 3], [1, 2, 3, 0]) == 2
    assert ref.levenshtein([0, 0, 0], [1, 1, 1]) == 3
    assert ref.levenshtein([2, 0, 1, 3, 3], [2, 1, 0, 3]) == 2    # delete 0, substitute the first 3
    assert ref.evaluate(_rows([4, 0, 4, 1, 1, 4]), 6, [0, 1])[1:] == (0, 2, 0)
