"""GPU checks of the event kernel (rd_event_stats / Backend.event_stats, radian_amd/csrc/events.hip) against the plain-Python restatement
of its contract (tests/_events_ref.py) and against rd_event_stats_host.  Everything is compared for EXACT equality.

Sizes follow the kernel: a wave owns 64 consecutive events and sweeps their samples 64 at a time -- event lengths 1, 63, 64, 65 and 4097
in every order, reads of 1, 64, 65 and 70 labels, an event of 70 000 samples of the int16 extremes, a read of 7000 labels (110 waves) and
a read that is one event of 40 960 samples (640 chunks of one wave)."""
import numpy as np
import pytest

import _events_ref as ref
from _events_cases import NO_PATH, OK, aln_of, raw_call, refusal_cases, same_events, seeded_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    return seeded_cases()


@pytest.fixture(scope="module")
def long_reads():
    """a 40 960-sample read with 7000 labels, one whose single event spans all 40 960 samples, and reads of 1, 64 and 65 short events"""
    rng = np.random.default_rng(23)
    T = 40960
    raws, firsts, lasts = [], [], []
    lengths = 1 + rng.multinomial(T - 7000 - 11, np.full(7000, 1 / 7000))
    first, last = ref.steps_from_lengths(4, [int(n) for n in lengths], rng)
    raws.append(rng.integers(-32768, 32768, T).astype(np.int16))
    firsts.append(first), lasts.append(last)
    raws.append(rng.integers(-32768, 32768, T).astype(np.int16))
    firsts.append([0]), lasts.append([T - 1])
    for L in (1, 64, 65):
        lengths = [int(n) for n in rng.integers(1, 7, L)]
        first, last = ref.steps_from_lengths(int(rng.integers(0, 3)), lengths, rng)
        raws.append(rng.integers(-4000, 4000, last[-1] + 1 + int(rng.integers(0, 3))).astype(np.int16))
        firsts.append(first), lasts.append(last)
    exp = [ref.events(x, f, l) for x, f, l in zip(raws, firsts, lasts)]
    return raws, firsts, lasts, [OK] * len(raws), exp


def test_event_stats_equals_the_restatement_on_the_cpu_cases(be, cases):
    raws, firsts, lasts, status, exp = cases
    got = be.event_stats(raws, aln_of(firsts, lasts, status))
    for r in range(len(raws)):
        same_events(got, r, exp[r])
    assert status[5] == NO_PATH and got.start[5].tolist() == [-1] * 37 and got.sum[5].tolist() == [0] * 37


def test_event_stats_on_long_reads(be, long_reads):
    raws, firsts, lasts, status, exp = long_reads
    assert len(firsts[0]) == 7000 and len(raws[0]) == 40960 and exp[1]["n"] == [40960]
    got = be.event_stats(raws, aln_of(firsts, lasts, status))
    for r in range(len(raws)):
        same_events(got, r, exp[r])
        assert ref.partitions(exp[r], firsts[r], lasts[r])


def test_event_stats_does_not_depend_on_the_grouping_and_equals_the_host(be, cases, long_reads):
    from radian_amd.backend import event_stats_host
    raws = cases[0] + long_reads[0]
    firsts, lasts, status = cases[1] + long_reads[1], cases[2] + long_reads[2], cases[3] + long_reads[3]
    whole = be.event_stats(raws, aln_of(firsts, lasts, status))
    host = event_stats_host(raws, aln_of(firsts, lasts, status))
    rev = be.event_stats(raws[::-1], aln_of(firsts[::-1], lasts[::-1], status[::-1]))
    n = len(raws)
    for name in ("start", "end", "n", "sum", "sumsq", "min", "max"):
        for r in range(n):
            a = getattr(whole, name)[r]
            assert a.dtype == getattr(host, name)[r].dtype and np.array_equal(a, getattr(host, name)[r]), (name, r)
            assert np.array_equal(a, getattr(rev, name)[n - 1 - r]), (name, r)
    for r in range(n):
        one = be.event_stats([raws[r]], aln_of([firsts[r]], [lasts[r]], [status[r]]))
        for name in ("start", "end", "sum", "sumsq", "min", "max"):
            assert np.array_equal(getattr(one, name)[0], getattr(whole, name)[r]), (name, r)


def test_event_stats_refuses_bad_arguments_before_anything_is_launched(be):
    good, bad = refusal_cases()
    fn = lambda *a: be._L.rd_event_stats(be._h, *a)
    assert raw_call(fn, **good) == 0
    for name, kw in bad:
        outs = [np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(4, 77, np.int64), np.full(4, 77, np.int64), np.full(4, 77, np.int16),
                np.full(4, 77, np.int16)]
        assert raw_call(fn, outs=outs, **kw) == -1, name   # RD_ERR_ARG
        assert all((o == 77).all() for o in outs), name
    assert raw_call(lambda *a: be._L.rd_event_stats(None, *a), **good) == -1   # a null context
