"""Seeded inputs shared by tests/test_resquiggle_cpu.py, tests/test_gpu_events.py and tests/test_gpu_resquiggle.py: reads with steps (and the
restatement's events for them, computed once), the argument refusals, and forced alignments of mutated labels."""
import numpy as np

import _ctcalign_ref as caref
import _events_ref as ref

OK, NO_PATH = 0, 1
LENGTHS = [1, 63, 64, 65, 4097]   # event lengths around the kernel's 64-sample chunk


def aln_of(first, last, status):
    from radian_amd.backend import CtcAlignResult
    n = len(first)
    return CtcAlignResult([np.asarray(f, dtype=np.int32) for f in first], [np.asarray(l, dtype=np.int32) for l in last],
                          [np.zeros(len(f), dtype=np.uint8) for f in first], np.zeros(n), np.asarray(status, dtype=np.int32))


def same_events(got, r, exp):
    """read r of an EventsResult equals the restatement's dict"""
    for name in ("start", "end", "n", "sum", "sumsq", "min", "max"):
        assert [int(v) for v in getattr(got, name)[r]] == exp[name], (r, name)


def seeded_cases():
    """reads, steps and status of the seeded cases (shared with tests/test_gpu_events.py): the chunk-edge lengths in every order, the int16
    extremes in an event of 70 000 samples, a read without a path between two good ones, and a read without labels"""
    rng = np.random.default_rng(17)
    raws, firsts, lasts, status = [], [], [], []

    def add(raw, first, last, st=OK):
        raws.append(np.ascontiguousarray(raw, dtype=np.int16))
        firsts.append(first)
        lasts.append(last)
        status.append(st)

    for lead, tail, with_rng in ((0, 0, False), (5, 9, True), (130, 1, True)):
        lengths = [int(x) for x in rng.permutation(LENGTHS * 2)]
        first, last = ref.steps_from_lengths(lead, lengths, rng if with_rng else None)
        add(rng.integers(-32768, 32768, lead + sum(lengths) + tail), first, last)
    # the int16 extremes in events of 70 000 samples: all -32768, all 32767 (the sums leave int32 on either side, the sums of squares pass
    # 2^32), and half of each
    big = np.concatenate([rng.integers(-500, 500, 7), np.full(70000, -32768), np.full(70000, 32767), np.full(35000, -32768), np.full(35000, 32767),
                          rng.integers(-500, 500, 40)])
    first, last = ref.steps_from_lengths(3, [4, 70000, 70000, 70000, 30], rng)
    add(big, first, last)
    # a read without a path between two good ones (its steps are the aligner's -1s), and a read with no labels
    add(rng.integers(-3000, 3000, 500), *ref.steps_from_lengths(2, [int(x) for x in rng.integers(1, 9, 70)], rng))
    add(rng.integers(-3000, 3000, 300), [-1] * 37, [-1] * 37, NO_PATH)
    add(rng.integers(-3000, 3000, 400), *ref.steps_from_lengths(0, [int(x) for x in rng.integers(1, 6, 66)], rng))
    add(rng.integers(-3000, 3000, 50), [], [])
    exp = [ref.events(x, f, l, s) for x, f, l, s in zip(raws, firsts, lasts, status)]
    return raws, firsts, lasts, status, exp


def raw_call(fn, raw, read_off, first, last, label_off, label_len, status, outs=None, null=()):
    """the C entry point with explicit arrays (null: names passed as null pointers) -> return code"""
    import ctypes
    a = {"raw": np.asarray(raw, dtype=np.int16), "read_off": np.asarray(read_off, dtype=np.int64), "first": np.asarray(first, dtype=np.int32),
         "last": np.asarray(last, dtype=np.int32), "label_off": np.asarray(label_off, dtype=np.int64),
         "label_len": np.asarray(label_len, dtype=np.int32), "status": np.asarray(status, dtype=np.int32)}
    n = max(1, len(first))
    o = outs or [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int16), np.zeros(n, np.int16)]
    p = lambda name: None if name in null else a[name].ctypes.data_as(ctypes.c_void_p)
    po = [None if f"out{i}" in null else x.ctypes.data_as(ctypes.c_void_p) for i, x in enumerate(o)]
    return fn(p("raw"), p("read_off"), len(label_len), p("first"), p("last"), p("label_off"), p("label_len"), p("status"), *po)


def refusal_cases():
    """(name, keyword arguments of raw_call) of every argument refusal of rd_event_stats / rd_event_stats_host: one read of 10 samples and
    3 labels unless said otherwise"""
    good = dict(raw=np.arange(10), read_off=[0, 10], first=[1, 3, 6], last=[2, 4, 8], label_off=[0], label_len=[3], status=[OK])
    out = [("first-negative", {**good, "first": [-1, 3, 6]}), ("first-after-last", {**good, "first": [1, 5, 6]}),
           ("last-at-T", {**good, "last": [2, 4, 10]}), ("last-reaches-next-first", {**good, "last": [3, 4, 8]}),
           ("last-beyond-next-first", {**good, "last": [2, 7, 8]}), ("negative-label-len", {**good, "label_len": [-1]}),
           ("read-offsets-decrease", dict(raw=np.arange(10), read_off=[0, 10, 4], first=[1, 3, 6], last=[2, 4, 8], label_off=[0, 3], label_len=[3, 0],
                                          status=[OK, OK])),
           ("label-offsets-overlap", dict(raw=np.arange(20), read_off=[0, 10, 20], first=[1, 3, 6, 1], last=[2, 4, 8, 1], label_off=[0, 2],
                                          label_len=[3, 1], status=[OK, OK])),
           ("label-offsets-decrease", dict(raw=np.arange(20), read_off=[0, 10, 20], first=[1, 1, 3, 6], last=[1, 2, 4, 8], label_off=[1, 0],
                                           label_len=[3, 1], status=[OK, OK]))]
    for name in ("raw", "read_off", "first", "last", "label_off", "label_len", "status", "out0", "out1", "out2", "out3", "out4", "out5"):
        out.append(("null-" + name, {**good, "null": (name,)}))
    return good, out


def mutated_alignment_cases(n_cases=20, seed=7):
    """peaky matrices of T = 200 .. 3000 rows and, as the labels to align, the generating labels with 12 % substitutions / insertions /
    deletions: the inputs wherever a test needs "a reference that is not the call" (none of them may come back without a path)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        T = int(rng.integers(200, 3001))
        lab = [int(c) for c in rng.integers(0, 4, T // 5)]
        out.append((caref.peaky(T, lab, rng, np.float32), ref.mutate(lab, 0.12, rng), rng.integers(-2000, 2000, T)))
    return out


