"""Plain-Python restatement of the event contract (include/radian_hip.h, rd_event_stats): what
tests/test_resquiggle_cpu.py, tests/test_gpu_events.py and tests/test_gpu_resquiggle.py compare the library with, for equality.  Loops over
Python ints; no numpy in the arithmetic.

    event k of L   samples [start_k, end_k): start_k = first_step[k]; end_k = first_step[k+1] for k < L-1, last_step[L-1] + 1 for k = L-1
    per event      n = end - start, sum, sum of squares, min, max of the raw samples
    no path        status != OK (or L = 0): start = end = -1, everything else 0, for each label"""
OK = 0


def bounds(first_step, last_step, k):
    L = len(first_step)
    start = int(first_step[k])
    end = int(first_step[k + 1]) if k < L - 1 else int(last_step[L - 1]) + 1
    return start, end


def events(raw, first_step, last_step, status=OK):
    """one read: raw -- its samples; -> {"start", "end", "n", "sum", "sumsq", "min", "max"}: lists of Python ints, one entry per label"""
    L = len(first_step)
    assert len(last_step) == L
    out = {k: [] for k in ("start", "end", "n", "sum", "sumsq", "min", "max")}
    for k in range(L):
        if status != OK:
            vals = (-1, -1, 0, 0, 0, 0, 0)
        else:
            start, end = bounds(first_step, last_step, k)
            assert 0 <= start < end <= len(raw), "an empty event or one outside the read"
            s = sq = 0
            mn, mx = None, None
            for i in range(start, end):
                v = int(raw[i])
                s += v
                sq += v * v
                mn = v if mn is None or v < mn else mn
                mx = v if mx is None or v > mx else mx
            vals = (start, end, end - start, s, sq, mn, mx)
        for name, v in zip(("start", "end", "n", "sum", "sumsq", "min", "max"), vals):
            out[name].append(v)
    return out


def partitions(ev, first_step, last_step):
    """the events of an OK read with L >= 1 are non-empty, back to back, and cover exactly [first_step[0], last_step[L-1] + 1)"""
    L = len(first_step)
    if L == 0:
        return True
    return (all(n >= 1 for n in ev["n"]) and all(ev["end"][k] == ev["start"][k + 1] for k in range(L - 1))
            and ev["start"][0] == int(first_step[0]) and ev["end"][-1] == int(last_step[-1]) + 1
            and sum(ev["n"]) == int(last_step[-1]) + 1 - int(first_step[0]))


def steps_from_lengths(lead, lengths, rng=None):
    """first / last steps of events of the given lengths after `lead` samples of no event; a label's own rows are a random prefix of its event
    (the rest are the blank rows it owns), its whole event without rng"""
    first, last, t = [], [], lead
    for n in lengths:
        first.append(t)
        own = n if rng is None else int(rng.integers(1, n + 1))
        last.append(t + own - 1)
        t += n
    return first, last


def mutate(labels, rate, rng):
    """labels with about `rate` substitutions / insertions / deletions (a third each), as a list of ints"""
    out = []
    for c in labels:
        u = rng.random()
        if u < rate / 3:
            continue                                        # deletion
        if u < 2 * rate / 3:
            out.append(int((int(c) + 1 + rng.integers(0, 3)) % 4))   # substitution
        else:
            out.append(int(c))
        if rng.random() < rate / 3:
            out.append(int(rng.integers(0, 4)))             # insertion
    return out
