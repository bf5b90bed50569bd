"""The seeded cases of the tests of eventalign on event rows (tests/test_eventalign_events_cpu.py asserts every case's defining condition
without a GPU and holds rd_eventalign_events_host to the restatement on them; tests/test_gpu_eventalign_events.py runs them on the device).
A CASE is one read of one call: {"name", "ev" (the events' records), "T", "codes" uint8, "m2", "d4", "pen", "off", "model", "cond":
callable(out) -> bool} where out is _eventalign_events_ref's dict.  The skip penalty belongs to the call, so a batch is the cases of one
(model, pen): groups().  The restatement of a case is computed once (reference()) and shared."""
import numpy as np

import _eventalign_cases as sc
import _eventalign_events_ref as ref

# the kernel's boundaries (eventalign.hip, ear_dp_kernel): 16 states per lane and per back-pointer word, 32 per pair of words, 1024 per
# wave, 4096 per band, and a third band -- in states, L + 2 of them
STATE_COUNTS = (15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
PENS = (0, 32, 96, 256)
K, MODEL, MEDIAN, D4 = sc.K, sc.MODEL, sc.MEDIAN, sc.D4
M2 = 2 * MEDIAN


def bound_model():
    """every state at level 0 with the largest weight and the largest bias: a sample far away costs the cap plus 256 in every state"""
    n = 4 ** K
    return ref.Model(K, [0] * n, [(1 << 32) - 1] * n, [256] * n, (0, (1 << 32) - 1, 256))


BOUND_MODEL = bound_model()


def _levels(codes, model):
    return [model.bg[0]] + [model.lvl[ref.kmer(codes, b, model.k)] for b in range(len(codes))] + [model.bg[0]]


def random_path(rng, L, E, start, end, extra_skips=0.02):
    """E states, one per row, from `start` (0 or 1) to `end` (L or L + 1) in steps of 0, 1 or 2, with as few steps of 2 as E allows plus a few"""
    D, n = end - start, E - 1
    assert 0 <= D <= 2 * n
    k2 = max(0, D - n)
    k2 = min(D // 2, k2 + int(rng.integers(0, int(extra_skips * D) + 2)))
    k1 = D - 2 * k2
    assert k1 + k2 <= n
    steps = np.concatenate([np.full(k2, 2), np.full(k1, 1), np.zeros(n - k1 - k2, dtype=np.int64)]).astype(np.int64)
    rng.shuffle(steps)
    return np.concatenate([[start], start + np.cumsum(steps)]).astype(np.int64)


def signal_on_path(rng, codes, path, model=MODEL, noise=3.0, n_max=24, n=None):
    """the events of a signal that sits on the level of path[e] during event e -> (ev, T)"""
    lv = np.array(_levels(codes, model), dtype=np.float64)[np.asarray(path)]
    n = rng.integers(1, n_max + 1, len(path)) if n is None else np.asarray(n, dtype=np.int64)
    x = np.repeat(lv, n) * D4 / 1024 + MEDIAN + rng.normal(0, noise, int(n.sum()))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    return ref.events_of(x, starts), int(n.sum())


def _case(name, ev, T, codes, pen, m2=M2, d4=D4, off=0, model=MODEL, cond=None):
    ev = dict(start=np.ascontiguousarray(ev["start"], dtype=np.int32), sum=np.ascontiguousarray(ev["sum"], dtype=np.int64),
              sumsq=np.ascontiguousarray(ev["sumsq"], dtype=np.int64), min=np.ascontiguousarray(ev["min"], dtype=np.int16),
              max=np.ascontiguousarray(ev["max"], dtype=np.int16))
    return dict(name=name, ev=ev, T=int(T), codes=np.ascontiguousarray(codes, dtype=np.uint8), pen=int(pen), m2=int(m2), d4=int(d4), off=int(off),
                model=model, cond=cond or (lambda o: o["status"] == ref.OK))


def no_events():
    return dict(start=np.zeros(0, np.int32), sum=np.zeros(0, np.int64), sumsq=np.zeros(0, np.int64), min=np.zeros(0, np.int16), max=np.zeros(0, np.int16))


def skipped(o):
    """the bases a restated path jumped over"""
    return {b for b, f in enumerate(o["row_first"]) if f < 0}


def entered_by_skip(o, s):
    """state s (base s - 1) is entered from s - 2: base s - 2 is skipped and base s - 1 is not"""
    return (s - 2) in skipped(o) and (s - 1) not in skipped(o)


def entered_by_advance(o, s):
    return (s - 2) not in skipped(o) and (s - 1) not in skipped(o) and o["row_first"][s - 1] == o["row_last"][s - 2] + 1


def shape_cases():
    """L + 2 on both sides of every boundary the kernel has; E = ceil((L + 1) / 2) (every transition is a skip), that plus 1, L and
    2 L + 3; the penalties in turn"""
    rng = np.random.default_rng(280)
    out, i = [], 0
    for S in STATE_COUNTS:
        L = S - 2
        codes = rng.integers(0, 4, L)
        for E in ((L + 2) // 2, (L + 2) // 2 + 1, L, 2 * L + 3):
            pen = PENS[(i + i // 4) % len(PENS)]      # every penalty meets every kind of E
            i += 1
            ways = [(a, b) for a in (0, 1) for b in (L, L + 1) if 0 <= b - a <= 2 * (E - 1)]      # the starts and ends E rows allow
            start, end = ways[int(rng.integers(0, len(ways)))]
            path = random_path(rng, L, E, start, end)
            ev, T = signal_on_path(rng, codes, path)
            all_skips = E == (L + 2) // 2 and L % 2 == 1
            out.append(_case(f"S{S}_E{E}", ev, T, codes, pen, off=int(rng.integers(0, 5000)),
                             cond=lambda o, L=L, E=E, a=all_skips: o["status"] == ref.OK and (not a or o["n_skipped"] == E - 1 == (L - 1) // 2)))
    return out


def skip_path_cases():
    """both parities of the all-skip path; a path that enters states 16, 1024 and 4096 by a skip (and 17, 1025, 4097 by an advance), one
    that enters 17, 1025 and 4097 by a skip (over 16, 1024 and 4096) and one that enters all six by an advance: both halves of the pair
    through DPP, LDS and the band column"""
    rng = np.random.default_rng(281)
    out = []
    for name, L, start in (("allskip_from0", 40, 0), ("allskip_from1", 41, 1), ("allskip_from0_long", 2100, 0), ("allskip_from1_long", 2101, 1)):
        codes = rng.integers(0, 4, L)
        E = (L + 2) // 2
        path = start + 2 * np.arange(E)
        assert path[-1] in (L, L + 1)
        ev, T = signal_on_path(rng, codes, path)
        out.append(_case(name, ev, T, codes, 96, cond=lambda o, E=E, s=start: o["status"] == ref.OK and o["n_skipped"] == E - 1
                         and (o["row_first"][0] == -1) == (s == 0)))
    L = 4300
    codes = rng.integers(0, 4, L)
    for name, by_skip, by_adv in (("enter_even_by_skip", (16, 1024, 4096), (17, 1025, 4097)), ("enter_odd_by_skip", (17, 1025, 4097), ()),
                                  ("enter_by_advance", (), (16, 17, 1024, 1025, 4096, 4097))):
        states = [s for s in range(0, L + 2) if s + 1 not in by_skip]       # the state below a skip's target has no row
        rows = np.ones(len(states), dtype=np.int64) + (rng.random(len(states)) < 0.3)
        for j, s in enumerate(states):
            if any(abs(s - t) <= 3 for t in by_skip + by_adv):
                rows[j] = 1
        path = np.repeat(states, rows)
        ev, T = signal_on_path(rng, codes, path, n=rng.integers(4, 12, len(path)))
        out.append(_case(name, ev, T, codes, 96, cond=lambda o, a=by_skip, b=by_adv: o["status"] == ref.OK
                         and all(entered_by_skip(o, s) for s in a) and all(entered_by_advance(o, s) for s in b)))
    return out


def edge_cases():
    rng = np.random.default_rng(282)
    out = []
    codes = rng.integers(0, 4, 40)
    # E = 1: one event; with skips it reaches state 1, so L <= 1
    one = ref.events_of(np.full(9, 640), [0])
    out.append(_case("E1_L0", one, 9, [], 96))
    out.append(_case("E1_L1", one, 9, [2], 96, cond=lambda o: o["status"] == ref.OK and o["row_first"] == [0] and o["row_last"] == [0]
                     and (o["start"], o["end"]) == ([0], [9])))
    out.append(_case("E1_L2", one, 9, [2, 1], 96, cond=lambda o: o["status"] == ref.NO_PATH))
    # NO_PATH one row short, and the last E that has a path: 2 E - 1 >= L with skips, E >= L without
    for pen, E_ok in ((96, 20), (-1, 39)):
        for E, want in ((E_ok, ref.OK), (E_ok - 1, ref.NO_PATH)):
            Lc = 39
            start, end = (1, Lc)
            path = random_path(rng, Lc, E_ok, start, end) if pen >= 0 else np.arange(1, Lc + 1)
            ev, T = signal_on_path(rng, codes[:Lc], path[:E])
            out.append(_case(f"rows_{'skips' if pen >= 0 else 'noskips'}_E{E}", ev, T, codes[:Lc], pen,
                             cond=lambda o, w=want: o["status"] == w and (w == ref.OK or o["sums"] == [0] * 5)))
    # skips off on an ordinary read, and the same read with the penalties' two ends
    path = random_path(rng, 40, 90, 0, 41, extra_skips=0.1)
    ev, T = signal_on_path(rng, codes, path)
    out.append(_case("pen_off", ev, T, codes, -1, cond=lambda o: o["status"] == ref.OK and o["n_skipped"] == 0))
    out.append(_case("pen_0", ev, T, codes, 0, cond=lambda o: o["status"] == ref.OK and o["n_skipped"] > 0))
    out.append(_case("pen_256", ev, T, codes, 256, cond=lambda o: o["status"] == ref.OK and o["n_skipped"] > 0))
    # ties: a constant signal on G's level (903: GGG costs 52 a sample there, the background 185) on a homopolymer with pen 0.  Every
    # reachable base cell of a row has the same value, so wherever two predecessors are reachable they tie: the path stays.  It moves
    # only where a state is first reachable, from whatever reaches it: state 3 at row 1 and state 5 at row 2 by the skip alone, state 6 at
    # row 3 by the advance and the skip, which tie -- the advance
    flat = ref.events_of(np.full(150, 903), np.arange(0, 150, 3))
    out.append(_case("tie_const", flat, 150, np.full(6, 2), 0, cond=lambda o: o["status"] == ref.OK and o["n_skipped"] == 2
                     and o["row_first"] == [0, -1, 1, -1, 2, 3] and o["row_last"] == [0, -1, 1, -1, 2, 49] and o["score"] == 150 * 52))
    # n_e = 1 throughout: the rows are the samples
    path = random_path(rng, 40, 120, 1, 41)
    ev, T = signal_on_path(rng, codes, path, n=np.ones(len(path), dtype=np.int64))
    out.append(_case("n1", ev, T, codes, 96, cond=lambda o, T=T: o["status"] == ref.OK and T == 120))
    # event means at the +-2^14 clamp: a small d4 puts the int16 extremes far outside
    path = random_path(rng, 40, 100, 0, 41)
    x_ev, T = signal_on_path(rng, codes, path)
    for f in ("sum", "min", "max"):
        x_ev[f] = x_ev[f].copy()
    n = np.diff(np.concatenate([x_ev["start"], [T]]))
    for e, v in ((10, 32767), (60, -32768)):
        x_ev["sum"][e], x_ev["sumsq"][e], x_ev["min"][e], x_ev["max"][e] = v * n[e], v * v * n[e], v, v
    out.append(_case("clamp", x_ev, T, codes, 96, d4=16, cond=lambda o: o["status"] == ref.OK and ref.quant(32767, M2, 16) == 1 << 14
                     and ref.quant(-32768, M2, 16) == -(1 << 14)))
    # w = 0 and w = 2^32 - 1: the two special entries of the model, AAA and TTT
    ends = np.array([0, 0, 0, 0, 3, 3, 3, 3, 1, 2, 0, 0, 0, 3, 3, 3])
    path = random_path(rng, len(ends), 40, 1, len(ends))
    ev, T = signal_on_path(rng, ends, path)
    out.append(_case("w_ends", ev, T, ends, 32, cond=lambda o: MODEL.w[0] == (1 << 32) - 1 and MODEL.w[63] == 0 and ref.kmer(ends, 1, K) == 0
                     and ref.kmer(ends, 5, K) == 63 and o["status"] == ref.OK))
    # a sample offset near the top of int32
    out.append(_case("off_top", ev, T, ends, 32, off=(1 << 31) - 1 - T, cond=lambda o, T=T: o["status"] == ref.OK and max(o["end"]) <= (1 << 31) - 1
                     and min(o["start"]) >= (1 << 31) - 1 - T))
    # every status beside unaffected neighbours
    out.append(_case("empty_T0", no_events(), 0, codes[:4], 96, cond=lambda o: o["status"] == ref.EMPTY and o["row_first"] == [-1] * 4))
    out.append(_case("empty_E0", no_events(), 500, codes[:4], 96, cond=lambda o: o["status"] == ref.EMPTY))
    long_ev = ref.events_of(rng.integers(400, 800, (1 << 19) + 1), np.arange(0, 1 << 19, 4096))
    out.append(_case("too_long", long_ev, (1 << 19) + 1, codes[:3], 96, cond=lambda o: o["status"] == ref.TOO_LONG))
    out.append(_case("mad_zero", ev, T, ends, 96, d4=0, cond=lambda o: o["status"] == ref.MAD_ZERO and o["score"] == 0))
    return out


def bound_cases():
    """the value bound: T = 2^19, one event of n = 2^19 - E + 1 samples far from every level, every state at the cost cap with bias 256:
    every row adds n_e * 1280 whatever the state, T * 1280 in all.  33 rows and 63 bases: 32 transitions from state 1 to state 63 need at
    least 30 skips (2 k + (32 - k) >= 62) at the largest penalty, 256 each"""
    rng = np.random.default_rng(283)
    E, L = 33, 63
    n = np.ones(E, dtype=np.int64)
    n[7] = (1 << 19) - E + 1
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    mean = rng.integers(3000, 3200, E)
    ev = dict(start=starts, sum=mean * n, sumsq=mean * mean * n, min=mean, max=mean)
    codes = rng.integers(0, 4, L)
    return [_case("bound", ev, 1 << 19, codes, 256, model=BOUND_MODEL,
                  cond=lambda o: o["status"] == ref.OK and o["n_skipped"] == 30 and o["score"] == (1 << 19) * 1280 + 30 * 256
                  and 5 * (1 << 27) < o["score"] < 3 * (1 << 28))]


_cache = {}


def all_cases():
    if "cases" not in _cache:
        _cache["cases"] = shape_cases() + skip_path_cases() + edge_cases() + bound_cases()
        assert len({c["name"] for c in _cache["cases"]}) == len(_cache["cases"])
    return _cache["cases"]


def small_cases():
    """the cases the plain-Python restatement can do in a moment"""
    return [c for c in all_cases() if len(c["ev"]["start"]) * (len(c["codes"]) + 2) <= 40000]


def groups(cases=None):
    """-> [(model, pen, the cases of that call)]"""
    out = {}
    for c in (all_cases() if cases is None else cases):
        out.setdefault((id(c["model"]), c["pen"]), []).append(c)
    return [(cs[0]["model"], cs[0]["pen"], cs) for cs in out.values()]


def reference(case):
    """the restatement's output of a case (the NumPy twin; the CPU test holds it to the plain version), computed once"""
    key = ("ref", case["name"])
    if key not in _cache:
        _cache[key] = ref.align_numpy(case["ev"], case["T"], case["codes"], case["model"], case["m2"], case["d4"], case["pen"], case["off"])
    return _cache[key]


def call_args(cases):
    """-> what Backend.eventalign_events / eventalign_events_host take, but the model and the penalty"""
    return dict(events=[c["ev"] for c in cases], n_samples=[c["T"] for c in cases], seqs=[c["codes"] for c in cases],
                m2=[c["m2"] for c in cases], d4=[c["d4"] for c in cases], sample_off=[c["off"] for c in cases])


def backend_model(m=MODEL):
    from radian_amd.backend import EvalModel
    return EvalModel(m.k, m.lvl, np.array(m.w, dtype=np.uint64).astype(np.uint32), m.bias, m.bg)


# ------------------------------------------------------------------------------------------------ the identity with sample rows
def sample_events(c):
    """every sample of an _eventalign_cases case's window as one event"""
    x = c["raw"][c["t_lo"]:c["t_hi"]].astype(np.int64)
    return dict(start=np.arange(len(x), dtype=np.int32), sum=x, sumsq=x * x, min=x.astype(np.int16), max=x.astype(np.int16))


def assert_identity(got, want, cases):
    """an EvalRowsResult of one event per sample without skips against the EvalResult of the same windows"""
    for r, c in enumerate(cases):
        ok = int(want.status[r]) == ref.OK
        assert int(got.status[r]) == int(want.status[r]) and int(got.score[r]) == int(want.score[r]) and int(got.n_skipped[r]) == 0, c["name"]
        assert got.fit_sums[r].tolist() == want.fit_sums[r].tolist(), c["name"]
        shift = c["t_lo"] if ok else 0
        assert (got.row_first[r] + shift).tolist() == want.first_step[r].tolist() and (got.row_last[r] + shift).tolist() == want.last_step[r].tolist(), c["name"]
        for f in ("start", "end", "sum", "sumsq", "min", "max"):
            assert getattr(got.events, f)[r].tolist() == getattr(want.events, f)[r].tolist(), (c["name"], f)
