"""The seeded cases of the banded eventalign tests (tests/test_eventalign_banded_cpu.py asserts every case's defining condition without a
GPU and holds rd_eventalign_banded_host to the restatement on them; tests/test_gpu_eventalign_banded.py runs them on the device).  A CASE
is one read of one call: {"name", "raw" int16, "codes" uint8, "guide" int32, "t_lo", "t_hi", "m2", "d4", "model", "kind", "cond":
callable(out, full) -> bool} where out is _eventalign_banded_ref's dict and full _eventalign_ref's on the same scale.  The model belongs
to the call, so a batch is the cases of one model: groups().  The restatements of a case are computed once and shared."""
import numpy as np

import _eventalign_banded_ref as ref
import _eventalign_cases as sc
import _eventalign_events_cases as evc
import _eventalign_events_ref as eref
import _eventalign_ref as fref

# the kernel's boundaries (eventalign.hip, eab_dp_kernel): a state index against the 64 lanes and the window's width, and against the wave and
# band sizes of the full DP's kernel -- in states, L + 2 of them
STATE_COUNTS = (63, 64, 65, 66, 127, 128, 129, 1025, 4097)
W = ref.W
MODEL, BOUND_MODEL, MEDIAN, D4 = sc.MODEL, evc.BOUND_MODEL, sc.MEDIAN, sc.D4
SCALE = dict(m2=2 * MEDIAN, d4=D4)

_cache = {}


def full_of(raw, codes, model, t_lo, t_hi, m2, d4):
    return fref.align_numpy(raw, codes, model, t_lo, t_hi, m2, d4)


def _case(name, kind, raw, codes, guide, t_lo=0, t_hi=None, m2=0, d4=0, model=MODEL, cond=None):
    raw = np.ascontiguousarray(raw, dtype=np.int16)
    guide = np.ascontiguousarray(guide, dtype=np.int32)
    assert len(guide) == len(codes) and (np.diff(guide.astype(np.int64)) >= 0).all(), name
    return dict(name=name, kind=kind, raw=raw, codes=np.ascontiguousarray(codes, dtype=np.uint8), guide=guide, t_lo=int(t_lo),
                t_hi=len(raw) if t_hi is None else int(t_hi), m2=int(m2), d4=int(d4), model=model, cond=cond or (lambda o, f: True))


def same(o, f):
    """every field the two contracts share"""
    return all(o[k] == f[k] for k in f)


def is_interior(c, f):
    """does the full DP's path meet the identity's condition under this case's guide?"""
    T, L = c["t_hi"] - c["t_lo"], len(c["codes"])
    return f["status"] == fref.OK and ref.interior(f["first"], f["last"], L, c["guide"], c["t_lo"], T)


def shift(guide, k, t_lo, t_hi):
    """the guide whose count g(t) is the given one plus k (k > 0: the window runs ahead of the path by k states; k < 0: it lags)"""
    L = len(guide)
    k = max(-L, min(L, k))
    if k >= 0:
        return np.concatenate([np.full(k, t_lo), guide[:L - k]])
    return np.concatenate([guide[-k:], np.full(-k, t_hi + 1)])


def lo_rows(c):
    return np.asarray(ref.window_rows(c["guide"], len(c["codes"]), c["t_lo"], c["t_hi"] - c["t_lo"]))


def shape_cases():
    """L + 2 on both sides of every boundary, with T = L, L + 1, 2 L and 8 L + 5, the guide the full path's own first steps; at T = 2 L the
    same read under every other guide of the list"""
    rng = np.random.default_rng(300)
    out = []
    for S in STATE_COUNTS:
        L = S - 2
        codes = rng.integers(0, 4, L)
        for T in (L, L + 1, 2 * L, 8 * L + 5):
            lead = 0 if T <= L + 1 else int(rng.integers(0, 2)) * ((T - L) // 3)
            trail = 0 if T <= L + 1 else int(rng.integers(0, 2)) * ((T - L) // 3)
            raw = sc.signal(rng, codes, T, lead, trail)
            full = full_of(raw, codes, MODEL, 0, T, **SCALE)
            assert full["status"] == fref.OK
            own = np.asarray(full["first"], dtype=np.int64)
            mk = lambda tag, kind, guide, cond: out.append(_case(f"S{S}_T{T}_{tag}", kind, raw, codes, guide, cond=cond, **SCALE))
            mk("own", "own", own, lambda o, f: same(o, f) and o["n_edge"] == 0)
            if T != 2 * L:
                continue
            for k in (30, 31, 32, 33, -30, -31, -32, -33):
                inside = -31 <= k <= 30                      # the path sits at lo + 31 - k: inside while 1 <= 31 - k <= 62
                mk(f"shift{k:+d}", "inside" if inside else "rim", shift(own, k, 0, T),
                   (lambda o, f: same(o, f)) if inside or S <= W else
                   (lambda o, f: o["status"] == ref.OFF_BAND or (o["status"] == ref.OK and (o["n_edge"] > 0 or o["score"] >= f["score"]))))
            mid = int(own[L // 2])
            mk("const", "const", np.full(L, mid), lambda o, f, S=S: same(o, f) if S <= W else o["status"] in (ref.OK, ref.OFF_BAND))
            # (lo(0) = 1 still holds state 1, which starts a path: the window is lost from lo(0) = 2 on, L + 2 >= 66)
            mk("before", "before", np.full(L, -5), lambda o, f, S=S: same(o, f) if S <= W else (o["status"] == ref.OFF_BAND or S == W + 1))
            mk("after", "after", np.full(L, T + 7), lambda o, f, S=S: same(o, f) if S <= W else (o["status"] == ref.OFF_BAND or S == W + 1))
            runs = own.copy()
            runs[1::2] = runs[0:L - 1:2][:len(runs[1::2])]   # every second base repeats the value before it: skipped bases
            mk("runs", "runs", runs, lambda o, f: same(o, f))
            # the guide eventalign on event rows gives on the same read: an event every 3 samples, skips at 96
            starts = np.arange(0, T, 3)
            ev = eref.events_of(raw, starts)
            eo = eref.align_numpy(ev, T, codes, MODEL, SCALE["m2"], SCALE["d4"], 96, 0)
            assert eo["status"] == eref.OK
            mk("events", "events", np.asarray(eo["start"]), None)
    return out


def jump_cases():
    """the window's lowest state rises by exactly 63, 64 and 65 in one row: that many bases of the guide share one value"""
    rng = np.random.default_rng(301)
    L = 1023
    codes = rng.integers(0, 4, L)
    raw = sc.signal(rng, codes, 3 * L, 50, 50)
    full = full_of(raw, codes, MODEL, 0, 3 * L, **SCALE)
    own = np.asarray(full["first"], dtype=np.int64)
    out = []
    for j in (63, 64, 65):
        g = own.copy()
        g[400:400 + j] = g[400]
        c = _case(f"jump{j}", "jump", raw, codes, g, **SCALE)
        c["cond"] = lambda o, f, c=c, j=j: int(np.diff(lo_rows(c)).max()) == j and o["status"] in (ref.OK, ref.OFF_BAND)
        out.append(c)
    return out


def edge_cases():
    """_eventalign_cases' edge cases (windows, scales, T = 1, T < L, every status, the clamp, the cap, ties: all with L + 2 <= 64, so any
    guide gives rd_eventalign), ties with a window that slides, and the value bound at T = 2^19"""
    rng = np.random.default_rng(302)
    out = []
    for c in sc.edge_cases():
        L = len(c["codes"])
        guide = np.sort(rng.integers(-50, len(c["raw"]) + 50, L))
        out.append(_case("e_" + c["name"], "edge", c["raw"], c["codes"], guide, c["t_lo"], c["t_hi"], c["m2"], c["d4"],
                         cond=lambda o, f, cc=c["cond"]: same(o, f) and cc(f)))
    # a constant signal on a homopolymer of 100 bases, nearer the background's level than the base's: the lead keeps every sample it can and
    # every base takes one sample, the last 100; every compare between two base states ties.  The guide says so
    out.append(_case("tie_const_slide", "own", np.full(300, 717), np.full(100, 1), 200 + np.arange(100), d4=240, m2=1200,
                     cond=lambda o, f: same(o, f) and f["first"] == list(range(200, 300))))
    # T = 2^19, every cell at the cap plus the largest bias: the values end at 2^19 * 1280.  Every compare ties, so the path advances only
    # where it must: under a diagonal guide it rides the window's upper rim
    T, L = 1 << 19, 200
    out.append(_case("bound_2p19", "bound", np.full(T, 32767), rng.integers(0, 4, L), (np.arange(L) * (T // L)), d4=16, m2=1200, model=BOUND_MODEL,
                     cond=lambda o, f: o["status"] == ref.OK and o["score"] == (1 << 19) * 1280 and o["n_edge"] > 0))
    return out


def all_cases():
    if "cases" not in _cache:
        _cache["cases"] = shape_cases() + jump_cases() + edge_cases()
        assert len({c["name"] for c in _cache["cases"]}) == len(_cache["cases"])
    return _cache["cases"]


def small_cases():
    """the cases the plain-Python restatement can do in a moment"""
    return [c for c in all_cases() if (c["t_hi"] - c["t_lo"]) * min(len(c["codes"]) + 2, W) <= 20000]


def groups(cases=None):
    """[(model, [case])]: the batches"""
    cases = all_cases() if cases is None else cases
    return [(m, [c for c in cases if c["model"] is m]) for m in (MODEL, BOUND_MODEL) if any(c["model"] is m for c in cases)]


def reference(case):
    """the banded restatement's output of a case (the NumPy twin), computed once"""
    key = ("ref", case["name"])
    if key not in _cache:
        _cache[key] = ref.align_numpy(case["raw"], case["codes"], case["guide"], case["model"], case["t_lo"], case["t_hi"], case["m2"], case["d4"])
    return _cache[key]


def full_reference(case):
    """_eventalign_ref's output on the same read and scale, computed once (the bound case: its path is known, see edge_cases)"""
    key = ("full", case["name"].rsplit("_", 1)[0] if case["kind"] not in ("edge", "bound", "jump") and "_T" in case["name"] else case["name"])
    if key not in _cache:
        if case["kind"] == "bound":
            _cache[key] = None
        else:
            _cache[key] = full_of(case["raw"], case["codes"], case["model"], case["t_lo"], case["t_hi"], case["m2"], case["d4"])
    return _cache[key]


def call_args(cases):
    """-> what Backend.eventalign_banded / eventalign_banded_host take besides the model"""
    return dict(raws=[c["raw"] for c in cases], seqs=[c["codes"] for c in cases], guides=[c["guide"] for c in cases], t_lo=[c["t_lo"] for c in cases],
                t_hi=[c["t_hi"] for c in cases], m2=[c["m2"] for c in cases], d4=[c["d4"] for c in cases])


def full_args(cases):
    a = call_args(cases)
    del a["guides"]
    return a


def backend_model(m=MODEL):
    from radian_amd.backend import EvalModel
    return EvalModel(m.k, m.lvl, np.array(m.w, dtype=np.uint64).astype(np.uint32), m.bias, m.bg)
