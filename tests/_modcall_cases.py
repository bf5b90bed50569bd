"""The seeded cases of the modcall tests (tests/test_modcall_cpu.py asserts every case's defining condition without a GPU and holds
rd_modcall_host to the restatement on them; tests/test_gpu_modcall.py runs them on the device).  A CASE is one read of one call with its
jobs: {"name", "raw" int16, "codes" uint8, "m2", "d4", "first", "last" int32 per base, "jobs": [(alt_first, [(lvl, w, bias)])], "group",
"cond": callable(outs) -> bool} where outs are _modcall_ref's dicts, one per job.  Model and flank belong to the call, so a batch is
the cases of one group: GROUPS[group] = (model, flank).  The restatements of a case are computed once and shared."""
import numpy as np

import _eventalign_cases as sc
import _eventalign_ref as fref
import _modcall_ref as ref

MEDIAN, D4 = sc.MEDIAN, sc.D4
SCALE = dict(m2=2 * MEDIAN, d4=D4)
_cache = {}


def small_model(k, seed):
    """a model of any k: levels within +-1600, weights of sd 8 .. 400, biases over +-256"""
    rng = np.random.default_rng(seed)
    n = 4 ** k
    sd = rng.choice([8, 30, 79, 150, 400], n)
    w = np.minimum(np.rint(16.0 * 2.0 ** 32 / (sd * sd)), 2.0 ** 32 - 1).astype(np.uint64)
    return fref.Model(k, rng.integers(-1600, 1601, n), w, rng.integers(-256, 257, n), (0, 0, 0))


def flat_model(lvl, w, biases):
    """k = 1: the four bases' entries share lvl and w and take the four biases"""
    return fref.Model(1, [lvl] * 4, [w] * 4, biases, (0, 0, 0))


# (model, flank) of a call
GROUPS = {
    "k3": (sc.MODEL, 6),
    "k1": (small_model(1, 11), 0),
    "k1f1": (small_model(1, 12), 1),
    "k5": (small_model(5, 13), 6),
    "k9": (small_model(9, 14), 6),
    "wide": (sc.MODEL, 27),
    "cap": (flat_model((1 << 14) - 1, (1 << 32) - 1, [256] * 4), 27),      # every cost at the cap, bias +256
    "zero": (flat_model(0, 0, [-256] * 4), 27),                             # every cost 0, bias -256: the lower bound of fwd
    "d132": (flat_model(0, 0, [0, 132, -133, 134]), 1),                     # w = 0: a cell costs its bias, whatever the sample
}


def _case(name, group, raw, codes, first, last, jobs, m2=SCALE["m2"], d4=SCALE["d4"], cond=None):
    return dict(name=name, group=group, raw=np.ascontiguousarray(raw, dtype=np.int16), codes=np.ascontiguousarray(codes, dtype=np.uint8),
                first=np.ascontiguousarray(first, dtype=np.int32), last=np.ascontiguousarray(last, dtype=np.int32), m2=int(m2), d4=int(d4),
                jobs=[(int(a), [tuple(int(v) for v in e) for e in alts]) for a, alts in jobs],
                cond=cond or (lambda outs: all(o["status"] == ref.OK for o in outs)))


def read_of(rng, model, codes, dwell, lead=0, trail=0, noise=20):
    """samples at the bases' levels for dwell[b] samples each (0: a base without rows, steps -1) between lead and trail samples of noise
    -> (raw, first, last)"""
    L = len(codes)
    dwell = np.asarray(dwell, dtype=np.int64)
    lv = np.array([model.lvl[fref.kmer(codes, b, model.k)] for b in range(L)], dtype=np.float64)
    T = lead + int(dwell.sum()) + trail
    x = np.concatenate([np.zeros(lead), np.repeat(lv, dwell), np.zeros(trail)]) * D4 / 1024 + MEDIAN + rng.normal(0, noise, T)
    start = lead + np.concatenate([[0], np.cumsum(dwell)[:-1]])
    first = np.where(dwell > 0, start, -1)
    last = np.where(dwell > 0, start + dwell - 1, -1)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16), first, last


def shifted(model, codes, b, dz=256):
    """base b's own entry with its level moved by dz (MAD/256)"""
    i = fref.kmer(codes, b, model.k)
    return (model.lvl[i] + dz, model.w[i], model.bias[i])


def dwell_summing(rng, S, R):
    """S dwells of at least 1 that sum to R"""
    return 1 + rng.multinomial(R - S, np.full(S, 1.0 / S))


def window_of(c, j):
    F = GROUPS[c["group"]][1]
    a, alts = c["jobs"][j]
    return ref.window(c["first"], c["last"], len(c["codes"]), len(c["raw"]), a, len(alts), F)


def shape_cases():
    out = []
    rng = np.random.default_rng(310)
    # S = 1: one base, no flank; R = S and R = S + 1
    m = GROUPS["k1"][0]
    for R in (1, 2):
        raw, first, last = read_of(rng, m, [2], [R])
        out.append(_case(f"S1_R{R}", "k1", raw, [2], first, last, [(0, [shifted(m, [2], 0)])], cond=lambda o, R=R: o[0]["n_states"] == 1 and o[0]["n_rows"] == R))
    # S = 2: two bases, flank 1, either base (the window clipped at a0 = 0 and at a1 = L - 1)
    m = GROUPS["k1f1"][0]
    codes = [1, 3]
    raw, first, last = read_of(rng, m, codes, [3, 4], lead=2, trail=2)
    out.append(_case("S2_both_ends", "k1f1", raw, codes, first, last, [(0, [shifted(m, codes, 0)]), (1, [shifted(m, codes, 1)])],
                     cond=lambda o: all(v["n_states"] == 2 and v["n_rows"] == 7 for v in o)))
    # n_alt = 1, 5, 9 with k = 1, 5, 9; k = 9 at flank 6 is S = 21
    for g, n_alt in (("k1f1", 1), ("k5", 5), ("k9", 9)):
        m, F = GROUPS[g]
        L = 40
        codes = rng.integers(0, 4, L)
        raw, first, last = read_of(rng, m, codes, 1 + rng.poisson(8, L), lead=5, trail=5)
        jobs = [(a, [shifted(m, codes, a + i, 256 if i == n_alt // 2 else 40) for i in range(n_alt)]) for a in (0, 15, L - n_alt)]
        S_mid = n_alt + 2 * F
        out.append(_case(f"{g}_nalt{n_alt}", g, raw, codes, first, last, jobs,
                         cond=lambda o, S_mid=S_mid, n_alt=n_alt, F=F: [v["n_states"] for v in o] == [n_alt + F, S_mid, n_alt + F] and all(v["status"] == 0 for v in o)))
    # S = 62 and 63 (flank 27, n_alt 8 and 9) with R = S, S + 1 and a few tiles
    m, F = GROUPS["wide"]
    for n_alt in (8, 9):
        S = n_alt + 2 * F
        for R in sorted({S, S + 1, 64, 65, 300}):
            L = S + 4
            codes = rng.integers(0, 4, L)
            dwell = np.concatenate([[3, 2], dwell_summing(rng, S, R), [2, 3]])
            raw, first, last = read_of(rng, m, codes, dwell)
            out.append(_case(f"S{S}_R{R}", "wide", raw, codes, first, last, [(2 + F, [shifted(m, codes, 2 + F + i) for i in range(n_alt)])],
                             cond=lambda o, S=S, R=R: o[0]["status"] == 0 and o[0]["n_states"] == S and o[0]["n_rows"] == R))
    # S = 13 (k = 3, flank 6) at the tile edges
    m, F = GROUPS["k3"]
    for R in (13, 14, 63, 64, 65, 127, 128, 129, 1000):
        codes = rng.integers(0, 4, 20)
        dwell = np.concatenate([[4, 4, 4], dwell_summing(rng, 13, R), [4, 4, 4, 4]])
        raw, first, last = read_of(rng, m, codes, dwell)
        out.append(_case(f"S13_R{R}", "k3", raw, codes, first, last, [(9, [shifted(m, codes, 9)])],
                         cond=lambda o, R=R: o[0]["status"] == 0 and o[0]["n_states"] == 13 and o[0]["n_rows"] == R))
    return out


def extreme_cases():
    out = []
    rng = np.random.default_rng(311)
    S, R = 63, ref.MAX_R
    codes = rng.integers(0, 4, S)
    dwell = dwell_summing(rng, S, R)
    first = np.concatenate([[0], np.cumsum(dwell)[:-1]])
    last = first + dwell - 1
    far = np.full(R, -3000, dtype=np.int16)                  # zq far below the level 2^14 - 1: every cell at the cap
    alts = [((1 << 14) - 1, (1 << 32) - 1, 256)] * 9
    out.append(_case("cap_2p15", "cap", far, codes, first, last, [(27, alts)],
                     cond=lambda o: o[0]["status"] == 0 and o[0]["vit_ref"] == (1 << 15) * 1280 and o[0]["fwd_ref"] <= o[0]["vit_ref"]))
    out.append(_case("zero_2p15", "zero", far, codes, first, last, [(27, [(0, 0, -256)] * 9)],
                     cond=lambda o: o[0]["status"] == 0 and o[0]["vit_ref"] == -(1 << 15) * 256 and o[0]["fwd_ref"] > -(1 << 15) * 278))
    # one row more: TOO_LONG, beside a job of the same read that is not
    last2 = last.copy()
    last2[-1] += 1
    far2 = np.full(R + 1, -3000, dtype=np.int16)
    out.append(_case("too_long", "zero", far2, codes, first, last2, [(27, [(0, 0, -256)] * 9), (0, [(5, 7, 9)])],
                     cond=lambda o: o[0]["status"] == ref.TOO_LONG and o[1]["status"] == 0))
    # real levels over 2^15 rows
    m = GROUPS["wide"][0]
    raw, first, last = read_of(rng, m, codes, dwell)
    out.append(_case("wide_2p15", "wide", raw, codes, first, last, [(27, [shifted(m, codes, 27 + i) for i in range(9)])],
                     cond=lambda o: o[0]["status"] == 0 and o[0]["n_rows"] == 1 << 15))
    # stay and advance exactly 132, 133 and 134 apart: w = 0 and state 0 costs 0, so with b the bias of state 1, row 1 leaves (0, b) and
    # row 2 of state 1 sees stay = b and advance = 0.  The second job puts -b in b's place
    for c1, b in ((1, 132), (2, -133), (3, 134)):
        want = lambda b: (b + min(b, 0), b + min(b, 0) - (1 if abs(b) == 132 else 0))   # LSE[132] = 1, LSE[133] = LSE[min(134, 133)] = 0
        out.append(_case(f"diff{abs(b)}", "d132", [600, 600, 600], [0, c1], [0, 1], [0, 2], [(0, [(0, 0, 0)]), (1, [(0, 0, -b)])],
                         cond=lambda o, b=b, want=want: (o[0]["vit_ref"], o[0]["fwd_ref"]) == want(b) == (o[0]["vit_alt"], o[0]["fwd_alt"]) and
                         (o[1]["vit_alt"], o[1]["fwd_alt"]) == want(-b) and (o[1]["vit_ref"], o[1]["fwd_ref"]) == want(b)))
    return out


def status_cases():
    out = []
    rng = np.random.default_rng(312)
    m, F = GROUPS["k3"]
    L = 30
    codes = rng.integers(0, 4, L)
    dwell = 1 + rng.poisson(9, L)
    dwell[3] = 0            # a base without rows: the anchor a0 of a job at base 9, the anchor a1 of none
    dwell[20] = 0
    raw, first, last = read_of(rng, m, codes, dwell, lead=10, trail=10)
    jobs = [(9, [shifted(m, codes, 9)]),            # a0 = 3: NO_ANCHOR
            (14, [shifted(m, codes, 14)]),          # a1 = 20: NO_ANCHOR
            (12, [shifted(m, codes, 12)]),          # 6 .. 18: OK
            (12, [shifted(m, codes, 12)]),          # two jobs at one site
            (12, [shifted(m, codes, 12, 0)]),       # alt equal to ref
            (25, [shifted(m, codes, 25)])]          # clipped at a1 = L - 1
    out.append(_case("anchors", "k3", raw, codes, first, last, jobs,
                     cond=lambda o: [v["status"] for v in o] == [1, 1, 0, 0, 0, 0] and o[2] == o[3] and o[4]["vit_alt"] == o[4]["vit_ref"] and
                     o[4]["fwd_alt"] == o[4]["fwd_ref"] and o[2]["fwd_alt"] != o[2]["fwd_ref"]))
    # R < S; rows past the read's end; rows before its start
    codes = rng.integers(0, 4, 16)
    raw, first, last = read_of(rng, m, codes, np.full(16, 5))
    short = last.copy()
    short[14] = first[2] + 11     # job at 8: a0 = 2, a1 = 14, S = 13, R = 12
    past = last.copy()
    past[15] = len(raw)           # job at 12: a1 = 15
    before = first.copy()
    before[0] = -3                # job at 3: a0 = 0
    out.append(_case("short", "k3", raw, codes, first, short, [(8, [shifted(m, codes, 8)]), (3, [shifted(m, codes, 3)])],
                     cond=lambda o: [v["status"] for v in o] == [ref.NO_PATH, 0]))
    out.append(_case("past_end", "k3", raw, codes, first, past, [(12, [shifted(m, codes, 12)]), (3, [shifted(m, codes, 3)])],
                     cond=lambda o: [v["status"] for v in o] == [ref.NO_PATH, 0]))
    out.append(_case("before_start", "k3", raw, codes, before, last, [(3, [shifted(m, codes, 3)]), (9, [shifted(m, codes, 9)])],
                     cond=lambda o: [v["status"] for v in o] == [ref.NO_PATH, 0]))
    # a read without jobs between reads that have some, and a window that ends on the read's last sample (this case sorts last in its group)
    raw, first, last = read_of(rng, m, codes, np.full(16, 5))
    out.append(_case("no_jobs", "k3", raw, codes, first, last, [], cond=lambda o: o == []))
    raw, first, last = read_of(rng, m, codes, 1 + rng.poisson(6, 16), lead=7, trail=0)
    out.append(_case("zz_ends_on_last_sample", "k3", raw, codes, first, last, [(12, [shifted(m, codes, 12)]), (1, [shifted(m, codes, 1)])],
                     cond=lambda o, n=len(raw), l15=int(last[15]): all(v["status"] == 0 for v in o) and l15 == n - 1 and o[0]["n_rows"] % 64 != 0))
    return out


def all_cases():
    if "cases" not in _cache:
        _cache["cases"] = shape_cases() + extreme_cases() + status_cases()
        assert len({c["name"] for c in _cache["cases"]}) == len(_cache["cases"])
    return _cache["cases"]


def groups():
    """-> {group: its cases, the one whose window ends on the last sample of the batch last}"""
    out = {}
    for c in all_cases():
        out.setdefault(c["group"], []).append(c)
    return {g: sorted(cs, key=lambda c: c["name"].startswith("zz_")) for g, cs in out.items()}


def reference(case):
    """the restatement's outputs of a case's jobs (the NumPy twin; test_modcall_cpu.py holds it to the plain version), computed once"""
    key = ("ref", case["name"])
    if key not in _cache:
        model, F = GROUPS[case["group"]]
        _cache[key] = [ref.job_numpy(case["raw"], case["codes"], case["m2"], case["d4"], case["first"], case["last"], model, a, alts, F)
                       for a, alts in case["jobs"]]
    return _cache[key]


def plain(case):
    model, F = GROUPS[case["group"]]
    return [ref.job_plain(case["raw"], case["codes"], case["m2"], case["d4"], case["first"], case["last"], model, a, alts, F) for a, alts in case["jobs"]]


def is_small(case):
    """can the plain-Python restatement do it in a moment?"""
    return all(window_of(case, j)[4] * window_of(case, j)[2] <= 40000 for j in range(len(case["jobs"])))


def backend_model(group):
    from radian_amd.backend import EvalModel
    m = GROUPS[group][0]
    return EvalModel(m.k, m.lvl, np.array(m.w, dtype=np.uint64).astype(np.uint32), m.bias, m.bg)


def call_args(cases, order=None):
    """-> (what Backend.modcall / modcall_host take but the model and the flank, jobs -> (case index, job index)); order: a permutation
    of the flattened jobs"""
    flat = [(ci, ji) for ci, c in enumerate(cases) for ji in range(len(c["jobs"]))]
    if order is not None:
        flat = [flat[i] for i in order]
    jobs = [cases[ci]["jobs"][ji] for ci, ji in flat]
    alts = [(np.array([e[0] for e in a], np.int32), np.array([e[1] for e in a], np.uint64).astype(np.uint32), np.array([e[2] for e in a], np.int32))
            for _, a in jobs]
    return dict(raws=[c["raw"] for c in cases], seqs=[c["codes"] for c in cases], m2=[c["m2"] for c in cases], d4=[c["d4"] for c in cases],
                firsts=[c["first"] for c in cases], lasts=[c["last"] for c in cases], job_read=[ci for ci, _ in flat],
                alt_first=[a for a, _ in jobs], alts=alts), flat
