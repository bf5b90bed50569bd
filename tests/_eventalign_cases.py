"""The seeded cases of the eventalign tests (tests/test_eventalign_cpu.py asserts every case's defining condition without a GPU and holds
rd_eventalign_host to the restatement on them; tests/test_gpu_eventalign.py runs them on the device).  A CASE is one read of one call:
{"name", "raw" int16, "codes" uint8, "t_lo", "t_hi", "m2", "d4", "cond": callable(out) -> bool} where out is _eventalign_ref's dict.
Every case shares MODEL, so any subset of them is one batch.  The restatement of a case is computed once (reference()) and shared."""
import numpy as np

import _eventalign_ref as ref

# the kernel's boundaries (eventalign.hip): 16 states per lane, 32 per back-pointer word, 1024 per wave, 4096 per band -- in states, L + 2 of them
LANE, WORD, WAVE, BAND = 16, 32, 1024, 4096
STATE_COUNTS = (2, 3, 4, LANE - 1, LANE, LANE + 1, WORD - 1, WORD, WORD + 1, WAVE - 1, WAVE, WAVE + 1, BAND - 1, BAND, BAND + 1)
K = 3
MEDIAN, D4 = 600, 240     # DAQ units: x = MEDIAN + l D4 / 1024 for a level l in MAD / 256


def random_model(seed=5):
    """k = 3; levels within +-1600 and the two ends of their range, weights from a spread of 8 (the sd floor) up and the 2^32 - 1 clamp,
    biases over +-256"""
    rng = np.random.default_rng(seed)
    n = 4 ** K
    lvl = rng.integers(-1600, 1601, n)
    sd = rng.choice([8, 30, 79, 150, 400], n)
    w = np.minimum(np.rint(16.0 * 2.0 ** 32 / (sd * sd)), 2.0 ** 32 - 1).astype(np.uint64)
    bias = rng.integers(-256, 257, n)
    lvl[0], w[0], bias[0] = -(1 << 14) + 1, (1 << 32) - 1, -256      # the ends of every range in one entry ...
    lvl[n - 1], w[n - 1], bias[n - 1] = (1 << 14) - 1, 0, 256         # ... and in another (w = 0: the distance does not count)
    lvl[21], lvl[22] = 500, 500                                        # equal neighbouring levels: CCC -> CCG
    w[21] = w[22] = int(w[21])
    bias[21] = bias[22] = int(bias[21])
    return ref.Model(K, lvl, w, bias, (0, int(16 * 2 ** 32 / (380 * 380)), 0))


MODEL = random_model()


def signal(rng, codes, T, lead, trail, noise=20):
    """T samples: `lead` of background, every base at its k-mer's level for at least one sample, `trail` of background"""
    L = len(codes)
    body = T - lead - trail
    assert body >= L
    dwell = np.ones(L, dtype=np.int64)
    if L:
        dwell += rng.multinomial(body - L, np.full(L, 1.0 / L))
    else:
        lead += body
    lv = np.array([MODEL.lvl[ref.kmer(codes, b, K)] for b in range(L)], dtype=np.float64)
    x = np.concatenate([np.zeros(lead), np.repeat(lv, dwell), np.zeros(trail)]) * D4 / 1024 + MEDIAN + rng.normal(0, noise, T)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _case(name, raw, codes, t_lo=0, t_hi=None, m2=0, d4=0, cond=None):
    raw = np.ascontiguousarray(raw, dtype=np.int16)
    return dict(name=name, raw=raw, codes=np.ascontiguousarray(codes, dtype=np.uint8), t_lo=int(t_lo), t_hi=len(raw) if t_hi is None else int(t_hi),
                m2=int(m2), d4=int(d4), cond=cond or (lambda o: o["status"] == ref.OK))


def shape_cases():
    """L on both sides of every boundary the kernel has, with T = L, L + 1, 2 L and about 8 L"""
    rng = np.random.default_rng(240)
    out = []
    for S in STATE_COUNTS:
        L = S - 2
        codes = rng.integers(0, 4, L)
        for T in sorted({max(L, 1), L + 1, max(2 * L, 2), 8 * L + 5}):
            lead = 0 if T <= L + 1 else int(rng.integers(0, 2)) * ((T - L) // 3)      # empty and non-empty lead and trail
            trail = 0 if T <= L + 1 else int(rng.integers(0, 2)) * ((T - L) // 3)
            m2, d4 = (2 * MEDIAN, D4) if T < 8 else (0, 0)      # (a handful of samples has no MAD to speak of: the scale is given)
            out.append(_case(f"S{S}_T{T}", signal(rng, codes, T, lead, trail), codes, m2=m2, d4=d4,
                             cond=lambda o, L=L: o["status"] == ref.OK and (L == 0 or (o["first"][0] >= 0 and o["end"][L - 1] > o["start"][L - 1]))))
    return out


def edge_cases():
    rng = np.random.default_rng(241)
    out = []
    codes = rng.integers(0, 4, 40)
    x = signal(rng, codes, 700, 100, 100)
    m2, d4 = ref.window_scale(x[100:650])
    # window edges
    out.append(_case("win_lo0", x, codes, 0, 650, cond=lambda o: o["status"] == ref.OK and o["first"][0] >= 0))
    out.append(_case("win_hi_n", x, codes, 100, 700, cond=lambda o: o["status"] == ref.OK and o["first"][0] >= 100 and o["last"][-1] <= 699))
    out.append(_case("win_inner", x, codes, 100, 650, cond=lambda o: o["status"] == ref.OK and o["first"][0] >= 100 and o["last"][-1] <= 649))
    out.append(_case("win_empty", x, codes, 300, 300, cond=lambda o: o["status"] == ref.EMPTY and o["first"] == [-1] * 40 and o["d4"] == 0))
    # d4 given against d4 computed: the same read, the same scale
    out.append(_case("scale_given", x, codes, 100, 650, m2, d4, cond=lambda o, s=(m2, d4): o["status"] == ref.OK and (o["m2"], o["d4"]) == s))
    out.append(_case("scale_other", x, codes, 100, 650, m2 + 37, d4 + 11, cond=lambda o, s=(m2 + 37, d4 + 11): (o["m2"], o["d4"]) == s))
    # T = 1; T < L
    out.append(_case("T1_L0", [612], [], d4=240, m2=1200))
    out.append(_case("T1_L1", [700], [2], d4=240, m2=1200, cond=lambda o: o["status"] == ref.OK and o["first"] == [0] and o["last"] == [0]))
    out.append(_case("T_lt_L", x[:39], codes, d4=240, m2=1200, cond=lambda o: o["status"] == ref.NO_PATH and o["sums"] == [0] * 5))
    out.append(_case("L0", x[:300], [], cond=lambda o: o["status"] == ref.OK and o["sums"] == [0] * 5))
    # statuses
    out.append(_case("mad_zero", np.full(90, 77), codes[:5], cond=lambda o: o["status"] == ref.MAD_ZERO and (o["m2"], o["d4"]) == (154, 0)))
    out.append(_case("too_long", rng.integers(400, 800, (1 << 19) + 1), codes[:3], cond=lambda o: o["status"] == ref.TOO_LONG and o["m2"] == 0))
    out.append(_case("empty_read", np.zeros(0), codes[:4], cond=lambda o: o["status"] == ref.EMPTY))
    # samples at the +-2^14 clamp (a small d4 puts the int16 extremes far outside), costs at the cap
    y = signal(rng, codes, 400, 30, 30)
    y[50:60], y[200:210] = 32767, -32768
    out.append(_case("clamp", y, codes, d4=16, m2=1200, cond=lambda o: o["status"] == ref.OK and ref.quant(32767, 1200, 16) == 1 << 14
                     and ref.quant(-32768, 1200, 16) == -(1 << 14)))
    far = signal(rng, codes, 400, 30, 30) + 3000        # every sample more than the cap away from every level but the w = 0 entry's
    out.append(_case("cost_cap", far, codes, d4=240, m2=1200, cond=lambda o: o["status"] == ref.OK
                     and ref.cost(ref.quant(3600, 1200, 240), (500, MODEL.w[21], 0)) == ref.CAP))
    # ties: a constant signal on a homopolymer (every boundary is the tie-break's: every base but the last takes one sample, at the start),
    # equal neighbouring levels (CCC and CCG share one model entry here)
    out.append(_case("tie_const", np.full(50, 717), np.full(6, 1), d4=240, m2=1200,
                     cond=lambda o: o["status"] == ref.OK and len(set(o["min"] + o["max"])) == 1))
    cc = np.array([0, 1, 1, 1, 1, 2, 3, 1, 1, 1, 2, 0])
    out.append(_case("tie_levels", signal(rng, cc, 200, 20, 20, noise=0), cc, d4=240, m2=1200,
                     cond=lambda o: MODEL.lvl[21] == MODEL.lvl[22] and ref.kmer(cc, 3, K) == 21 and ref.kmer(cc, 4, K) == 22))
    return out


_cache = {}


def all_cases():
    if "cases" not in _cache:
        _cache["cases"] = shape_cases() + edge_cases()
        assert len({c["name"] for c in _cache["cases"]}) == len(_cache["cases"])
    return _cache["cases"]


def small_cases():
    """the cases the plain-Python restatement can do in a moment"""
    return [c for c in all_cases() if (c["t_hi"] - c["t_lo"]) * (len(c["codes"]) + 2) <= 40000]


def reference(case):
    """the restatement's output of a case (the NumPy twin; test_eventalign_cpu.py holds it to the plain version), computed once"""
    key = ("ref", case["name"])
    if key not in _cache:
        _cache[key] = ref.align_numpy(case["raw"], case["codes"], MODEL, case["t_lo"], case["t_hi"], case["m2"], case["d4"])
    return _cache[key]


def call_args(cases):
    """-> what Backend.eventalign / eventalign_host take after the model"""
    return dict(raws=[c["raw"] for c in cases], seqs=[c["codes"] for c in cases], t_lo=[c["t_lo"] for c in cases], t_hi=[c["t_hi"] for c in cases],
                m2=[c["m2"] for c in cases], d4=[c["d4"] for c in cases])


def backend_model():
    from radian_amd.backend import EvalModel
    return EvalModel(MODEL.k, MODEL.lvl, np.array(MODEL.w, dtype=np.uint64).astype(np.uint32), MODEL.bias, MODEL.bg)


# ------------------------------------------------------------------------------------------------ the simulated reads of the accuracy test
SIM_SEEDS = tuple(range(1, 17))
SIM_K, SIM_MODEL_SEED, SIM_LEAD, SIM_MEDIAN, SIM_SCALE_Q10 = 5, 7, 400, 600, 91091     # 91091 = 60 * 1.4826 * 1024: a MAD of 60, d4 = 240
SIM_ADAPTER, SIM_TAIL, SIM_SLACK = 30, 60, 32


def sim_read(seed):
    """-> (raw, fragment codes in pore order, t_lo, the true first sample of every fragment base)"""
    from radian_amd.backend import SimModel, sim_signal_host
    from radian_amd.simulate import dwell_cdf, standin_tables
    key = ("sim", seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        adapter = rng.integers(0, 4, SIM_ADAPTER)
        L = (200, 300)[int(rng.integers(0, 2))]
        frag = rng.integers(0, 4, L)
        codes = np.concatenate([adapter, np.zeros(SIM_TAIL, dtype=np.int64), frag]).astype(np.uint8)
        model = SimModel(SIM_K, *standin_tables(SIM_K, SIM_MODEL_SEED), dwell_cdf(0.2))
        res = sim_signal_host([codes], model, SIM_LEAD, 2048, 307, SIM_MEDIAN, SIM_SCALE_Q10, np.array([[seed, 99]], dtype=np.uint32))
        first = res.base_first[0][SIM_ADAPTER + SIM_TAIL:].astype(np.int64)
        _cache[key] = (res.raw[0], frag.astype(np.uint8), int(first[0]) - SIM_SLACK, first)
    return _cache[key]


def accuracy(first_got, first_true):
    """-> (within 10, within 30, exact, bases, the largest error) of one read's first samples"""
    err = np.abs(np.asarray(first_got, dtype=np.int64) - first_true)
    return int((err <= 10).sum()), int((err <= 30).sum()), int((err == 0).sum()), len(err), int(err.max())
