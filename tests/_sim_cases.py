"""TEST INFRASTRUCTURE: the seeded cases of the signal-simulation tests (tests/test_sim_cpu.py, tests/test_gpu_sim.py).  A group is one call:
a model, reads and their per-read parameters.  Sizes follow the sample kernel: a workgroup takes a tile of S = 2048 consecutive samples of
one read (csrc/sim_rules.h SIM_TILE).  The `fixed` model makes lengths exact: k = 1 and a constant cdf of 65536 give code 0 a dwell of 1,
code 1 of 30, code 2 of 32767 (the clamp) and code 3 of 100, whatever the random numbers."""
import numpy as np

import _sim_ref as ref

S = 2048
FIXED_DWELL = (1, 30, 32767, 100)


def exp_cdf(f=0.2):
    """the command's dwell quantiles: a floor of f plus an exponential of mean 1 - f, in Q16"""
    return np.rint(65536 * (f + (1 - f) * -np.log(1 - (np.arange(1024) + 0.5) / 1024))).astype(np.int64)


def fixed_model():
    return dict(k=1, level_q10=np.array([-1500, -300, 40, 1400]), sd_q10=np.array([300, 41, 307, 0]),
                dwell_q8=np.array([256, 30 * 256, 1 << 23, 100 * 256]), dwell_cdf=np.full(1024, 65536))


def random_model(k, seed, sd=307, mean_dwell=30):
    rng = np.random.default_rng(seed)
    n = 4 ** k
    return dict(k=k, level_q10=rng.integers(-1536, 1537, n), sd_q10=np.full(n, sd) if sd is not None else rng.integers(0, 600, n),
                dwell_q8=rng.integers(mean_dwell * 128, mean_dwell * 512, n), dwell_cdf=exp_cdf())


def _group(name, model, seqs, seed, lead=400, lead_level=2048, lead_sd=307, median=600, scale=91091, shift=None, dscale=None):
    n = len(seqs)
    rng = np.random.default_rng(seed)
    per = lambda a: np.broadcast_to(np.asarray(a, dtype=np.int64), (n,)).copy()
    return dict(name=name, model=model, seqs=[np.asarray(s, dtype=np.uint8) for s in seqs], lead=per(lead), lead_level=per(lead_level),
                lead_sd=per(lead_sd), median=per(median), scale=per(scale), keys=rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32),
                shift=shift, dscale=dscale)


def fixed_group():
    """lengths and base starts placed by hand on the tile grid"""
    z = lambda n: np.zeros(n, np.uint8)
    seqs, lead = [], []
    for n in (0, 1, S - 1, S, S + 1, 2 * S + 1):          # reads that are a lead alone: 0 (empty), 1, S - 1, S, S + 1, 2 S + 1 samples
        seqs.append(z(0)), lead.append(n)
    seqs.append([2]), lead.append(0)                       # one base of 32767 samples: 16 tiles
    seqs.append([1, 2, 1]), lead.append(100)               # the long base starts and ends inside a tile
    seqs.append([1, 1, 1]), lead.append(S - 30)            # base 1 starts exactly at S
    seqs.append(z(3 * S + 5)), lead.append(0)              # every dwell 1: a tile holds S base starts; lead 0
    seqs.append(z(S - 1)), lead.append(0)                  # S - 1 samples of S - 1 bases
    seqs.append(z(S)), lead.append(0)
    seqs.append(z(S + 1)), lead.append(0)
    seqs.append([3, 0, 1, 0, 3]), lead.append(2 * S + 77)  # a lead over two tiles
    seqs.append([0, 3, 1]), lead.append(S)                 # a lead that ends on a tile edge
    seqs.append([3] * 41 + [0] * 7), lead.append(2 * S)    # and on the second
    seqs.append([0]), lead.append(0)                       # one sample of one base
    seqs.append([1, 3]), lead.append(S - 29)               # base 1 starts one sample after a tile edge
    return _group("fixed", fixed_model(), seqs, 11, lead=lead)


def fixed_expect(g):
    """(n_samples, base_first) of the fixed group by plain addition"""
    out = []
    for s, ld in zip(g["seqs"], g["lead"]):
        d = np.array([FIXED_DWELL[c] for c in s], dtype=np.int64)
        out.append((int(ld + d.sum()), (ld + np.concatenate([[0], np.cumsum(d)[:-1]])).astype(np.int64) if len(s) else np.zeros(0, np.int64)))
    return out


def k_group(k, seed):
    """L = 0, 1, h and h + 1 and longer reads; leads 0, S and over 2 S; per-base shifts and scales with their limits among them"""
    rng = np.random.default_rng(seed)
    h = k // 2
    Ls = [0, 1, max(h, 1), h + 1, 2 * h + 1, 57, 300, 701]
    seqs = [rng.integers(0, 4, L).astype(np.uint8) for L in Ls]
    lead = [0, 0, 3, 0, S, 2 * S + 1, 400, 0]
    shift = [rng.integers(-400, 401, L) for L in Ls]
    dscale = [rng.integers(64, 1025, L) for L in Ls]
    shift[6][:4], dscale[6][:4] = [-32768, 32767, 0, -1], [1, 4096, 256, 4095]
    shift[7][-2:], dscale[7][-2:] = [32767, -32768], [4096, 1]
    return _group(f"k{k}", random_model(k, seed, sd=None), seqs, seed + 1, lead=lead, median=[600, -5, 0, 32767, -32768, 600, 611, 589],
                  scale=[91091, 1, 1 << 26, 91091, 91091, 50000, 120000, 91091], shift=shift, dscale=dscale)


def clamp_group():
    """raw clamps at both ends (a scale of 2^26 turns one z unit into 65536 DAQ units; lead levels and sds at their limits); sd 0"""
    rng = np.random.default_rng(5)
    m = random_model(5, 5)
    m["sd_q10"] = np.where(np.arange(1024) % 3 == 0, 0, m["sd_q10"])
    m["sd_q10"][0] = 1 << 15
    m["level_q10"][1], m["level_q10"][2] = 1 << 15, -(1 << 15)
    seqs = [rng.integers(0, 4, 80).astype(np.uint8), np.zeros(40, np.uint8), rng.integers(0, 4, 80).astype(np.uint8), rng.integers(0, 4, 33).astype(np.uint8)]
    return _group("clamp", m, seqs, 6, lead=[50, 9, 0, 64], lead_level=[1 << 15, -(1 << 15), 0, 0], lead_sd=[1 << 15, 0, 0, 1 << 15],
                  median=[0, 32767, -32768, 0], scale=[1 << 26, 1 << 26, 1 << 20, 1])


def many_group():
    """70 reads for the budget cut"""
    rng = np.random.default_rng(70)
    seqs = [rng.integers(0, 4, int(L)).astype(np.uint8) for L in rng.integers(20, 400, 70)]
    seqs[17] = np.zeros(0, np.uint8)
    return _group("many", random_model(5, 71), seqs, 72, lead=rng.integers(0, 600, 70))


def all_groups():
    return [fixed_group(), k_group(1, 21), k_group(5, 25), k_group(9, 29), clamp_group(), many_group()]


def expect(g):
    """the restatement of every read of a group: (n_samples, base_first, raw, status)"""
    return [ref.simulate(g["seqs"][r], g["model"], int(g["lead"][r]), int(g["lead_level"][r]), int(g["lead_sd"][r]), int(g["median"][r]),
                         int(g["scale"][r]), g["keys"][r], None if g["shift"] is None else g["shift"][r],
                         None if g["dscale"] is None else g["dscale"][r]) for r in range(len(g["seqs"]))]


def model_of(g):
    from radian_amd.backend import SimModel
    return SimModel(**g["model"])


def call_args(g, idx=None):
    """(positional arguments, keyword arguments) of Backend.sim_signal / sim_signal_host for the group's reads idx (all of them)"""
    idx = list(range(len(g["seqs"]))) if idx is None else list(idx)
    pick = lambda a: None if a is None else [a[i] for i in idx]
    return ([g["seqs"][i] for i in idx], model_of(g), g["lead"][idx], g["lead_level"][idx], g["lead_sd"][idx], g["median"][idx], g["scale"][idx],
            g["keys"][idx]), dict(level_shift=pick(g["shift"]), dwell_scale=pick(g["dscale"]))


def same(res, r, exp, who=""):
    """read r of a SimResult against one entry of expect()"""
    n, bf, raw, st = exp
    assert res.raw[r].dtype == np.int16 and res.base_first[r].dtype == np.int32, who
    assert int(res.status[r]) == st and len(res.raw[r]) == n, (who, r, int(res.status[r]), len(res.raw[r]), n)
    assert np.array_equal(res.base_first[r], bf), (who, r, "base_first")
    assert np.array_equal(res.raw[r], raw), (who, r, "raw", int(np.argmax(res.raw[r] != raw)))


# ---------------------------------------------------------------------------------------------- refusals, through the raw C entry points
def raw_inputs(g):
    """the sixteen leading arguments of rd_sim_* as numpy arrays by name"""
    from radian_amd.backend import _concat_codes, _pack
    codes, off = _concat_codes(g["seqs"])
    m = g["model"]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(codes=codes, seq_off=off, n_reads=len(g["seqs"]), shift=None if g["shift"] is None else _pack(g["shift"], np.int16, pad=1)[0],
                dscale=None if g["dscale"] is None else _pack(g["dscale"], np.uint16, pad=1)[0], lead=i32(g["lead"]), lead_level=i32(g["lead_level"]),
                lead_sd=i32(g["lead_sd"]), median=i32(g["median"]), scale=i32(g["scale"]), key=np.ascontiguousarray(g["keys"], dtype=np.uint32).ravel(),
                k=int(m["k"]), level=i32(m["level_q10"]), sd=i32(m["sd_q10"]), dwell=i32(m["dwell_q8"]), cdf=np.ascontiguousarray(m["dwell_cdf"], dtype=np.uint32))


ORDER = ("codes", "seq_off", "n_reads", "shift", "dscale", "lead", "lead_level", "lead_sd", "median", "scale", "key", "k", "level", "sd", "dwell", "cdf")


def raw_args(a):
    from radian_amd.backend import _p
    return [a[n] if n in ("n_reads", "k") else _p(a[n]) for n in ORDER]


def refusal_cases():
    """-> (good inputs with raw_off, [(name, inputs)]): every one of the bad ones is RD_ERR_ARG"""
    g = k_group(5, 25)
    good = raw_inputs(g)
    ns = [e[0] for e in expect(g)]
    good["raw_off"] = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    bad = []

    def mut(name, key, fn):
        a = dict(good)
        if fn is None:
            a[key] = None
        else:
            a[key] = good[key].copy() if isinstance(good[key], np.ndarray) else good[key]
            a[key] = fn(a[key])
        bad.append((name, a))

    def setv(i, v):
        def f(x):
            x[i] = v
            return x
        return f
    for key in ("codes", "seq_off", "lead", "lead_level", "lead_sd", "median", "scale", "key", "level", "sd", "dwell", "cdf", "raw_off"):
        mut(f"null {key}", key, None)
    mut("negative n_reads", "n_reads", lambda n: -1)
    mut("k even", "k", lambda k: 4)
    mut("k 0", "k", lambda k: 0)
    mut("k 11", "k", lambda k: 11)
    mut("offsets decrease", "seq_off", setv(3, 0))
    mut("negative offset", "seq_off", setv(0, -1))
    mut("code 4", "codes", setv(100, 4))
    mut("code 255", "codes", setv(-1, 255))
    mut("negative lead", "lead", setv(2, -1))
    mut("lead level", "lead_level", setv(0, (1 << 15) + 1))
    mut("lead sd negative", "lead_sd", setv(1, -1))
    mut("lead sd large", "lead_sd", setv(1, (1 << 15) + 1))
    mut("median", "median", setv(4, 32768))
    mut("scale 0", "scale", setv(5, 0))
    mut("scale large", "scale", setv(5, (1 << 26) + 1))
    mut("level entry", "level", setv(1023, -(1 << 15) - 1))
    mut("sd entry", "sd", setv(0, -1))
    mut("dwell entry small", "dwell", setv(7, 255))
    mut("dwell entry large", "dwell", setv(7, (1 << 23) + 1))
    mut("cdf decreases", "cdf", setv(500, 0))
    mut("cdf large", "cdf", setv(1023, (1 << 20) + 1))
    mut("dwell scale 0", "dscale", setv(9, 0))
    mut("dwell scale 4097", "dscale", setv(9, 4097))
    mut("raw_off short by one", "raw_off", lambda x: np.concatenate([x[:-1], [x[-1] - 1]]))
    mut("raw_off shifted inside", "raw_off", setv(4, int(good["raw_off"][4]) + 1))
    mut("raw_off decreases", "raw_off", setv(6, 0))
    mut("raw_off negative", "raw_off", lambda x: x - 1 - x[0])
    return good, bad
