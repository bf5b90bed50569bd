"""The seeded cases of the sigmap tests (tests/test_sigmap_cpu.py asserts every case's defining condition without a GPU and holds
rd_sigmap_host to the restatement on them; tests/test_gpu_sigmap.py runs them on the device).  All cases share one PANEL, one MODEL and one
buffer of samples (raw()), so any subset of them is one call.  A CASE is one query:
{"name", "q_lo", "q_hi", "sc_lo", "sc_hi", "m2", "d4", "s_lo", "s_hi", "cond": callable(out) -> bool}, out being _sigmap_ref's dict at
n_best = N_BEST.  The restatement of a case is computed once (reference()) and shared."""
import numpy as np

import _sigmap_ref as ref
from _eventalign_ref import CAP, Model, cost, kmer, quant, window_scale

from radian_amd.backend import SIGMAP_BAND, SIGMAP_PAYLOAD

# the kernel's boundaries (sigmap.hip): 16 states per lane, 1024 per wave, 4096 per band, the stripe's payload
LANE, WAVE, BAND, P = 16, 1024, SIGMAP_BAND, SIGMAP_PAYLOAD
LENGTHS = (LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, BAND - 1, BAND, BAND + 1, P - 1, P, P + 1)
ROWS = (300, 17, 16, 129, 128, 127, 300, 300, 300, 300, 300, 300)     # T of the query on the target of that length
K = 3
N_BEST = 8
MEDIAN, D4 = 600, 240     # DAQ units: x = MEDIAN + l D4 / 1024 for a level l in MAD / 256
LONG_T = 1 << 14


def make_model(seed=25):
    """k = 3; 64 distinct levels 50 apart in a random order, a spread of 30, biases within +-20 -- and the ends of every range in the
    entries of AAA (w = 2^32 - 1, bias -256) and TTT (w = 0: the distance does not count; bias 256)"""
    rng = np.random.default_rng(seed)
    n = 4 ** K
    lvl = rng.permutation(n) * 50 - 1600
    w = np.full(n, int(16 * 2 ** 32 / (30 * 30)), dtype=np.uint64)
    bias = rng.integers(-20, 21, n)
    lvl[0], w[0], bias[0] = -(1 << 14) + 1, (1 << 32) - 1, -256
    lvl[n - 1], w[n - 1], bias[n - 1] = (1 << 14) - 1, 0, 256
    return Model(K, lvl, w, bias, (0, 0, 0))


MODEL = make_model()
_cache = {}


def _build():
    rng = np.random.default_rng(250)
    names, targets = [], []

    def add(name, codes):
        names.append(name)
        targets.append(np.asarray(codes, dtype=np.uint8))

    add("empty_first", [])
    for L in LENGTHS:
        add(f"L{L}", rng.integers(0, 4, L))
    add("one", [2])
    add("empty_a", [])
    add("empty_b", [])
    add("short40", rng.integers(0, 4, 40))
    tie = rng.integers(0, 4, 200)
    add("tieA", tie)
    add("tieB", tie)
    x = rng.integers(0, 4, 120)
    add("rep", np.concatenate([rng.integers(0, 4, 50), x, rng.integers(0, 4, 50), x, rng.integers(0, 4, 50)]))
    add("joinA", rng.integers(0, 4, 300))
    add("joinB", rng.integers(0, 4, 300))
    add("big", rng.integers(0, 4, 2 * P + 710))
    add("empty_last", [])
    panel = ref.Panel(targets, MODEL)
    J = {n: j for j, n in enumerate(names)}
    lvl_of = panel.arrays()[0]

    chunks, cases, at = [], [], [0]

    def put(x):
        """appends samples to the shared buffer -> (lo, hi)"""
        x = np.clip(np.rint(np.asarray(x, dtype=np.float64)), -32768, 32767).astype(np.int16)
        chunks.append(x)
        at[0] += len(x)
        return at[0] - len(x), at[0]

    def walk(first, n_states, T, noise=5):
        """T samples of a path through the global states first .. first + n_states - 1, every state at least once"""
        assert 1 <= n_states <= T
        dwell = np.ones(n_states, dtype=np.int64) + rng.multinomial(T - n_states, np.full(n_states, 1.0 / n_states))
        return np.repeat(lvl_of[first:first + n_states].astype(np.float64), dwell) * D4 / 1024 + MEDIAN + rng.normal(0, noise, T)

    def case(name, win, s_lo, s_hi, sc=None, m2=2 * MEDIAN, d4=D4, cond=None):
        sc = win if sc is None else sc
        cases.append(dict(name=name, q_lo=win[0], q_hi=win[1], sc_lo=sc[0], sc_hi=sc[1], m2=m2, d4=d4, s_lo=int(s_lo), s_hi=int(s_hi),
                          cond=cond or (lambda o: o["status"] == ref.OK and o["tgt"][0] >= 0)))

    def tgt_range(name):
        return panel.off[J[name]], panel.off[J[name] + 1]

    # target lengths, that is state ranges, on both sides of 16, 1024, 4096 and the payload; T on both sides of 16 and 128, and 300
    for L, T in zip(LENGTHS, ROWS):
        lo, hi = tgt_range(f"L{L}")
        n = min(L, max(1, T // 3))
        first = lo + int(rng.integers(0, L - n + 1))
        case(f"L{L}_T{T}", put(walk(first, n, T)), lo, hi,
             cond=lambda o, j=J[f"L{L}"], L=L, T=T: o["status"] == ref.OK and o["tgt"][:2] == [j, -1] and 0 <= o["org"][0] <= o["end"][0] < L
             and o["end"][0] - o["org"][0] <= T - 1)
    for name, T in (("L16", 1), ("L17", 2), ("L1024", 15)):
        lo, hi = tgt_range(name)
        case(f"{name}_T{T}", put(walk(lo + 3, 1, T)), lo, hi)
    # T = 2^14 on 40 states; one row more is too long
    lo, hi = tgt_range("short40")
    w_long = put(walk(lo, 40, LONG_T + 1))
    case("long_T", (w_long[0], w_long[0] + LONG_T), lo, hi, cond=lambda o: o["status"] == ref.OK and (o["org"][0], o["end"][0]) == (0, 39))
    case("too_long", w_long, lo, hi, cond=lambda o: o["status"] == ref.TOO_LONG and (o["m2"], o["d4"]) == (0, 0) and o["tgt"] == [-1] * N_BEST)
    # the whole panel, n_best = 8; the same samples with the scale computed
    blo, bhi = tgt_range("big")
    w_all = put(walk(blo + 5000, 100, 300))
    m2c, d4c = window_scale(chunks[-1])
    case("panel_given", w_all, 0, panel.R, cond=lambda o: o["status"] == ref.OK and o["tgt"][0] == J["big"] and -1 not in o["tgt"]
         and abs(o["org"][0] - 5000) < 8 and abs(o["end"][0] - 5099) < 8)
    case("panel_computed", w_all, 0, panel.R, m2=0, d4=0,
         cond=lambda o: (o["m2"], o["d4"]) == (m2c, d4c) and (m2c, d4c) != (2 * MEDIAN, D4) and o["tgt"][0] == J["big"])
    # a scale window that is not the query's
    case("scale_window", (w_all[0] + 20, w_all[0] + 220), blo, bhi, sc=(w_all[0] + 10, w_all[1]), m2=0, d4=0,
         cond=lambda o, s=window_scale(chunks[-1][10:]): (o["m2"], o["d4"]) == s and o["status"] == ref.OK)
    # a single-state target; a range of that target, two empty ones and a target shorter than T: n_best above the number of targets
    lo1, hi1 = tgt_range("one")
    case("one_state", put(walk(lo1, 1, 16)), lo1, hi1, cond=lambda o: o["tgt"][:2] == [J["one"], -1] and (o["org"][0], o["end"][0]) == (0, 0))
    case("few_targets", put(walk(lo + 5, 30, 90)), lo1, hi,
         cond=lambda o: sorted(o["tgt"][:2]) == [J["one"], J["short40"]] and o["tgt"][2:] == [-1] * 6 and o["score"][2:] == [-1] * 6
         and o["tgt"][0] == J["short40"] and J["short40"] - J["one"] == 3)
    # the optimum's end on a stripe's last and first state, its origin exactly T - 1 states before the second stripe: a state per row, no noise
    for name, e in (("end_stripe_last", blo + P - 1), ("end_stripe_first", blo + P), ("end_stripe2_last", blo + 2 * P - 1)):
        T = 40
        case(name, put(walk(e - (T - 1), T, T, noise=0)), blo, bhi,
             cond=lambda o, e=e - blo, T=T: o["status"] == ref.OK and o["end"][0] == e and o["org"][0] == e - (T - 1))
    # a band's last state and the next band's first inside one stripe (two bands: the column between them carries the path)
    T = 60
    case("band_crossing", put(walk(blo + BAND - 30, T, T, noise=0)), blo, blo + P,
         cond=lambda o, T=T: (o["org"][0], o["end"][0]) == (BAND - 30, BAND - 30 + T - 1))
    # the join of joinA's end and joinB's start fits better than any one target: it must not be found
    alo, ahi = tgt_range("joinA")
    w_join = put(walk(ahi - 20, 40, 120, noise=5))
    case("join", w_join, alo, ahi + 300,
         cond=lambda o: o["status"] == ref.OK and ref.map_numpy(raw(), PANEL, w_join[0], w_join[1], w_join[0], w_join[1], 2 * MEDIAN, D4, alo, ahi + 300, 1,
                                                                 join=True)["score"][0] < o["score"][0] and set(o["tgt"][:2]) == {J["joinA"], J["joinB"]})
    # s_lo inside a target: the path begins in the range's first state, which is a head without being a target's first
    case("s_lo_inside", put(walk(blo + 100, 41, 123)), blo + 100, blo + 400,
         cond=lambda o: o["status"] == ref.OK and o["tgt"][:2] == [J["big"], -1] and (o["org"][0], o["end"][0]) == (100, 140)
         and not PANEL.first[blo + 100])
    # exact ties: two equal targets (the smaller index first); one target with a repeat (the smaller state)
    tlo, thi = tgt_range("tieA")
    case("tie_targets", put(walk(tlo + 60, 50, 150)), tlo, thi + 200,
         cond=lambda o: o["tgt"][:3] == [J["tieA"], J["tieB"], -1] and o["score"][0] == o["score"][1] and o["end"][0] == o["end"][1])
    rlo, rhi = tgt_range("rep")
    w_rep = put(walk(rlo + 60, 80, 160, noise=0))
    case("tie_within", w_rep, rlo, rhi,
         cond=lambda o: o["end"][0] == 60 + 79 and o["org"][0] == 60 and
         (lambda f: f.count(min(f)) == 2 and f.index(min(f)) == 139 and f[139 + 170] == min(f))(
             ref.map_numpy(raw(), PANEL, w_rep[0], w_rep[1], w_rep[0], w_rep[1], 2 * MEDIAN, D4, rlo, rhi, 1, keep_final=True)["final"]))
    # samples at the +-2^14 clamp (a small d4 puts the int16 extremes far outside); costs at the cap
    y = walk(blo + 300, 40, 200)
    y[50:60], y[120:130] = 32767, -32768
    case("clamp", put(y), blo, blo + 1000, d4=16,
         cond=lambda o: o["status"] == ref.OK and quant(32767, 2 * MEDIAN, 16) == 1 << 14 and quant(-32768, 2 * MEDIAN, 16) == -(1 << 14))
    case("cost_cap", put(walk(blo + 300, 40, 200) + 3000), blo, blo + 1000,
         cond=lambda o: o["status"] == ref.OK and cost(quant(3600, 2 * MEDIAN, D4), (1550, MODEL.w[5], 0)) == CAP and o["score"][0] >= 200 * 256)     # (256: TTT's w = 0 entry)
    # statuses
    w_flat = put(np.full(90, 77))
    case("empty", (w_all[0] + 7, w_all[0] + 7), 0, panel.R, cond=lambda o: o["status"] == ref.EMPTY and (o["m2"], o["d4"]) == (0, 0))
    case("mad_zero", w_flat, blo, bhi, m2=0, d4=0, cond=lambda o: o["status"] == ref.MAD_ZERO and (o["m2"], o["d4"]) == (154, 0) and o["tgt"][0] == -1)
    case("no_scale_window", w_all, blo, bhi, sc=(w_all[0], w_all[0]), m2=0, d4=0, cond=lambda o: o["status"] == ref.MAD_ZERO and (o["m2"], o["d4"]) == (0, 0))
    case("no_target", w_all, lo1 + 1, lo1 + 1, cond=lambda o: o["status"] == ref.NO_TARGET and (o["m2"], o["d4"]) == (2 * MEDIAN, D4) and o["tgt"][0] == -1)
    case("no_target_mad_zero", w_flat, 0, 0, m2=0, d4=0, cond=lambda o: o["status"] == ref.MAD_ZERO)      # the scale comes first
    return panel, J, np.concatenate(chunks), cases


def _get():
    if "built" not in _cache:
        _cache["built"] = _build()
        names = [c["name"] for c in _cache["built"][3]]
        assert len(set(names)) == len(names)
    return _cache["built"]


class _Lazy:
    """PANEL as a module attribute that is built on first use (the cases' conditions name it)"""

    def __getattr__(self, a):
        return getattr(_get()[0], a)


PANEL = _Lazy()


def panel():
    return _get()[0]


def target_index():
    return _get()[1]


def raw():
    return _get()[2]


def all_cases():
    return _get()[3]


def cells(c):
    return (c["q_hi"] - c["q_lo"]) * (c["s_hi"] - c["s_lo"])


def small_cases():
    """the cases the plain-Python restatement can do in a moment"""
    return [c for c in all_cases() if cells(c) <= 40000]


def reference(c, n_best=N_BEST):
    """the restatement's output of a case (the NumPy twin; test_sigmap_cpu.py holds it to the plain version), computed once"""
    key = ("ref", c["name"], n_best)
    if key not in _cache:
        _cache[key] = ref.map_numpy(raw(), panel(), c["q_lo"], c["q_hi"], c["sc_lo"], c["sc_hi"], c["m2"], c["d4"], c["s_lo"], c["s_hi"], n_best)
    return _cache[key]


def call_args(cases):
    """-> what Backend.sigmap / sigmap_host take after the model"""
    return {k: [c[k] for c in cases] for k in ("q_lo", "q_hi", "sc_lo", "sc_hi", "m2", "d4", "s_lo", "s_hi")}


def backend_panel():
    from radian_amd.backend import sigmap_panel
    return sigmap_panel([np.asarray(t, dtype=np.uint8) for t in panel().targets])


def backend_model():
    from radian_amd.backend import EvalModel
    return EvalModel(MODEL.k, MODEL.lvl, np.array(MODEL.w, dtype=np.uint64).astype(np.uint32), MODEL.bias, MODEL.bg)


# ------------------------------------------------------------------------------------------------ the simulated reads of the accuracy test
ACC_K, ACC_MODEL_SEED, ACC_LEAD, ACC_MEDIAN, ACC_SCALE_Q10 = 5, 7, 400, 600, 91091     # 91091 = 60 * 1.4826 * 1024: a MAD of 60, d4 = 240
ACC_ADAPTER, ACC_TAIL, ACC_SHARED, ACC_GENES, ACC_ISOFORMS, ACC_UNRELATED = 30, 60, 600, 8, 3, 16
ACC_QUERY, ACC_PAD, ACC_BEYOND, ACC_READS, ACC_INSIDE = 2048, 8, 100, 36, 8


def accuracy_transcripts():
    """-> (radian_amd.map.Transcripts, the gene of every transcript or -1): eight genes of three isoforms that share their last 600 bases
    and differ in the 300 .. 500 before them, and sixteen unrelated transcripts"""
    from radian_amd.map import Transcripts
    if "acc_tr" not in _cache:
        rng = np.random.default_rng(77)
        seqs, names, gene = [], [], []
        for g in range(ACC_GENES):
            shared = rng.integers(0, 4, ACC_SHARED)
            for i in range(ACC_ISOFORMS):
                seqs.append(np.concatenate([rng.integers(0, 4, int(rng.integers(300, 501))), shared]))
                names.append(f"gene{g}_iso{i}")
                gene.append(g)
        for u in range(ACC_UNRELATED):
            seqs.append(rng.integers(0, 4, int(rng.integers(500, 801))))
            names.append(f"other{u}")
            gene.append(-1)
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        _cache["acc_tr"] = (Transcripts(np.concatenate(seqs).astype(np.uint8), off, names), gene)
    return _cache["acc_tr"]


def accuracy_reads():
    """-> [dict(id, raw, tail_end, t, start, beyond)]: read i is a fragment of transcript t anchored at its 3' end, [start, length) in
    transcript orientation, behind 30 adapter bases and 60 A; the last ACC_INSIDE reads end inside their gene's shared part, the others at
    least ACC_BEYOND bases beyond it.  tail_end is the truth's: the first sample after the bases whose whole k-mer is A"""
    from radian_amd.backend import SimModel, sim_signal_host
    from radian_amd.simulate import dwell_cdf, standin_tables
    if "acc_reads" not in _cache:
        tr, gene = accuracy_transcripts()
        rng = np.random.default_rng(78)
        model = SimModel(ACC_K, *standin_tables(ACC_K, ACC_MODEL_SEED), dwell_cdf(0.2))
        adapter = rng.integers(0, 4, ACC_ADAPTER)
        reads = []
        for i in range(ACC_READS):
            t = (i % ACC_GENES) * ACC_ISOFORMS + (i // ACC_GENES) % ACC_ISOFORMS
            L = tr.length(t)
            beyond = i < ACC_READS - ACC_INSIDE
            n = int(rng.integers(ACC_SHARED + ACC_BEYOND, L + 1)) if beyond else int(rng.integers(300, ACC_SHARED - 40))
            frag = tr.codes[int(tr.offsets[t]) + L - n:int(tr.offsets[t]) + L][::-1]
            codes = np.concatenate([adapter, np.zeros(ACC_TAIL, dtype=np.int64), frag]).astype(np.uint8)
            res = sim_signal_host([codes], model, ACC_LEAD, 2048, 307, ACC_MEDIAN, ACC_SCALE_Q10, np.array([[i + 1, 25]], dtype=np.uint32))
            reads.append(dict(id=f"read{i:02d}", raw=res.raw[0], tail_end=int(res.base_first[0][ACC_ADAPTER + ACC_TAIL - ACC_K // 2]), t=t,
                              start=L - n, beyond=beyond))
        _cache["acc_reads"] = reads
    return _cache["acc_reads"]


def accuracy_args(**kw):
    from types import SimpleNamespace
    return SimpleNamespace(**{**dict(query_samples=ACC_QUERY, start_slack=32, max_cand=8, cand_slack=2.0, max_cost=0.0), **kw})


def accuracy_rows(sig_of=None):
    """the command's two passes over the accuracy reads (and two reads without a bound, the last two rows) through sig_of(panel, model) -> sig; the default is
    rd_sigmap_host, computed once -> (panel, rows)"""
    from radian_amd import sigmap as cmd
    from radian_amd.backend import SigmapPanel, sigmap_host
    from radian_amd.simulate import standin_tables
    key = "acc_rows"
    if sig_of is not None or key not in _cache:
        tr, _ = accuracy_transcripts()
        panel = cmd.Panel(tr, ACC_PAD)
        model = cmd.model_tables(ACC_K, *standin_tables(ACC_K, ACC_MODEL_SEED)[:2])[0]
        reads = accuracy_reads()
        bounds = {r["id"]: r["tail_end"] for r in reads}
        bounds["no_bound_b"] = -1
        sig = sig_of(panel, model) if sig_of else (lambda raw, q_lo, q_hi, **kw: sigmap_host(raw, SigmapPanel(panel.codes, panel.off), model, q_lo, q_hi, **kw))
        batch = [(r["id"], r["raw"]) for r in reads] + [("no_bound_a", reads[0]["raw"]), ("no_bound_b", reads[1]["raw"])]
        rows = cmd.map_batch(sig, batch, panel, bounds, accuracy_args())
        if sig_of is not None:
            return panel, rows
        _cache[key] = (panel, rows)
    return _cache[key]
