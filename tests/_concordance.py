"""End-to-end concordance of a basecall against the all-CPU path: inputs, the CPU path itself and the classifier of a differing
sequence.  Plain Python plus oracle calls; nothing here touches the GPU (tests/test_concordance_cpu.py checks this file without one,
tests/test_gpu_e2e_concordance.py uses it against the device).

The beam search is discontinuous in its input, so a forward within the project's tolerance of the oracle's can still change a call.
`explain` says whether a changed sequence is what such a tolerance can do (two candidates within the reach of the perturbation, or an
LM gate whose entropy test fell on the other side) or is something else."""
import functools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 1024
OUTLIER_CLIP = 4
FORWARD_TOL = 1e-4          # the project's bound on |softmax(GPU) - softmax(oracle)| (test_gpu_forward.py)
LM_K = 3
S_THRESHOLD = R_THRESHOLD = 0.5
# the global default geometry (step 128) on the whole signals would be 200+ windows: these cuts keep it at 65
TRUNCATE = (3000, None, 700, 2600, 1024)

CONFIGS = {
    "chunk_w1": dict(route="chunk", signals="full", step=512, W=1, lm=False),            # BASELINE configs[0]
    "chunk_w10": dict(route="chunk", signals="full", step=512, W=10, lm=False),          # BASELINE configs[2]
    "global_default": dict(route="global", signals="truncated", step=128, W=6, lm=True),  # the reference's defaults
}
WEIGHT_SETS = {"soft": dict(seed=77, head_gain=0.3),          # labelings of the size real models give (hundreds of bases per read)
               "he": dict(seed=1234)}                         # the bench's weights: peaky rows, 4-31 bases per read


def lm_dict(k=LM_K):
    """the synthetic k-mer model of test_gpu_cli._make_inputs, as the dict its JSON holds"""
    rng = np.random.default_rng(21)
    raw = {}
    for i in range(4 ** k):
        ctx = "".join("ACGT"[(i >> (2 * (k - 1 - j))) & 3] for j in range(k))
        raw[ctx] = [float(x) for x in rng.dirichlet([0.3] * 4)]
    return raw


@functools.lru_cache(maxsize=None)
def inputs():
    """-> dict: ids, full (the five golden signals), truncated (TRUNCATE applied: read 2 is the single-window float32 case, the
    others assemble to float64), weights {name: flat float32}, lm_table [4^k, 4], lm_k."""
    from radian_amd import lm, weights
    ids = json.load(open(os.path.join(GOLDEN, "reads_fast5_ids.json")))["read_ids"]
    sig = np.load(os.path.join(GOLDEN, "reads_fast5_signals.npz"))
    full = [np.ascontiguousarray(sig[r]) for r in ids]
    trunc = [s if n is None else np.ascontiguousarray(s[:n]) for s, n in zip(full, TRUNCATE)]
    table, k = lm.table_from_dict(lm_dict())
    return {"ids": list(ids), "full": full, "truncated": trunc, "lm_table": table, "lm_k": k,
            "weights": {name: weights.synthetic_weights(**kw) for name, kw in WEIGHT_SETS.items()}}


NO_LM = (None, 0.0, 0.0, 0)


def lm_args(cfg):
    """the decoder's LM arguments (table, s_threshold, r_threshold, len_context) of a configuration"""
    return (inputs()["lm_table"], S_THRESHOLD, R_THRESHOLD, inputs()["lm_k"]) if cfg["lm"] else NO_LM


def _oracle():
    from oracle import oracle as orc          # (test infrastructure; built by build() or by the `oracle` fixture)
    orc.build()
    return orc


def windows_of(raws, step):
    """mad_normalise(., 4) -> get_windows(., 1024, step) per read -> (windows float32 [n, 1024] of all reads, first window per read
    [reads + 1], pad of each read's last window)"""
    oracle = _oracle()
    wins, off, pads = [], [0], []
    for raw in raws:
        w, pad = oracle.get_windows(oracle.mad_normalise(raw, OUTLIER_CLIP), CHUNK, step)
        wins.append(np.asarray(w, dtype=np.float32))
        off.append(off[-1] + len(w))
        pads.append(int(pad))
    return np.concatenate(wins), off, pads


def labels_to_str(labels):
    return "".join("ACGT"[c] for c in labels)


def decode_probs(probs, off, pads, cfg):
    """The CPU path behind the forward, on window probabilities [n, 1024, 5] of all reads (the oracle's or the device's).
    -> per read {"mats": the matrices its searches read, "labels": one uint8 array per matrix, "fasta": the record's sequence}.
    Chunk route: one matrix per window, the pad trimmed from the last; global route: the one assembled matrix."""
    oracle, lm = _oracle(), lm_args(cfg)
    out = []
    for r in range(len(pads)):
        p = probs[off[r]: off[r + 1]]
        if cfg["route"] == "chunk":
            mats = [p[i] if i < len(p) - 1 else p[i][: CHUNK - pads[r]] for i in range(len(p))]
            labels = [oracle.beam_search_labels(m, cfg["W"])[0] for m in mats]
            seq = oracle.chunk_consensus([labels_to_str(l) for l in labels])
        else:
            mats = [oracle.assemble_matrices(p, pads[r], cfg["step"])]
            labels = [oracle.beam_search_labels(mats[0], cfg["W"], *lm)[0]]
            seq = labels_to_str(labels[0])
        out.append({"mats": mats, "labels": labels, "fasta": seq[::-1]})
    return out


def cpu_path(weights, raws, cfg, acc64=False, probs=None):
    """The whole path on the CPU: normalise, windows, tcn_forward (acc64: every dot product summed in float64), decode, stitch.
    probs: tcn_forward's output for these very windows, where a caller already holds it (configurations that share windows)."""
    win, off, pads = windows_of(raws, cfg["step"])
    if probs is None:
        probs = _oracle().tcn_forward(weights, win, acc64=acc64)
    assert probs.shape == win.shape + (5,)
    return decode_probs(probs, off, pads, cfg)


# ---------------------------------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------------------------------
def ranked(M, t, W, lm):
    """L(M, t): the final BeamList of the prefix M[:t], sorted as the search sorts it, whole (a step keeps at most 5 W + 1 entries) --
    the candidates step t + 1 prunes.  -> [(labeling, pr_total)]"""
    _, final = _oracle().beam_search_labels(M[:t], W, *lm, max_final=5 * W + 1)
    return [(f[0], f[1]) for f in final]


def log_reach(M_c, M_g, t):
    """E(t) = sum over rows u < t of max_c |log M_g[u, c] - log M_c[u, c]| in float64.  A candidate's pr_total is the log of a sum of
    products of one entry (or, behind an open LM gate, one positive combination of entries) per row, so between the two matrices it
    moves by at most E(t)."""
    a = np.asarray(M_c[:t], dtype=np.float64)
    b = np.asarray(M_g[:t], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(np.log(b) - np.log(a))
    d[(a == 0) & (b == 0)] = 0.0          # (a zero on one side only stays inf: no bound)
    return float(d.max(axis=1).sum()) if t else 0.0


def _gate_rows(M_c, M_g, t, lm):
    """rows u < t whose LM gate decides differently on the two matrices: [(u, entropy under M_c, entropy under M_g)]"""
    oracle = _oracle()
    table, s_thr, r_thr, _ = lm
    probe = np.array([0.4, 0.3, 0.2, 0.05, 0.05])
    # a context whose own entropy passes r_threshold; without one the gate never opens and no row can flip it
    if not any(not np.array_equal(oracle.apply_rna_model(probe, c, table, math.inf, r_thr, s_thr), probe) for c in range(len(table))):
        return []
    rows = []
    for u in range(t):
        ec, eg = oracle.row_entropy(M_c[u]), oracle.row_entropy(M_g[u])
        if (ec > s_thr) != (eg > s_thr):
            rows.append((u, ec, eg))
    return rows


def explain(M_c, M_g, W, lm=NO_LM):
    """Classify one sequence whose labels differ between M_c (the CPU path's matrix) and M_g (the other side's).

    Bisects to a step t with L(M_c, t-1) == L(M_g, t-1) and L(M_c, t) != L(M_g, t): equal ranked lists at t-1 give both searches the
    same candidates at t.  Two candidates can swap places only if their pr_total under M_c are within 2 E(t) of each other.
      near-tie     every pair the two lists order differently is within 2 E(t) + 1e-9 (float64 rounding slack; 2 E(t) is the derived
                   figure, nothing is tuned), and no row < t differs by more than FORWARD_TOL
      gate-flip    (LM) a row < t has its entropy on the other side of s_threshold; `gate_rows` lists each with both entropies
      unexplained  anything else: a different candidate set, a swap across a gap the perturbation cannot close, or a perturbation
                   over the forward's tolerance (E(t) bounds whatever the matrices differ by, so without this last condition a
                   matrix that is simply wrong would excuse itself with its own large E)
    -> dict(verdict, t, E, max_dp, min_gap, max_gap, pairs, gate_rows, labels_c, labels_g)"""
    T = M_c.shape[0]
    assert M_g.shape == M_c.shape and M_g.dtype == M_c.dtype
    lc, lg = ranked(M_c, T, W, lm), ranked(M_g, T, W, lm)
    rep = {"verdict": "unexplained", "t": None, "E": None, "max_dp": None, "min_gap": None, "max_gap": None, "pairs": 0,
           "gate_rows": [], "labels_c": lc[0][0], "labels_g": lg[0][0]}
    if [x[0] for x in lc] == [x[0] for x in lg]:
        rep["why"] = "the ranked lists of the whole sequence are equal: nothing to explain"
        return rep
    lo, hi = 0, T
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if [x[0] for x in ranked(M_c, mid, W, lm)] == [x[0] for x in ranked(M_g, mid, W, lm)]:
            lo = mid
        else:
            hi = mid
    t = hi
    lc, lg = ranked(M_c, t, W, lm), ranked(M_g, t, W, lm)
    rep["t"] = t
    rep["E"] = E = log_reach(M_c, M_g, t)
    rep["max_dp"] = float(np.abs(np.asarray(M_g[:t], dtype=np.float64) - np.asarray(M_c[:t], dtype=np.float64)).max())
    rep["labels_c"], rep["labels_g"] = lc[0][0], lg[0][0]
    if len(lc) != len(lg) or {x[0] for x in lc} != {x[0] for x in lg}:
        rep["why"] = "the two searches hold different candidates at step t"
        return rep
    tot = dict(lc)
    pos_g = {x[0]: i for i, x in enumerate(lg)}
    gaps = []
    for i in range(len(lc)):
        for j in range(i + 1, len(lc)):
            X, Y = lc[i][0], lc[j][0]
            if pos_g[X] > pos_g[Y]:
                gaps.append(0.0 if tot[X] == tot[Y] else abs(tot[X] - tot[Y]))
    rep["pairs"], rep["min_gap"], rep["max_gap"] = len(gaps), min(gaps), max(gaps)
    if lm[0] is not None:
        rep["gate_rows"] = _gate_rows(M_c, M_g, t, lm)
    if not rep["max_dp"] <= FORWARD_TOL:
        rep["why"] = f"rows below t differ by {rep['max_dp']:.3g}, over the forward's tolerance {FORWARD_TOL:g}"
    elif rep["gate_rows"]:
        rep["verdict"] = "gate-flip"
    elif rep["max_gap"] <= 2.0 * E + 1e-9:
        rep["verdict"] = "near-tie"
    else:
        rep["why"] = f"a pair {rep['max_gap']:.3g} apart changed order; the matrices can move a candidate by E = {E:.3g} at most"
    return rep


def format_report(rep):
    s = (f"{rep['verdict']}: t={rep['t']} E(t)={rep['E']} max|dp|={rep['max_dp']} reordered pairs={rep['pairs']} "
         f"gap min={rep['min_gap']} max={rep['max_gap']} cpu={rep['labels_c'][-24:]!r} other={rep['labels_g'][-24:]!r}")
    if rep["gate_rows"]:
        s += " gate rows " + ", ".join(f"{u}: {ec:.9g} / {eg:.9g}" for u, ec, eg in rep["gate_rows"][:4])
    return s + (" -- " + rep["why"] if rep.get("why") else "")


def concordance(cpu, got, W, lm):
    """Compare the per-read results of two runs (cpu_path's structure) sequence by sequence.
    -> dict(records, same_records, sequences, same_sequences, max_dp, reports [(read, sequence, explain's dict)])"""
    res = {"records": len(cpu), "same_records": sum(a["fasta"] == b["fasta"] for a, b in zip(cpu, got)), "sequences": 0,
           "same_sequences": 0, "max_dp": 0.0, "reports": []}
    for r, (a, b) in enumerate(zip(cpu, got)):
        assert len(a["mats"]) == len(b["mats"])
        for i, (mc, mg) in enumerate(zip(a["mats"], b["mats"])):
            res["sequences"] += 1
            if mc.size:
                res["max_dp"] = max(res["max_dp"], float(np.abs(mg.astype(np.float64) - mc.astype(np.float64)).max()))
            if np.array_equal(a["labels"][i], b["labels"][i]):
                res["same_sequences"] += 1
            else:
                res["reports"].append((r, i, explain(mc, mg, W, lm)))
    return res


def summary_line(name, res):
    kinds = [rep["verdict"] for _, _, rep in res["reports"]]
    excused = kinds.count("near-tie") + kinds.count("gate-flip")
    big_e = max([rep["E"] for _, _, rep in res["reports"] if rep["E"] is not None], default=0.0)
    return (f"{name}: identical records {res['same_records']}/{res['records']}, identical sequences {res['same_sequences']}/{res['sequences']}, "
            f"max|dp| {res['max_dp']:.3g}, excused {excused} (near-tie {kinds.count('near-tie')}, gate-flip {kinds.count('gate-flip')}), "
            f"largest E(t) {big_e:.3g}")


def cap(n_sequences):
    """excused sequences allowed: 5 % of the configuration's sequences, rounded up"""
    return -(-5 * n_sequences // 100)
