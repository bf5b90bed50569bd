"""The end-to-end concordance helper (tests/_concordance.py) checked without a GPU: the reference path alone stays at zero discordant
sequences under its own float32 summation noise on the inputs the GPU test uses, and the classifier of a changed sequence says
near-tie for changes that small noise makes and unexplained for a change that noise of the forward's tolerance cannot make."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _concordance as cc


@pytest.fixture(scope="module")
def forwards(oracle):
    """oracle forward of a weight set on the windows of a signal set, float32 or float64 accumulation; computed once each"""
    inp = cc.inputs()
    cache = {}

    def get(wname, cfg, acc64):
        key = (wname, cfg["signals"], cfg["step"], acc64)
        if key not in cache:
            win, _, _ = cc.windows_of(inp[cfg["signals"]], cfg["step"])
            cache[key] = oracle.tcn_forward(inp["weights"][wname], win, acc64=acc64)
        return cache[key]
    return get


def test_inputs_are_the_stated_ones(oracle):
    inp = cc.inputs()
    assert [len(s) for s in inp["truncated"]] == [3000, 4863, 700, 2600, 1024]
    assert cc.windows_of(inp["full"], 512)[0].shape == (103, 1024)
    win, off, pads = cc.windows_of(inp["truncated"], 128)
    assert win.shape == (65, 1024)
    P = np.full((65, 1024, 5), 0.2, dtype=np.float32)
    kinds = [oracle.assemble_matrices(P[off[r]: off[r + 1]], pads[r], 128).dtype for r in range(5)]
    assert kinds == [np.float64, np.float64, np.float32, np.float64, np.float64]      # assembled matrices and the single-window case
    assert inp["lm_table"].shape == (64, 4) and inp["lm_k"] == 3
    assert np.array_equal(inp["lm_table"], np.random.default_rng(21).dirichlet([0.3] * 4, size=64))


def test_cap_is_five_percent_rounded_up():
    assert cc.cap(103) == 6 and cc.cap(5) == 1 and cc.cap(100) == 5 and cc.cap(101) == 6


@pytest.mark.parametrize("wname", list(cc.WEIGHT_SETS))
@pytest.mark.parametrize("cname", list(cc.CONFIGS))
def test_null_experiment_reference_alone_has_no_discordance(forwards, cname, wname):
    """cpu_path with float32 and with float64 accumulation: every sequence's labels and every record equal.  The reference's own
    summation noise (max |dp| 7e-6 ... 2.9e-5 here) changes no call on these inputs, so whatever the GPU test has to excuse is the GPU's."""
    inp, cfg = cc.inputs(), cc.CONFIGS[cname]
    raws, w = inp[cfg["signals"]], inp["weights"][wname]
    a = cc.cpu_path(w, raws, cfg, acc64=False, probs=forwards(wname, cfg, False))
    b = cc.cpu_path(w, raws, cfg, acc64=True, probs=forwards(wname, cfg, True))
    res = cc.concordance(a, b, cfg["W"], cc.lm_args(cfg))
    print(cc.summary_line(f"{cname} {wname} fp32 vs fp64 accumulation", res))
    assert res["sequences"] == (103 if cfg["route"] == "chunk" else 5)
    assert 0 < res["max_dp"] <= cc.FORWARD_TOL
    assert res["same_sequences"] == res["sequences"] and not res["reports"]
    assert [x["fasta"] for x in a] == [x["fasta"] for x in b]
    if wname == "soft" and cfg["W"] > 1:
        assert sum(len(x["fasta"]) for x in a) > 1000          # labelings of real size


@pytest.fixture(scope="module")
def soft_chunk_windows(forwards):
    cfg = cc.CONFIGS["chunk_w10"]
    base = cc.cpu_path(None, cc.inputs()["full"], cfg, probs=forwards("soft", cfg, False))
    return [m.astype(np.float64) for r in base for m in r["mats"]], [l for r in base for l in r["labels"]]


def _names(lst):
    return [x[0] for x in lst]


def test_classifier_on_known_flips(oracle, soft_chunk_windows):
    """Uniform noise of +-1e-4 on every entry of the soft-head chunk windows (W = 10, no LM) flips some: each must come back near-tie
    -- without an LM the 2 E(t) bound is rigorous -- at a step where the two searches really part."""
    mats, labels = soft_chunk_windows
    W = 10
    rng = np.random.default_rng(5)
    flips = []
    for _ in range(8):
        for i, m in enumerate(mats):
            mg = np.abs(m + rng.uniform(-1e-4, 1e-4, size=m.shape))          # (reflected at 0: still within 1e-4 of m)
            if not np.array_equal(oracle.beam_search_labels(mg, W)[0], labels[i]):
                flips.append((i, mg))
        if len(flips) >= 5:
            break
    assert len(flips) >= 5
    # noise AT the forward's tolerance on the 103 windows is several times over the GPU test's cap: a forward that degrades towards
    # 1e-4 cannot pass there on excuses
    print(len(flips), "of", len(mats), "windows flipped by the first draw")
    assert len(mats) == 103 and len(flips) > 2 * cc.cap(103)
    for i, mg in flips[:12]:
        rep = cc.explain(mats[i], mg, W)
        print(i, cc.format_report(rep))
        assert rep["verdict"] == "near-tie", cc.format_report(rep)
        t = rep["t"]
        assert 1 <= t <= mats[i].shape[0]
        assert _names(cc.ranked(mats[i], t - 1, W, cc.NO_LM)) == _names(cc.ranked(mg, t - 1, W, cc.NO_LM))
        assert _names(cc.ranked(mats[i], t, W, cc.NO_LM)) != _names(cc.ranked(mg, t, W, cc.NO_LM))
        assert rep["pairs"] >= 1 and 0 <= rep["min_gap"] <= rep["max_gap"] <= 2 * rep["E"] + 1e-9 and rep["max_dp"] <= 1e-4


def test_classifier_negative_control(oracle, soft_chunk_windows):
    """One row's two largest classes swapped: far over the forward's tolerance.  Where that changes the labels the verdict is
    unexplained.  (2 E(t) bounds what ANY two matrices can do to a pair, the swapped row's log ratio included, so the gap rule alone
    would pass this as a near-tie with a large E: the excuse holds only for rows within the forward's tolerance.)"""
    mats, labels = soft_chunk_windows
    m, W = mats[3], 10
    rng = np.random.default_rng(7)
    for _ in range(200):
        u = int(rng.integers(0, m.shape[0]))
        mg = m.copy()
        o = np.argsort(m[u])
        mg[u, o[-1]], mg[u, o[-2]] = m[u, o[-2]], m[u, o[-1]]
        if not np.array_equal(oracle.beam_search_labels(mg, W)[0], labels[3]):
            break
    else:
        pytest.fail("no swapped row changes the labels")
    assert abs(m[u, o[-1]] - m[u, o[-2]]) > 100 * cc.FORWARD_TOL
    rep = cc.explain(m, mg, W)
    print(u, cc.format_report(rep))
    assert rep["verdict"] == "unexplained" and rep["t"] > u and rep["max_dp"] > 100 * cc.FORWARD_TOL
    # equal matrices, or labels that do not differ: never an excuse either
    assert cc.explain(m, m.copy(), W)["verdict"] == "unexplained"


def test_gate_flip_is_reported_with_its_row(oracle):
    """With the LM: a row whose entropy sits at s_threshold, moved across it by a change within the forward's tolerance, changes which
    distribution every gated extension reads.  If the ranked lists part there, the verdict names the row and both entropies."""
    inp = cc.inputs()
    lm = (inp["lm_table"], cc.S_THRESHOLD, cc.R_THRESHOLD, inp["lm_k"])
    rng = np.random.default_rng(11)
    T, W = 60, 6
    found = None
    for _ in range(400):
        m = rng.dirichlet([0.6] * 5, size=T)
        # bring one row's entropy to just under the threshold by sharpening it, then a copy just over
        u = int(rng.integers(8, T))
        row = m[u].copy()
        lo, hi = 0.0, 1.0          # mix with the uniform distribution over the four bases: entropy grows with the mix
        peak = np.array([0.97, 0.01, 0.01, 0.01]) * row[:4].sum()
        flat = np.full(4, row[:4].sum() / 4)
        for _ in range(60):
            mid = (lo + hi) / 2
            r4 = (1 - mid) * peak + mid * flat
            if oracle.row_entropy(np.concatenate([r4, row[4:]])) > cc.S_THRESHOLD:
                hi = mid
            else:
                lo = mid
        a, b = m.copy(), m.copy()
        a[u, :4] = (1 - lo) * peak + lo * flat
        b[u, :4] = (1 - hi) * peak + hi * flat
        if (oracle.row_entropy(a[u]) > cc.S_THRESHOLD) == (oracle.row_entropy(b[u]) > cc.S_THRESHOLD):
            continue
        if not np.array_equal(oracle.beam_search_labels(a, W, *lm)[0], oracle.beam_search_labels(b, W, *lm)[0]):
            found = (a, b, u)
            break
    assert found is not None, "no gate flip changed a labeling"
    a, b, u = found
    assert np.abs(a - b).max() < 1e-9
    rep = cc.explain(a, b, W, lm)
    print(cc.format_report(rep))
    assert rep["verdict"] == "gate-flip" and rep["t"] > u
    assert [g[0] for g in rep["gate_rows"]] == [u]
    (_, ea, eb), = rep["gate_rows"]
    assert (ea > cc.S_THRESHOLD) != (eb > cc.S_THRESHOLD) and abs(ea - eb) < 1e-6


def test_log_reach_bounds_every_total(oracle):
    """E(t) on a random 40-row matrix perturbed by known relative factors: no entry of the final list moves by more than E."""
    rng = np.random.default_rng(3)
    T, W = 40, 10
    m = rng.dirichlet([0.5] * 5, size=T)
    f = rng.uniform(-1e-5, 1e-5, size=m.shape)
    mg = m * np.exp(f)
    E = cc.log_reach(m, mg, T)
    assert E == pytest.approx(np.abs(f).max(axis=1).sum(), rel=1e-6) and 0 < E <= T * 1e-5
    assert cc.log_reach(m, mg, 7) == pytest.approx(np.abs(f[:7]).max(axis=1).sum(), rel=1e-6)
    assert cc.log_reach(m, m, T) == 0.0 and cc.log_reach(m, mg, 0) == 0.0
    z, zg = m.copy(), mg.copy()
    z[2, 1] = zg[2, 1] = 0.0          # a class that is exactly 0 on both sides adds nothing; on one side only there is no bound
    assert np.isfinite(cc.log_reach(z, zg, T))
    zg[2, 1] = 1e-9
    assert cc.log_reach(z, zg, T) == np.inf
    for lm in (cc.NO_LM, (cc.inputs()["lm_table"], 0.0, 9.0, 3)):          # (the second: LM gate open on every row with a context)
        lc, lg = dict(cc.ranked(m, T, W, lm)), dict(cc.ranked(mg, T, W, lm))
        assert len(lc) > W and set(lc) == set(lg)
        moved = max(abs(lc[k] - lg[k]) for k in lc)
        assert 0 < moved <= E, (moved, E)
