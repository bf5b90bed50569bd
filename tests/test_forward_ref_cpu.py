"""tests/_forward_ref.py -- the float64 statement of the forward that tests/test_gpu_forward_logratio.py holds the HIP kernels to -- checked
here, without a GPU:

  * it IS the graph: with the inter-layer rounding off it equals the stock-PyTorch statement (tests/test_forward_torch_cpu.py) to 1e-9,
    and with it on the oracle's float64-accumulated rows lie inside the CPU-float32 yardstick of the same case;
  * the blind spot it closes is real: on the stock weights most rows hold a class above 1 - 1e-4 and a dropped conv tap passes
    |d softmax| <= 1e-4;
  * the criterion the GPU test applies (centred log-ratios within 3 x the yardstick, max and rms) sees every fault of the catalogue on
    every weight set and input of the GPU test: structural faults by >= 100 x the bound, a low term lost in one conv above the bound in
    rms, lost in every layer by 3 x.

The log-ratios `u_c = ln p_c - mean_c ln p_c` are the logits minus their row mean: what a softmax row still says about the network's
output when no class is saturated, which is why the cases use a soft head (`soft_weights`, last Dense kernel x 0.05)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _forward_ref as R  # noqa: E402

CASES = R.cases()
_clean = {}


def _reference(wi, ci):
    """(flat, cache of the clean exact run, its softmax rows, their log-ratios) of weight set wi on case ci, computed once"""
    if (wi, ci) not in _clean:
        seed, dil = R.WEIGHT_SETS[wi]
        flat = R.soft_weights(seed, dil)
        _, x, valid = CASES[ci]
        cache = {}
        p = R.softmax64(R.logits64(flat, x, dil, cache=cache, valid=valid))
        _clean[wi, ci] = (flat, cache, p, R.clr(p))
    return _clean[wi, ci]


@pytest.mark.parametrize("wi", range(len(R.WEIGHT_SETS)), ids=lambda i: "seed%d_d%s" % (R.WEIGHT_SETS[i][0], "_".join(map(str, R.WEIGHT_SETS[i][1]))))
def test_restatement_is_the_graph(oracle, wi):
    pytest.importorskip("torch")
    from test_forward_torch_cpu import _torch_forward
    seed, dil = R.WEIGHT_SETS[wi]
    flat = R.soft_weights(seed, dil)
    for name in ("windows_T33", "windows_T300"):
        ci = [c[0] for c in CASES].index(name)
        _, x, valid = CASES[ci]
        ref = _torch_forward(flat, x, dil)                                   # float64 throughout
        got = R.softmax64(R.logits64(flat, x, dil, rounded=False))
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-9 and np.abs(R.clr(got) - R.clr(ref)).max() <= 1e-9, (name, np.abs(R.clr(got) - R.clr(ref)).max())
        # float32 between layers: the oracle with float64 accumulation rounds at the same places (and a few more), so it must sit
        # inside what the all-float32 oracle differs by
        _, cache, p, E = _reference(wi, ci)
        ymax, yrms = R.yardstick(oracle, flat, x, dil, ref=cache["logits"])
        amax, arms = R.distance(oracle.tcn_forward(flat, x, dilations=dil, acc64=True), E)
        print(f"{name} seed {seed} dilations {dil}: yardstick max {ymax:.2e} rms {yrms:.2e}; acc64 oracle max {amax:.2e} rms {arms:.2e}")
        assert amax <= ymax and arms <= yrms, (name, amax, ymax, arms, yrms)
        for mode in ("f16x3", "bf16x3"):                                     # the split statements are the same function to ~2^-22
            dm, dr = R.distance(R.softmax64(R.logits64(flat, x, dil, mode=mode)), E)
            assert dm <= ymax, (name, mode, dm, ymax)


def test_soft_cases_are_unsaturated():
    """every input of the GPU test, on every weight set: the smallest reference probability of a kept row is >= 2^-10"""
    for wi, (seed, dil) in enumerate(R.WEIGHT_SETS):
        for ci, (name, x, valid) in enumerate(CASES):
            p = _reference(wi, ci)[2]
            pmin = float(p[R.keep_mask(*x.shape, valid)].min())
            assert pmin >= R.P_MIN, (seed, dil, name, pmin)


def test_stock_weights_hide_a_dropped_tap():
    """The bench's He-normal weights (head gain 1): most rows saturated, and the catalogue's faults measured both ways.  A conv tap
    dropped on the first row of every 128-row tile moves the logits by several units and the softmax by less than the 1e-4 every
    other forward test applies."""
    from radian_amd import weights
    flat, dil = weights.synthetic_weights(seed=1234), R.DEFAULT
    name, x, valid = CASES[[c[0] for c in CASES].index("windows_T129")]
    cache = {}
    z = R.logits64(flat, x, dil, cache=cache)
    p = R.softmax64(z)
    E = R.clr(p)
    span = z.max(axis=-1) - z.min(axis=-1)
    saturated = float((p.max(axis=-1) > 1 - 1e-4).mean())
    print(f"stock weights seed 1234, {name}: logit span median {np.median(span):.1f} max {span.max():.1f}, rows with a class above 1 - 1e-4: "
          f"{100 * saturated:.0f} %, smallest probability {p.min():.1e}")
    assert saturated >= 0.5
    hidden = []
    for f in R.catalogue(dil):
        pf = R.softmax64(R.logits64(flat, x, dil, fault=f, cache=cache))
        du, dp = R.distance(pf, E)[0], float(np.abs(pf - p).max())
        print(f"  {f.name:45s} max|d log-ratio| {du:9.3e}   max|d softmax| {dp:9.3e}")
        if f.structural and dp <= 1e-4:
            assert du >= 1.0                      # ... while the logits moved by whole units
            hidden.append(f.name)
    assert "tap_dropped_first_row_of_every_tile" in hidden, hidden


@pytest.mark.parametrize("wi", range(len(R.WEIGHT_SETS)), ids=lambda i: "seed%d_d%s" % (R.WEIGHT_SETS[i][0], "_".join(map(str, R.WEIGHT_SETS[i][1]))))
def test_criterion_sees_every_fault(oracle, wi):
    """bound = 3 x yardstick per case, max and rms separately (what the GPU test applies).  Prints, per fault, the smallest ratio of its
    distance to the bound over the cases it reaches, and the cases it cannot reach."""
    seed, dil = R.WEIGHT_SETS[wi]
    faults = R.catalogue(dil)
    ratio = {f.name: [] for f in faults}
    unreached = {f.name: [] for f in faults}
    for ci, (name, x, valid) in enumerate(CASES):
        flat, cache, p, E = _reference(wi, ci)
        ymax, yrms = R.yardstick(oracle, flat, x, dil, valid=valid, ref=cache["logits"])
        for f in faults:
            if not R.fault_reaches(f, x.shape[1], valid):
                unreached[f.name].append(name)
                continue
            dm, dr = R.distance(R.softmax64(R.logits64(flat, x, dil, fault=f, cache=cache, valid=valid)), E, valid)
            rm, rr = dm / (3 * ymax), dr / (3 * yrms)
            ratio[f.name].append((rm, rr))
            if f.structural:
                assert max(rm, rr) >= 100, (f.name, name, rm, rr)
            elif f.block is None:
                assert rr >= 3, (f.name, name, rr)
            else:
                assert rr > 1, (f.name, name, rr)
    print(f"seed {seed} dilations {dil}: distance / bound, smallest over the cases a fault reaches")
    for f in faults:
        r = ratio[f.name]
        assert len(r) >= 2, (f.name, "bites on fewer than two cases")
        print(f"  {f.name:45s} cases {len(r):2d}  max {min(a for a, _ in r):10.1f}  rms {min(b for _, b in r):10.2f}"
              + (f"   not reached: {', '.join(unreached[f.name])}" if unreached[f.name] else ""))
