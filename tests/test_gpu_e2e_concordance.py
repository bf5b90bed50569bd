"""End to end: the FASTA records of a GPU basecall against the records of a run that never touches the GPU (tests/_concordance.py's
cpu_path: oracle normalise -> windows -> oracle forward -> oracle decode -> stitch), on the five real signals.

Every other end-to-end expectation in the suite decodes the GPU's OWN probabilities with the oracle, and the forward is bounded
separately (|d softmax| <= 1e-4).  The beam search is discontinuous in its input, so those two together do not say how many records of
a GPU job equal the all-CPU job's.  Here each configuration
  1. runs the CLI and the blocking calls on the device,
  2. pins each stage with no exception (forward within 1e-4 of the oracle's on every window; the device's labels == the oracle's decode
     of the device's probabilities; the CLI's records == the records rebuilt from those labels),
  3. compares records and labels with the all-CPU run and sends every differing sequence through _concordance.explain: an
     `unexplained` verdict fails,
  4. caps the excused sequences (near-tie + gate-flip) at 5 % of the configuration's sequences, rounded up: 6 of 103 windows on the chunk
     route, 1 of 5 reads on the global route.  The reference alone (float32 against float64 accumulation, test_concordance_cpu.py) sits at
     0 on these inputs; 5 % is what the oracle shows under uniform noise of +-3e-5 on every entry, three times the forward's documented
     worst case -- a forward that degrades towards the 1e-4 bound breaks the cap while every stage test still passes.
The measured lines are in DESIGN.md section 2."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _concordance as cc


@pytest.fixture(scope="module", params=list(cc.WEIGHT_SETS))
def side(request, oracle):
    """One weight set: the oracle's float32 forward and Backend.forward (exact fp32) of the same oracle-made windows, for the whole
    signals at step 512 and the truncated ones at step 128; computed once."""
    from radian_amd import Backend
    inp = cc.inputs()
    w = inp["weights"][request.param]
    be = Backend(0)
    be.load_weights(w)
    be.set_decode_math("glibc")          # (the CLI's default)
    out = {"name": request.param, "weights": w, "be": be, "cpu": {}}
    for kind, step in (("full", 512), ("truncated", 128)):
        win, off, pads = cc.windows_of(inp[kind], step)
        out[kind] = {"win": win, "off": off, "pads": pads, "P_c": oracle.tcn_forward(w, win), "P_g": be.forward(win)}
    yield out
    be.close()


def _read_fasta(d):
    recs = {}
    for fn in sorted(os.listdir(d)):
        lines = open(os.path.join(d, fn)).read().split("\n")
        for i in range(0, len(lines) - 1, 2):
            recs[lines[i][1:]] = lines[i + 1]
    return recs


def _cli_records(side, cfg, raws, precision, tmp_path):
    """the GPU job: fast5 in, FASTA out, through radian_amd.basecall.main"""
    from radian_amd import basecall, fast5, h5weights
    inp = cc.inputs()
    in_dir, out_dir = tmp_path / "fast5", tmp_path / "fasta"
    in_dir.mkdir()
    out_dir.mkdir()
    fast5.write_multi_fast5(str(in_dir / "reads.fast5"), dict(zip(inp["ids"], raws)))
    if side["name"] == "he":
        model = "synthetic:1234"
    else:
        (tmp_path / "models").mkdir()
        model = str(tmp_path / "models" / "sig2seq.h5")
        h5weights.write_keras_weights(model, side["weights"], dilations=(1, 2, 4, 8, 16, 32), attr_kind="nullpad")
    argv = [str(in_dir), str(out_dir), "--decode-type", cfg["route"], "--step-size", str(cfg["step"]), "--beam-width", str(cfg["W"]),
            "--sig-model", model, "--sig-config", "none", "--precision", precision]
    if cfg["lm"]:
        lm_path = tmp_path / "lm.json"
        lm_path.write_text(json.dumps(cc.lm_dict()))
        argv += ["--rna-model", str(lm_path), "--context-len", str(inp["lm_k"])]          # thresholds: the defaults, 0.5 / 0.5
    else:
        argv += ["--rna-model", "None"]
    basecall.main(argv)
    recs = _read_fasta(str(out_dir))
    assert sorted(recs) == sorted(inp["ids"])
    return [recs[r] for r in inp["ids"]]


def _run(side, cname, precision, tmp_path, oracle):
    inp, cfg, be = cc.inputs(), cc.CONFIGS[cname], side["be"]
    raws, st = inp[cfg["signals"]], side[cfg["signals"]]
    lm = cc.lm_args(cfg)
    # 1. the GPU job, and the labels of every sequence from the blocking calls on the same raws
    records = _cli_records(side, cfg, raws, precision, tmp_path)
    be.set_precision(precision)
    try:
        P_g = st["P_g"] if precision == "fp32" else be.forward(st["win"])
        if cfg["route"] == "chunk":
            gpu_labels, status = be.basecall_raw_chunk(raws, cc.OUTLIER_CLIP, cc.CHUNK, cfg["step"], cfg["W"])
        else:
            be.load_lm(lm[0], lm[3])
            got, status = be.basecall_raw_global(raws, cc.OUTLIER_CLIP, cc.CHUNK, cfg["step"], cfg["W"], True, lm[1], lm[2])
            gpu_labels = [[g] for g in got]
    finally:
        be.set_precision("fp32")
        be.load_lm(None, 0)
    assert status.tolist() == [0] * len(raws)
    # 2. stage attribution: exact, or within the project's tolerance; no exceptions
    n_seq = 103 if cfg["route"] == "chunk" else 5
    assert len(st["win"]) == (103 if cfg["signals"] == "full" else 65)
    max_dp = float(np.abs(P_g.astype(np.float64) - st["P_c"].astype(np.float64)).max())
    print(f"{cname} {side['name']} {precision}: forward max|dp| over {len(st['win'])} windows {max_dp:.3g}")
    assert max_dp <= cc.FORWARD_TOL
    dev = cc.decode_probs(P_g, st["off"], st["pads"], cfg)          # the oracle's assembly / decode / stitch of the device's probabilities
    assert sum(len(x["mats"]) for x in dev) == n_seq
    for r, x in enumerate(dev):
        assert len(gpu_labels[r]) == len(x["labels"]), r
        for i, exp in enumerate(x["labels"]):
            assert np.array_equal(gpu_labels[r][i], exp), f"read {r} sequence {i}: the device's labels are not the oracle's decode of the device's rows"
        if cfg["route"] == "chunk":
            rebuilt = oracle.chunk_consensus([cc.labels_to_str(l) for l in gpu_labels[r]])[::-1]
        else:
            rebuilt = cc.labels_to_str(gpu_labels[r][0])[::-1]
        assert records[r] == rebuilt == x["fasta"], f"read {r}: the CLI's record is not the record of the device's labels"
    # 3. concordance with the run that never touched the GPU
    if cname not in side["cpu"]:
        side["cpu"][cname] = cc.cpu_path(side["weights"], raws, cfg, probs=st["P_c"])
    cpu = side["cpu"][cname]
    gpu = [{"mats": x["mats"], "labels": gpu_labels[r], "fasta": records[r]} for r, x in enumerate(dev)]
    res = cc.concordance(cpu, gpu, cfg["W"], lm)
    print(cc.summary_line(f"{cname} {side['name']} {precision}", res))
    for r, i, rep in res["reports"]:
        print(f"  read {r} sequence {i}: {cc.format_report(rep)}")
    assert res["sequences"] == n_seq and res["records"] == 5
    bad = [(r, i, cc.format_report(rep)) for r, i, rep in res["reports"] if rep["verdict"] not in ("near-tie", "gate-flip")]
    assert not bad, bad
    # 4. the cap: a condition, not a measurement
    assert len(res["reports"]) <= cc.cap(n_seq), [(r, i, cc.format_report(rep)) for r, i, rep in res["reports"]]
    if side["name"] == "soft" and cfg["W"] > 1:
        assert sum(len(x["fasta"]) for x in cpu) > 1000          # labelings of real size: the comparison has something to lose


@pytest.mark.parametrize("cname", list(cc.CONFIGS))
def test_gpu_job_against_all_cpu_run(side, cname, tmp_path, oracle):
    _run(side, cname, "fp32", tmp_path, oracle)


@pytest.mark.parametrize("side", ["soft"], indirect=True)
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_gpu_job_against_all_cpu_run_split_precision(side, precision, tmp_path, oracle):
    """the split-operand matrix modes on chunk_w10 with the soft-head weights: same rules, same cap"""
    _run(side, "chunk_w10", precision, tmp_path, oracle)
