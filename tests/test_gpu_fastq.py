"""GPU checks of the fused route rd_basecall_raw_global_q (Backend.basecall_raw_global_q) against its parts, and of
`python -m radian_amd.fastq` against `python -m radian_amd.basecall` on the same directory."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lm_table(k):
    rng = np.random.default_rng(21)
    return {"".join("ACGT"[(i >> (2 * (k - 1 - j))) & 3] for j in range(k)): [float(x) for x in rng.dirichlet([0.3] * 4)] for i in range(4 ** k)}


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("step", [128, 1024], ids=["assembled-f64", "single-coverage-f32"])
def test_fused_route_equals_its_parts(golden_dir, tmp_path, step):
    from radian_amd import Backend, lm, weights
    from radian_amd.backend import CTCALIGN_OK
    ids = json.load(open(os.path.join(golden_dir, "reads_fast5_ids.json")))["read_ids"]
    sig = np.load(os.path.join(golden_dir, "reads_fast5_signals.npz"))
    raws = [np.ascontiguousarray(sig[r][:6000]) for r in ids]
    (tmp_path / "lm.json").write_text(json.dumps(_lm_table(3)))
    table, k = lm.load_json(str(tmp_path / "lm.json"))
    flat = weights.synthetic_weights(seed=1234)
    flat[-645:-5] *= np.float32(0.05)          # soft head: labelings of hundreds of bases
    chunk, W = 1024, 6
    with Backend(0) as be:
        be.load_weights(flat)
        be.load_lm(table, k)
        want, want_status = be.basecall_raw_global(raws, 4, chunk, step, W, True, 0.5, 0.5)
        labels, status, aln = be.basecall_raw_global_q(raws, 4, chunk, step, W, True, 0.5, 0.5)
        assert status.tolist() == want_status.tolist() == [0] * len(raws)
        assert all(np.array_equal(a, b) for a, b in zip(labels, want))
        assert sum(len(l) for l in labels) > 200
        # the matrix the existing API yields for the same reads
        norm, _ = be.normalise_reads(raws, 4)
        probs = be.forward_reads(norm, chunk, step)
        mats = []
        for r, p in enumerate(probs):
            N = len(raws[r])
            mats.append(be.assemble(p, (p.shape[0] - 1) * step + chunk - N, step))
            assert mats[-1].shape == (N, 5) and mats[-1].dtype == (np.float64 if step < chunk else np.float32)
        for r, m in enumerate(mats):
            one = be.ctc_align(m, [0], [m.shape[0]], [labels[r]])
            assert int(aln.status[r]) == int(one.status[0]) == CTCALIGN_OK
            assert _bits(aln.score[r]) == _bits(one.score[0])
            assert np.array_equal(aln.first_step[r], one.first_step[0]) and np.array_equal(aln.last_step[r], one.last_step[0])
            assert np.array_equal(aln.qual[r], one.qual[0])
            assert len(aln.qual[r]) == len(labels[r])
        # the existing call still gives what it gave
        again, _ = be.basecall_raw_global(raws, 4, chunk, step, W, True, 0.5, 0.5)
        assert all(np.array_equal(a, b) for a, b in zip(again, want))


def _write_default_artifacts(cwd, seed, k):
    """models/sig2seq.h5 (Keras weights-only layout), models/sig2seq.yaml and the RNA model JSON at basecall's default relative paths"""
    import yaml
    from radian_amd import h5weights, weights
    models = cwd / "models"
    models.mkdir(exist_ok=True)
    dil = (1, 2, 4, 8, 16, 32)
    flat = weights.synthetic_weights(seed=seed, dilations=dil)
    h5weights.write_keras_weights(str(models / "sig2seq.h5"), flat, dilations=dil, attr_kind="nullpad")
    tcn = {"nb_filters": 256, "kernel_size": 3, "nb_stacks": 1, "dilations": list(dil), "padding": "causal", "use_skip_connections": False,
           "dropout_rate": 0.0, "return_sequences": True, "activation": "relu", "kernel_initializer": "he_normal", "use_batch_norm": False}
    cfg = {"data": {"n_classes": 5, "window_size": 1024}, "model": {"relu_units": 128, "softmax_units": 5, "timesteps": 1024, "tcn": tcn}}
    (models / "sig2seq.yaml").write_text(yaml.safe_dump(cfg))
    (models / "rnamodel_12mer_pc.json").write_text(json.dumps(_lm_table(k)))


def _read_fasta(d):
    recs = []
    for fn in sorted(os.listdir(d)):
        lines = open(os.path.join(d, fn)).read().split("\n")
        for i in range(0, len(lines) - 1, 2):
            recs.append((lines[i][1:], lines[i + 1]))
    return recs


def test_cli_fastq_against_basecall(golden_dir, tmp_path, monkeypatch, capsys):
    from radian_amd import basecall, fast5, fastq
    ids = json.load(open(os.path.join(golden_dir, "reads_fast5_ids.json")))["read_ids"]
    sig = np.load(os.path.join(golden_dir, "reads_fast5_signals.npz"))
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    fast5.write_multi_fast5(str(in_dir / "reads.fast5"), {r: sig[r] for r in ids})
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    _write_default_artifacts(cwd, 1234, 3)
    monkeypatch.chdir(cwd)
    fa, fq = tmp_path / "fa", tmp_path / "fq"
    fa.mkdir()
    flags = ["--context-len", "3"]
    basecall.main([str(in_dir), str(fa)] + flags)
    capsys.readouterr()
    st = fastq.main([str(in_dir), str(fq), "--moves", str(tmp_path / "moves.tsv"), "--summary", str(tmp_path / "summary.tsv")] + flags)
    out = capsys.readouterr().out
    assert os.listdir(str(fq)) == ["reads.fastq"]
    lines = open(str(fq / "reads.fastq")).read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    recs = [lines[i: i + 4] for i in range(0, len(lines) - 1, 4)]
    assert [(r[0][1:], r[1]) for r in recs] == _read_fasta(str(fa)) and len(recs) == len(ids)
    for r in recs:
        assert r[0][0] == "@" and r[2] == "+" and len(r[3]) == len(r[1])
        assert all("!" <= c <= "S" for c in r[3])
    assert st["reads"] == st["written"] == len(ids) and st["ok"] == len(ids) and st["bases"] == sum(len(r[1]) for r in recs)
    assert f"reads: {len(ids)} seen, {len(ids)} written" in out and "alignment: ok: 5; no-path: 0; too-large: 0" in out
    moves = [ln.split("\t") for ln in open(str(tmp_path / "moves.tsv")).read().splitlines()]
    assert moves[0] == ["read_id", "n_samples", "first_step", "last_step"] and [m[0] for m in moves[1:]] == list(ids)
    for m, r in zip(moves[1:], recs):
        n = int(m[1])
        assert n == len(sig[m[0]])
        first = [int(v) for v in m[2].split(",")] if m[2] else []
        last = [int(v) for v in m[3].split(",")] if m[3] else []
        assert len(first) == len(last) == len(r[1])
        assert all(0 <= f <= l < n for f, l in zip(first, last))
        assert all(a > b for a, b in zip(first, first[1:])) and all(a > b for a, b in zip(last, last[1:]))
    summ = [ln.split("\t") for ln in open(str(tmp_path / "summary.tsv")).read().splitlines()]
    assert summ[0] == ["read_id", "length", "viterbi_score", "mean_q"] and [(s[0], int(s[1])) for s in summ[1:]] == [(r[0][1:], len(r[1])) for r in recs]
    assert all(float(s[2]) < 0 for s in summ[1:])
    # a read over the alignment budget is still written, with '!' qualities, and counted
    fq2 = tmp_path / "fq2"
    st2 = fastq.main([str(in_dir), str(fq2), "--budget-bytes", "4096"] + flags)
    capsys.readouterr()
    lines2 = open(str(fq2 / "reads.fastq")).read().split("\n")
    assert lines2[0::4] == lines[0::4] and lines2[1::4] == lines[1::4]
    assert st2["too-large"] == len(ids) and all(set(q) <= {"!"} for q in lines2[3::4])
    # chunk mode is refused
    with pytest.raises(SystemExit) as ei:
        fastq.main([str(in_dir), str(tmp_path / "fq3"), "--decode-type", "chunk"] + flags)
    assert ei.value.code not in (0, None) and "no single time axis" in str(ei.value.code)
