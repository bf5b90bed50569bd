"""Building the RNA k-mer model on the GPU (rd_lm_build / rd_lm_score; radian_amd.lm_build) against the CPU restatement of its contract
(tests/_lm_ref.py): counts exact, table bit-equal, invariances, the built model as the decoder's model, held-out scores, the command line."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _lm_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def transcripts(k):
    """Markov transcripts (k = 11: ~2e6 bases, so that most of the 4^11 contexts are unseen) with what the contract singles out: runs of N,
    IUPAC letters, records shorter than k + 1, empty records, a record that is one long break"""
    n, length = {1: (4, 200), 3: (6, 400), 5: (8, 600), 7: (10, 2000), 11: (2000, 1000)}[k]
    seqs = ref.markov_transcripts(40 + k, n, length)
    s = seqs[1]
    seqs[1] = s[:50] + "NNNNN" + s[55:120] + "n" + s[121:150] + "RYK" + s[153:]
    seqs[2] = "N" + seqs[2][1:-1] + "N"
    seqs += ["", "ACGT"[: min(k, 4)], "A" * k, "", "N" * (k + 3), "ACGTTGCA" * 4, "acgu" * 5]
    return seqs


def check_build(be, codes, off, k, unseen, alpha, as_written, cut=0):
    table, st = be.build_lm(codes, off, k, as_written=as_written, unseen=unseen, pseudocount=alpha, cut=cut, want_counts=True)
    C = ref.counts(codes, off, k, as_written)
    assert np.array_equal(st["counts"].astype(np.int64), C), (k, unseen, alpha, as_written)
    exp, order = ref.table(C, k, unseen, alpha)
    nan_e, nan_g = np.isnan(exp[:, 0]), np.isnan(table[:, 0])
    assert np.array_equal(nan_e, nan_g) and np.array_equal(np.isnan(table), np.isnan(exp))
    bad = table.view(np.uint64)[~nan_e] != exp.view(np.uint64)[~nan_e]
    assert not bad.any(), (k, unseen, alpha, int(bad.sum()), table[~nan_e][bad.any(1)][:3], exp[~nan_e][bad.any(1)][:3])
    assert st["windows"] == int(C.sum()) and st["contexts_seen"] == int((C.sum(1) > 0).sum()) and st["contexts"] == 4 ** k
    per = {int(j): int(n) for j, n in zip(*np.unique(order[order >= 0], return_counts=True))}
    assert st["rows_per_order"] == per
    left = int((order < 0).sum())
    assert st["absent_rows"] == (left if unseen == "absent" else 0) and st["uniform_rows"] == (left if unseen == "uniform" else 0)
    assert be.lm_k == k
    return table, st, order


@pytest.mark.parametrize("k", [1, 3, 5, 7, 11])
def test_counts_and_table_equal_the_restatement(be, k):
    codes, off = ref.encode(transcripts(k))
    assert (codes == 255).sum() > 10 and (np.diff(off) == 0).sum() >= 2 and ((np.diff(off) > 0) & (np.diff(off) < k + 1)).sum() >= 1
    combos = [(u, a, w) for u in ("backoff", "uniform", "absent") for a in (0.0, 0.5) for w in (False, True)]
    if k == 11:
        combos = [("backoff", 0.0, False), ("backoff", 0.5, True), ("uniform", 0.0, True), ("absent", 0.5, False)]
    for unseen, alpha, aw in combos:
        table, st, order = check_build(be, codes, off, k, unseen, alpha, aw)
        print(f"k={k} {unseen} alpha={alpha} as_written={aw}: {st['windows']} windows, {st['contexts_seen']} of {4 ** k} contexts, rows {st['rows_per_order']}")
        if unseen == "backoff":
            assert not np.isnan(table).any()
            if k == 11:   # most contexts unseen, a chain of back-off orders in use
                assert st["contexts_seen"] < 4 ** k // 2 and len(st["rows_per_order"]) >= 5


@pytest.mark.parametrize("k", [3, 5])
def test_back_off_reaches_order_zero(be, k):
    """a transcriptome of two letters: contexts ending in G or T have no counted suffix at all and take the order-0 row"""
    codes, off = ref.encode(["AAAAAAAACCCCCCCCAAAACCCC", "CCCCCCCCCCCCA"])
    for alpha in (0.0, 0.5):
        table, st, order = check_build(be, codes, off, k, "backoff", alpha, False)
        assert set(st["rows_per_order"]) >= {0, 1, k}
        assert order[4 ** k - 1] == 0 and table[4 ** k - 1, 2] == (alpha / (st["windows"] + 4 * alpha))


def test_result_depends_on_neither_record_order_nor_launch_cut_nor_run(be):
    k = 7
    seqs = transcripts(k)
    codes, off = ref.encode(seqs)
    base, st0 = be.build_lm(codes, off, k, pseudocount=0.5, want_counts=True)
    again, st1 = be.build_lm(codes, off, k, pseudocount=0.5, want_counts=True)
    assert again.tobytes() == base.tobytes() and st0["counts"].tobytes() == st1["counts"].tobytes()
    assert st0["launches"] == 1
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(seqs))
    c2, o2 = ref.encode([seqs[i] for i in perm])
    shuffled, st2 = be.build_lm(c2, o2, k, pseudocount=0.5, want_counts=True)
    assert shuffled.tobytes() == base.tobytes() and st2["counts"].tobytes() == st0["counts"].tobytes()
    for cut in (1, 5, 8, 997, 4096, len(codes) + len(seqs) - 1):
        if cut == 1:   # (one byte per launch: on a slice, to keep it short)
            c3, o3 = ref.encode(seqs[1:2] + seqs[-7:])
            whole, _ = be.build_lm(c3, o3, k, want_counts=False)
            pieces, st3 = be.build_lm(c3, o3, k, cut=1)
            assert pieces.tobytes() == whole.tobytes() and st3["launches"] == len(c3) + len(o3) - 1
            continue
        cutted, st3 = be.build_lm(codes, off, k, pseudocount=0.5, cut=cut, want_counts=True)
        assert st3["launches"] == -(-(len(codes) + len(seqs)) // cut) and st3["launches"] > 1
        assert cutted.tobytes() == base.tobytes() and st3["counts"].tobytes() == st0["counts"].tobytes(), cut
        for key in ("windows", "contexts_seen", "gate_contexts", "gate_windows", "rows_per_order"):
            assert st3[key] == st0[key]


def soft_rows(seed, T):
    rng = np.random.default_rng(seed)
    return rng.dirichlet([1.0] * 5, size=T).astype(np.float32)


@pytest.mark.parametrize("k,unseen,W", [(3, "backoff", 6), (5, "backoff", 6), (5, "uniform", 12), (7, "backoff", 25), (3, "absent", 6)])
def test_the_built_model_is_the_loaded_model(be, oracle, tmp_path, k, unseen, W):
    """after build_lm the context decodes as (i) a context given load_lm(table_out), (ii) one given the written file read back, (iii) the
    oracle's beam search with that table: same labelings, bit-equal scores; an absent context ends the read in all of them"""
    from radian_amd import Backend, lm
    seqs = ref.markov_transcripts(70 + k, 8, 600) if unseen != "absent" else ["ACGTACGGTTAACC" * 3]
    codes, off = ref.encode(seqs)
    s_thr, r_thr = 0.1, 1.0
    mats = [soft_rows(10 * k + i, T) for i, T in enumerate((60, 90, 75))]
    rows = np.concatenate(mats)
    lens = np.array([len(m) for m in mats], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    table, st = be.build_lm(codes, off, k, unseen=unseen, r_threshold=r_thr)
    assert st["gate_contexts"] > 0, "the thresholds must open the gate somewhere"
    got, sc = be.decode_batch(rows, offs, lens, W, use_lm=True, s_threshold=s_thr, r_threshold=r_thr, with_scores=True)
    path = str(tmp_path / "m.json")
    lm.write_json(path, table, k)
    t_file, k_file = lm.load_json(path)
    assert k_file == k and np.array_equal(np.isnan(t_file), np.isnan(table)) and np.array_equal(t_file[~np.isnan(t_file)], table[~np.isnan(table)])
    for name, tab in (("load_lm(table_out)", table), ("load_json(write_json)", t_file)):
        with Backend(0) as other:
            other.load_lm(tab, k)
            g2, s2 = other.decode_batch(rows, offs, lens, W, use_lm=True, s_threshold=s_thr, r_threshold=r_thr, with_scores=True)
        for a, b in zip(got, g2):
            assert (a is None and b is None) or np.array_equal(a, b), name
        live = [i for i, a in enumerate(got) if a is not None]
        assert np.array_equal(sc[live].view(np.uint64), s2[live].view(np.uint64)), name
    n_absent = 0
    for i, m in enumerate(mats):
        try:
            exp, final = oracle.beam_search_labels(m, W, table, s_thr, r_thr, k, max_final=1)
        except KeyError:
            assert got[i] is None
            n_absent += 1
            continue
        assert got[i] is not None and np.array_equal(got[i], exp), (k, unseen, i)
        assert len(exp) > k + 1
        assert sc[i] == final[0][1], (float(sc[i]).hex(), float(final[0][1]).hex())
    assert (n_absent > 0) == (unseen == "absent")
    # ... and with the model off the labelings differ somewhere: the model was consulted
    plain = be.decode_batch(rows, offs, lens, W)
    if unseen != "absent":
        assert any(not np.array_equal(a, b) for a, b in zip(got, plain))


@pytest.mark.parametrize("k,unseen", [(5, "backoff"), (5, "absent"), (7, "uniform")])
def test_held_out_score_equals_the_restatement(be, k, unseen):
    train = ref.markov_transcripts(90 + k, 8, 600)
    held = ref.markov_transcripts(90 + k, 12, 500)[8:] + ["ACGTNNNNACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTAGCTAGC", "", "AC"]
    codes, off = ref.encode(train)
    hc, ho = ref.encode(held)
    table, st = be.build_lm(codes, off, k, unseen=unseen)
    for r_thr, aw, cut in ((0.5, False, 0), (1.0, True, 0), (0.5, False, 333)):
        got = be.score_lm(hc, ho, as_written=aw, r_threshold=r_thr, cut=cut)
        exp = ref.score(table, k, hc, ho, r_thr, aw)
        print(f"k={k} {unseen} r={r_thr} as_written={aw} cut={cut}: {got} / restatement {exp['mean_nll']!r}")
        for key in ("windows", "scored", "zero", "absent", "gate_windows"):
            assert got[key] == exp[key], key
        n = exp["scored"]
        assert n > 100
        assert abs(got["mean_nll"] - exp["mean_nll"]) <= (n + 1) * 2.0 ** -52 * abs(exp["mean_nll"])
        if unseen == "absent":
            assert got["absent"] > 0
        assert got == be.score_lm(hc, ho, as_written=aw, r_threshold=r_thr, cut=cut)            # two runs: the same bits
    # the build's own gate statistics, from the restatement's entropies
    ent = ref.entropy(table)
    C = ref.counts(codes, off, k)
    _, st = be.build_lm(codes, off, k, unseen=unseen, r_threshold=0.5)
    assert st["gate_contexts"] == int((ent < 0.5).sum()) and st["gate_windows"] == int(C.sum(1)[ent < 0.5].sum())
    # a loaded model scores like the built one
    be.load_lm(table, k)
    assert be.score_lm(hc, ho) == got_default(be, table, k, hc, ho, codes, off, unseen)


def got_default(be, table, k, hc, ho, codes, off, unseen):
    be.build_lm(codes, off, k, unseen=unseen)
    return be.score_lm(hc, ho)


def _golden_fast5(tmp_path, golden_dir):
    from radian_amd import fast5
    ids = json.load(open(os.path.join(golden_dir, "reads_fast5_ids.json")))["read_ids"]
    sig = np.load(os.path.join(golden_dir, "reads_fast5_signals.npz"))
    in_dir = tmp_path / "fast5"
    in_dir.mkdir()
    fast5.write_multi_fast5(str(in_dir / "reads.fast5"), {r: sig[r] for r in ids})
    return str(in_dir)


def _fasta_out(d):
    return {fn: open(os.path.join(d, fn)).read() for fn in sorted(os.listdir(d))}


def test_command_line_end_to_end(be, tmp_path, golden_dir, capsys):
    """lm_build on a FASTA file, then basecall --rna-model with what it wrote, equals the run with the table built in-process"""
    import gzip
    from radian_amd import lm_build, basecall, lm
    k = 3
    seqs = ref.markov_transcripts(5, 12, 500)
    heads = [f"T{i}|G{i}|-|-|N-{i}|N|500|{'protein_coding' if i % 3 else 'lncRNA'}|" for i in range(len(seqs))]
    text = "".join(f">{h}\n" + "\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + "\n" for h, s in zip(heads, seqs))
    fa = tmp_path / "tx.fa.gz"
    fa.write_bytes(gzip.compress(text.encode()))
    held = tmp_path / "held.fa"
    held.write_text(">h|a|b|c|d|e|f|protein_coding|\n" + ref.markov_transcripts(5, 13, 400)[12] + "\n")
    model = str(tmp_path / "rnamodel.json")
    st = lm_build.main([str(fa), "-o", model, "--context-len", str(k), "--protein-coding", "--heldout", str(held)])
    out = capsys.readouterr().out
    kept = [s for i, s in enumerate(seqs) if i % 3]
    codes, off = ref.encode(kept)
    assert f"records: 12 read, {len(kept)} kept; bases: {len(codes)}; windows of {k + 1} labels counted: {st['windows']}" in out
    assert "gate open (entropy < 0.5):" in out and "held-out" in out and "mean -ln p" in out and f"wrote {model}: 64 contexts" in out
    table, _ = be.build_lm(codes, off, k)
    t_cli, k_cli = lm.load_json(model)
    assert k_cli == k and t_cli.tobytes() == table.tobytes()
    assert t_cli.tobytes() == lm.table_from_dict(json.load(open(model)))[0].tobytes()
    # --score alone on the written model gives the held-out figures of the build
    sc = lm_build.main(["--score", model, "--heldout", str(held)])
    hc, ho, _ = lm.read_fasta(str(held))
    assert {key: sc[key] for key in ("windows", "scored", "mean_nll")} == {key: be.score_lm(hc, ho)[key] for key in ("windows", "scored", "mean_nll")}
    capsys.readouterr()
    # the decoder takes the file
    own = str(tmp_path / "own.json")
    with open(own, "w") as f:
        json.dump({"".join("ACGT"[(c >> (2 * (k - 1 - j))) & 3] for j in range(k)): [float(x) for x in table[c]] for c in range(4 ** k)}, f)
    in_dir = _golden_fast5(tmp_path, golden_dir)
    outs = []
    for name, path in (("cli", model), ("own", own)):
        d = tmp_path / ("out_" + name)
        d.mkdir()
        basecall.main([in_dir, str(d), "--sig-model", "synthetic:1234", "--sig-config", "none", "--rna-model", path, "--context-len", str(k),
                       "--step-size", "512"])
        outs.append(_fasta_out(str(d)))
    assert outs[0] == outs[1] and sum(len(v) for v in outs[0].values()) > 100


def test_refusals(be):
    from radian_amd import RadianHipError, _lib
    codes, off = ref.encode(["ACGTACGTACGT"])
    for k in (0, 14, -1):
        with pytest.raises(RadianHipError, match="out of range"):
            be.build_lm(codes, off, k)
    for seqs in ([], [""], ["ACG", "NNNNNNNNNN", "ACNGT"], ["ACGT"]):
        c, o = ref.encode(seqs)
        with pytest.raises(RadianHipError, match="no window"):
            be.build_lm(c, o, 4 if seqs == ["ACGT"] else 3)
    with pytest.raises(RadianHipError, match="pseudocount"):
        be.build_lm(codes, off, 3, pseudocount=-1.0)
    with pytest.raises(ValueError):
        be.build_lm(codes, off, 3, unseen="other")
    with pytest.raises(ValueError):
        be.build_lm(codes, off[:1], 3)
    # 32-bit counters: a request that could hold more than 2^32 - 1 windows is refused by its arithmetic, before any base is read
    L = _lib.load()
    big = np.array([0, 2 ** 32], dtype=np.int64)
    st = np.zeros(32, dtype=np.int64)
    rc = L.rd_lm_build(be._h, codes.ctypes.data_as(ctypes.c_void_p), big.ctypes.data_as(ctypes.c_void_p), 1, 3, 0, 0, 0.0, 0.5, 0, None, None,
                       st.ctypes.data_as(ctypes.c_void_p))
    assert rc == -1 and "4294967296" in L.rd_last_error().decode() and "32-bit" in L.rd_last_error().decode()
    big[1] = 2 ** 32 - 1   # (the largest accepted size is not tried: it would read 4 G codes)
    # a failed build leaves no half-made model behind for the decoder, and the context still works
    be.load_lm(None, 0)
    with pytest.raises(RadianHipError):
        be.score_lm(codes, off)
    table, st = be.build_lm(codes, off, 3)
    assert st["windows"] == 9 and be.score_lm(codes, off)["windows"] == 9
    be.load_lm_hashed(np.full((64, 4), 0.25), 3, 20)
    with pytest.raises(RadianHipError, match="hashed"):
        be.score_lm(codes, off)
    be.load_lm(None, 0)
