"""GPU checks of training-shard building: rd_fit_batch (fit.hip) against the restatement of its contract (tests/_fit_ref.py) on every
output field (under the default scores and under every score set of tests/_align_ref.py, the int32 bound and the refusal of
gap_open > gap_extend among them), and python -m radian_amd.label_build end to end -- the windows, spans and labels the restatement plus the selection
rules give, shards that read back exactly, bytes that do not depend on the batch size, and `evaluate` / `train` running on the result."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _fit_cases as fc
import _fit_ref as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T0 = time.perf_counter()


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


def _mutate(rng, seq, rate):
    """substitutions, deletions and insertions at `rate` in all, a third each"""
    out = []
    for c in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(int(rng.integers(0, 4)) if r < 2 * rate / 3 else int(c))
        if rng.random() < rate / 3:
            out.append(int(rng.integers(0, 4)))
    return np.array(out if out else [int(rng.integers(0, 4))], dtype=np.uint8)


def _fit_cases():
    """(refs, queries, query_ref): every case the contract's check lists"""
    rng = np.random.default_rng(20)
    refs, queries, qref = [], [], []

    def add_ref(r):
        refs.append(np.asarray(r, dtype=np.uint8))
        return len(refs) - 1

    def add(r, q):
        q = np.asarray(q, dtype=np.uint8)
        assert 1 <= len(q) <= 1024 and q.max() <= 3
        queries.append(q)
        qref.append(r)

    def sub(r, m, rate):
        ref = refs[r]
        ref = np.where(ref == 4, rng.integers(0, 4, size=len(ref)), ref)
        lo = int(rng.integers(0, max(1, len(ref) - m + 1)))
        q = _mutate(rng, ref[lo: lo + m], rate)[:1024]
        return q

    # mutated substrings at 0-15 % against a 1.5 kb reference, every query length of the list: many queries per reference
    r0 = add_ref(rng.integers(0, 4, size=1500))
    for m in (1, 2, 63, 64, 65, 255, 256, 1024, 8, 30, 31, 32, 33, 100, 127, 128, 129, 500, 513):
        for rate in (0.0, 0.03, 0.08, 0.15):
            add(r0, sub(r0, m, rate))
    for m in (1, 2, 63, 64, 65, 255, 256, 1024):   # exact lengths (the mutations above move them)
        lo = int(rng.integers(0, 1500 - m + 1))
        add(r0, refs[r0][lo: lo + m])
        add(r0, rng.integers(0, 4, size=m))        # unrelated
    for _ in range(20):
        add(r0, rng.integers(0, 4, size=int(rng.integers(1, 80))))
    # 20 000 codes
    r1 = add_ref(rng.integers(0, 4, size=20000))
    for m, rate in ((30, 0.05), (64, 0.1), (256, 0.12), (17, 0.0)):
        add(r1, sub(r1, m, rate))
    add(r1, rng.integers(0, 4, size=40))
    # short references, n < m included
    for n in (0, 1, 63, 64, 65):
        r = add_ref(rng.integers(0, 4, size=n))
        for m in (1, 2, 5, 63, 64, 65, 100, 255):
            add(r, rng.integers(0, 4, size=m))
            if n >= 8:
                add(r, sub(r, min(m, n), 0.1))
    # many ties: homopolymers and dinucleotide repeats
    rh = add_ref(np.zeros(300, dtype=np.uint8))
    for m in (1, 2, 10, 64, 65, 200, 300, 320):
        add(rh, np.zeros(m, dtype=np.uint8))
    add(rh, [0] * 10 + [1] + [0] * 10)
    add(rh, [1] * 12)
    rd = add_ref(np.tile([0, 1], 200))
    for k in (1, 5, 32, 33, 100, 128):
        add(rd, np.tile([0, 1], k))
        add(rd, np.tile([1, 0], k))
        add(rd, np.tile([0, 1], k)[:-1])
    add(rd, list(np.tile([0, 1], 20)) + [0] + list(np.tile([0, 1], 20)))
    add(rd, list(np.tile([0, 1], 20)) + [2, 2] + list(np.tile([0, 1], 20)))
    rt = add_ref(np.tile([0, 0, 1], 100))
    add(rt, np.tile([0, 1], 30))
    add(rt, np.tile([0, 0, 1], 21)[1:])
    # references with code 4
    r4 = rng.integers(0, 4, size=800)
    r4[rng.random(800) < 0.05] = 4
    r4 = add_ref(r4)
    for m in (10, 30, 64, 200):
        for rate in (0.0, 0.1):
            add(r4, sub(r4, m, rate))
    add(add_ref(np.full(50, 4)), rng.integers(0, 4, size=20))
    return refs, queries, np.array(qref, dtype=np.int32)


@pytest.fixture(scope="module")
def fit_cases():
    refs, queries, qref = _fit_cases()
    want = [fr.fit_rows(refs[r], q) for q, r in zip(queries, qref)]
    return refs, queries, qref, want


def _check(res, want, idx=None):
    from radian_amd.backend import FIT_OK
    idx = range(len(want)) if idx is None else idx
    for p in idx:
        w = want[p]
        got = {"score": int(res.score[p]), "ref_start": int(res.ref_start[p]), "ref_end": int(res.ref_end[p]),
               "counts": tuple(int(c) for c in res.counts[p])}
        assert res.status[p] == FIT_OK and got == w, (p, got, w)


def test_fit_batch_equals_the_restatement_on_every_field(be, fit_cases):
    refs, queries, qref, want = fit_cases
    ms, ns = {len(q) for q in queries}, {len(r) for r in refs}
    assert {1, 2, 63, 64, 65, 255, 256, 1024} <= ms and {0, 1, 63, 64, 65, 1500, 20000} <= ns
    assert any(len(q) > len(refs[r]) for q, r in zip(queries, qref))
    res = be.fit_batch(refs, queries, qref)
    _check(res, want)
    # a second call (workspace reuse) and a permutation of the queries give the same
    perm = np.random.default_rng(2).permutation(len(queries))
    res2 = be.fit_batch(refs, [queries[p] for p in perm], qref[perm])
    _check(res2, [want[p] for p in perm])


def test_fit_batch_under_a_small_budget_equals_one_batch(be, fit_cases):
    refs, queries, qref, want = fit_cases
    budget = 22000   # the 20 000-code reference and its longest query fit (21 344 bytes); the sequences alone are more than twice that
    assert sum(len(r) for r in refs) + sum(len(q) for q in queries) > 2 * budget
    res = be.fit_batch(refs, queries, qref, budget_bytes=budget)
    _check(res, want)


def test_fit_batch_too_large_leaves_the_others_aligned(be, fit_cases):
    from radian_amd.backend import FIT_EMPTY, FIT_TOO_LARGE, RadianHipError
    refs, queries, qref, want = fit_cases
    big = [p for p in range(len(queries)) if len(refs[qref[p]]) == 20000][:1]
    small = [p for p in range(len(queries)) if len(refs[qref[p]]) <= 1500][:40]
    idx = small[:20] + big + small[20:]
    qs, qr = [queries[p] for p in idx], qref[idx]
    with pytest.raises(RadianHipError, match="RD_FIT_TOO_LARGE"):
        be.fit_batch(refs, qs, qr, budget_bytes=16000)
    res = be.fit_batch(refs, qs, qr, budget_bytes=16000, allow_too_large=True)
    assert list(np.flatnonzero(res.status == FIT_TOO_LARGE)) == [20]
    assert res.score[20] == 0 and not res.counts[20].any()
    _check(res, [want[p] for p in idx], [k for k in range(len(idx)) if k != 20])
    # an empty query is reported, not fitted; bad input is refused before anything runs
    res = be.fit_batch(refs[:1], [queries[0], np.zeros(0, np.uint8), queries[1]], [0, 0, 0])
    assert list(res.status) == [0, FIT_EMPTY, 0] and res.score[1] == 0
    _check(res, [want[0], None, want[1]], [0, 2])
    for bad_refs, bad_q, bad_r in (([[0, 1, 5]], [[0]], [0]), ([[0, 1]], [[4]], [0]), ([[0, 1]], [[0] * 1025], [0]), ([[0, 1]], [[0]], [1])):
        with pytest.raises(RadianHipError):
            be.fit_batch(bad_refs, bad_q, bad_r)
    assert len(be.fit_batch([], [], []).score) == 0


# ---------------------------------------------------------------- scores other than 2 / -4 / -4 / -2
_SET_ID = lambda sc: "_".join(str(v) for v in sc)


@pytest.fixture(scope="module")
def small_cases():
    refs, queries, qref = fc.fit_cases_small()
    ms = sorted({len(q) for q in queries})
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 128), (129, 256), (257, 512), (513, 1024)):   # fit.hip's launch classes
        assert any(lo <= m <= hi for m in ms), (lo, hi)
    assert any(len(q) > len(refs[r]) for q, r in zip(queries, qref))
    return refs, queries, qref


@pytest.mark.parametrize("sc", fr.SMALL_SETS, ids=_SET_ID)
def test_fit_batch_under_every_score_set(be, small_cases, sc):
    """Linear gaps (every `ee >= eo` / `fe >= fo` select of fit_kernel decided on a tie), a zero match score, a zero and a positive
    mismatch score, free extension, an expensive opening: every field equals the row-wise restatement's; the same after a permutation
    and under a budget that cuts the queries into several launches"""
    refs, queries, qref = small_cases
    want = [fr.fit_rows(refs[r], q, sc) for q, r in zip(queries, qref)]
    _check(be.fit_batch(refs, queries, qref, scores=sc), want)
    perm = np.random.default_rng(2).permutation(len(queries))
    _check(be.fit_batch(refs, [queries[p] for p in perm], qref[perm], scores=sc), [want[p] for p in perm])
    budget = 4096   # the 1500-code reference and a 1024-label query fit (1500 + 1024 + 64 + 1024 bytes)
    assert sum(len(r) for r in refs) + sum(len(q) for q in queries) > 2 * budget
    _check(be.fit_batch(refs, queries, qref, scores=sc, budget_bytes=budget), want)
    # the set's results hold gaps of both kinds, so both selects ran on a path that counts
    assert any(w["counts"][2] >= 2 for w in want) and any(w["counts"][3] >= 2 for w in want), sc


def _raw_fit(be, refs, queries, qref, sc, fill=-7):
    """rd_fit_batch on pre-filled outputs: (rc, error text, whether every output still holds the fill)"""
    from radian_amd.backend import _concat_codes, _p
    rbuf, roff = _concat_codes(refs)
    qbuf, qoff = _concat_codes(queries)
    n = len(queries)
    qr = np.ascontiguousarray(qref, dtype=np.int32)
    score, start, end, status = (np.full(n, fill, dtype=np.int32) for _ in range(4))
    counts = np.full((n, 4), fill, dtype=np.int32)
    rc = be._L.rd_fit_batch(be._h, _p(rbuf), _p(roff), len(roff) - 1, _p(qbuf), _p(qoff), _p(qr), n, *(int(v) for v in sc), 0, _p(score),
                            _p(start), _p(end), _p(counts), _p(status))
    return rc, be._L.rd_last_error().decode(), all((x == fill).all() for x in (score, start, end, status, counts))


def test_fit_batch_at_the_int32_bound(be, small_cases):
    """|score| = 65535: a reference of 3071 codes is the longest the argument check admits (65535 * (3071 + 1025) < 2^28); queries of 1, 64
    and 1024 against it and some of the small cases are exact against the restatement, whose stored -inf lies below every reachable value
    at these scores (tests/test_label_build_cpu.py).  3072 codes are refused before any output is written."""
    rng = np.random.default_rng(22)
    assert 65535 * (3071 + 1025) < 1 << 28 <= 65535 * (3072 + 1025)
    big = rng.integers(0, 4, size=3072).astype(np.uint8)
    big[rng.integers(0, 3071, size=20)] = 4
    qs = [_mutate(rng, np.where(big[lo: lo + m + 40] == 4, 0, big[lo: lo + m + 40]), 0.1)[:m] for lo, m in ((100, 1), (2000, 64), (1500, 1024))]
    assert [len(q) for q in qs] == [1, 64, 1024]
    qs.append(rng.integers(0, 4, size=1024).astype(np.uint8))                        # unrelated: the most negative scores
    refs, queries, qref = small_cases
    few = [p for p in range(len(queries)) if len(refs[qref[p]]) <= 300][:30]
    all_refs = list(refs) + [big[:3071]]
    all_q, all_r = [queries[p] for p in few] + qs, np.array([qref[p] for p in few] + [len(refs)] * len(qs), dtype=np.int32)
    for sc in fr.BOUND_SETS:
        want = [fr.fit_rows(all_refs[r], q, sc) for q, r in zip(all_q, all_r)]
        _check(be.fit_batch(all_refs, all_q, all_r, scores=sc), want)
        rc, msg, untouched = _raw_fit(be, list(refs) + [big], all_q, all_r, sc)
        assert rc == -1 and untouched and f"reference {len(refs)} (3072 codes)" in msg and "too long for int32 scores" in msg, (sc, rc, msg)


def test_fit_batch_refuses_gap_open_above_gap_extend_before_any_output(be, small_cases):
    """with open > extend the recurrence reopens adjacent gaps: its score is not the stated gap cost (tests/test_label_build_cpu.py)"""
    from radian_amd import RadianHipError
    refs, queries, qref = small_cases
    for sc in (fr.REFUSED_SET, (2, -4, -2, -4)):
        rc, msg, untouched = _raw_fit(be, refs, queries[:20], qref[:20], sc)
        assert rc == -1 and untouched and msg.startswith("rd_fit_batch: gap_open") and "gap_open <= gap_extend" in msg, (sc, rc, msg)
        with pytest.raises(RadianHipError, match="gap_open <= gap_extend"):
            be.fit_batch(refs, queries[:20], qref[:20], scores=sc)
    sc = (2, -4, -3, -3)                                                             # equality, linear gaps, is legal
    rc, msg, untouched = _raw_fit(be, refs, queries[:20], qref[:20], sc)
    assert rc == 0 and not untouched, (rc, msg)
    _check(be.fit_batch(refs, queries[:20], qref[:20], scores=sc), [fr.fit_rows(refs[r], q, sc) for q, r in zip(queries[:20], qref[:20])])


# ---------------------------------------------------------------- python -m radian_amd.label_build, end to end
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
CLIP, BEAM = 4, 6


def _run(args, cwd=ROOT):
    p = subprocess.run([sys.executable, "-m", *args], cwd=cwd, capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": ROOT})
    assert p.returncode == 0, p.stderr
    return p.stdout


def _is_val(rid, fraction):
    import _tfrecord_writer as tw
    return tw.crc32c(rid.encode()) % 10000 < fraction * 10000


def _job(tmp_path, be, seed, n_reads, without_reference=(), duplicate=False):
    """seeded int16 reads in two fast5 files, the model as an .rdnw, and a TSV whose references are built from the reads' own calls at
    step 1024: joined, 2 % mutated, 50 random bases on either side (duplicate: a copy of the third window's call put in front, so
    that this call fits twice), written 5'->3' (reversed).  Returns (ids, raws, {id: ref in decode order}, paths)."""
    from radian_amd import fast5, weights
    rng = np.random.default_rng(seed)
    w = weights.synthetic_weights(seed=seed, head_gain=3)
    be.load_weights(w)
    model = str(tmp_path / "model.rdnw")
    with open(model, "wb") as f:
        f.write(weights.pack_blob(w))
    ids = [f"read-{k:03d}" for k in range(n_reads)]
    raws = [np.round(rng.normal(500.0, 80.0, size=int(rng.integers(3500, 9000)))).astype(np.int16) for _ in ids]
    calls, status = be.basecall_raw_chunk(raws, CLIP, 1024, 1024, BEAM)
    assert not status.any()
    refs = {}
    for rid, c in zip(ids, calls):
        if rid in without_reference:
            continue
        body = _mutate(rng, np.concatenate(c), 0.02)
        front = [rng.integers(0, 4, size=50).astype(np.uint8)]
        if duplicate:
            front.append(np.asarray(c[2], dtype=np.uint8))
        refs[rid] = np.concatenate(front + [body, rng.integers(0, 4, size=50).astype(np.uint8)]).astype(np.uint8)
    d = tmp_path / "fast5"
    os.makedirs(d / "sub", exist_ok=True)
    half = n_reads // 2
    fast5.write_multi_fast5(str(d / "a.fast5"), {r: s for r, s in zip(ids[:half], raws[:half])})
    fast5.write_multi_fast5(str(d / "sub" / "b.fast5"), {r: s for r, s in zip(ids[half:], raws[half:])})
    tsv = str(tmp_path / "read_ref.tsv")
    with open(tsv, "w") as f:
        f.write("read\ttxt\tseq\n")
        for k, (rid, dec) in enumerate(refs.items()):
            s = LETTERS[dec[::-1]].tobytes().decode()
            f.write(f"{rid}\ttx{k}\t{s.replace('T', 'U') if k % 3 == 0 else s.lower() if k % 3 == 1 else s}\n")
    return ids, raws, refs, str(d), tsv, model


def _expected(be, ids, raws, refs, step, val_fraction):
    """what the restatement gives: {(read, window): (status, fit)} and per split the kept (signal, signal_length, label) in input order"""
    from radian_amd.preprocess import get_windows
    calls, status = be.basecall_raw_chunk(raws, CLIP, 1024, step, BEAM)
    norm, _ = be.normalise_reads(raws, CLIP)
    rows, kept = {}, {"train": [], "val": []}
    for rid, c, x in zip(ids, calls, norm):
        if rid not in refs:
            continue
        windows, pad_end = get_windows(x, 1024, step)
        assert len(windows) == len(c) and windows.dtype == np.float32
        sig_len = [1024] * (len(windows) - 1) + [1024 - pad_end]
        for w, (st, f) in enumerate(fr.select(c, sig_len, refs[rid])):
            rows[(rid, w)] = (st, f)
            if st == "kept":
                kept["val" if _is_val(rid, val_fraction) else "train"].append((windows[w], sig_len[w], refs[rid][f["ref_start"]:f["ref_end"]]))
    return rows, kept


def _read_manifest(path):
    rows = {}
    with open(path) as f:
        assert f.readline().split("\t")[:3] == ["read_id", "window", "status"]
        for line in f:
            c = line.rstrip("\n").split("\t")
            rows[(c[0], int(c[1]))] = (c[2], tuple(int(v) for v in c[3:]))
    return rows


def _compare(out_dir, manifest, rows, kept, per_shard):
    from radian_amd.tfrecord import read_shard
    got = _read_manifest(manifest)
    with_ref = {k: v for k, v in got.items() if v[0] != "no-reference"}
    assert set(with_ref) == set(rows)
    for key, (st, f) in rows.items():
        want = (f["ref_start"], f["ref_end"], f["score"], *f["counts"]) if f is not None else (0,) * 7
        assert got[key] == (st, want), (key, got[key], st, want)
    for split, want in kept.items():
        files = sorted(os.listdir(os.path.join(out_dir, split))) if os.path.isdir(os.path.join(out_dir, split)) else []
        assert files == [f"shard-{k:05d}.tfrecords" for k in range(-(-len(want) // per_shard))]
        at = 0
        for k, name in enumerate(files):
            sh = read_shard(os.path.join(out_dir, split, name))
            assert len(sh) == min(per_shard, len(want) - k * per_shard)
            for i in range(len(sh)):
                sig, sl, lab = want[at]
                assert sh.signals[i].tobytes() == np.ascontiguousarray(sig, dtype=np.float32).tobytes(), (split, at)
                assert sh.input_len[i] == sl and np.array_equal(sh.label(i), lab), (split, at)
                at += 1
        assert at == len(want)


def _files(out_dir):
    return {os.path.join(s, n): open(os.path.join(out_dir, s, n), "rb").read() for s in ("train", "val") for n in sorted(os.listdir(os.path.join(out_dir, s)))}


def test_label_build_end_to_end(be, tmp_path, capsys):
    from radian_amd import label_build
    ids, raws, refs, fast5_dir, tsv, model = _job(tmp_path, be, seed=31, n_reads=8, without_reference=("read-005",))
    val_fraction, per_shard = 0.4, 7
    rows, kept = _expected(be, ids, raws, refs, 1024, val_fraction)
    common = [fast5_dir, tsv, "--sig-model", model, "--sig-config", "none", "--step-size", "1024", "--val-fraction", str(val_fraction),
              "--windows-per-shard", str(per_shard)]
    out1, man1 = str(tmp_path / "shards1"), str(tmp_path / "windows1.tsv")
    st = label_build.main(common + ["-o", out1, "--manifest", man1, "--batch-reads", "3"])
    text = capsys.readouterr().out
    with capsys.disabled():
        print("\n" + text + f"[label_build e2e] labels per call: median {np.median([sum(f['counts'][:3]) for _, f in rows.values() if f]):.0f}")
    assert st["reads"] == 8 and st["reads_used"] == 7 and st["reads_no_reference"] == 1
    assert "reads: 8 seen, 7 used; no reference: 1" in text and "label length median:" in text
    # every read with a reference emits windows
    for rid in refs:
        assert any(k[0] == rid and v[0] == "kept" for k, v in rows.items()), rid
    assert kept["train"] and kept["val"]
    _compare(out1, man1, rows, kept, per_shard)
    got = _read_manifest(man1)
    assert {v[0] for k, v in got.items() if k[0] == "read-005"} == {"no-reference"}
    assert st["kept"] == len(kept["train"]) + len(kept["val"]) == sum(v[0] == "kept" for v in got.values())
    # another internal batch size, another process: byte-identical files (and a rerun over an existing directory)
    out2 = str(tmp_path / "shards2")
    for _ in range(2):
        _run(["radian_amd.label_build", *common, "-o", out2, "--batch-reads", "512", "--budget-bytes", "20000"])
        assert _files(out2) == _files(out1)
    # the shards feed evaluate and train
    ev = _run(["radian_amd.evaluate", out1, "--sig-config", "none", "--sig-model", model])
    lines = dict(l.split("\t", 1) for l in ev.splitlines() if "\t" in l)
    assert np.isfinite(float(lines["val_loss"])) and lines["infeasible_windows"] == "0" and lines["windows"] == str(len(kept["val"]))
    tr = _run(["radian_amd.train", "-s", out1, "-g", "none", "--sig-model", model, "--epochs", "1", "--steps-per-epoch", "2", "--batch-size", "4",
               "--out-dir", str(tmp_path / "run")])
    assert [l.split()[1] for l in tr.splitlines() if l.startswith("epoch ")] == ["1/1"] and os.path.exists(tmp_path / "run" / "model-01.rdnw")


def test_label_build_overlapping_windows_and_a_duplicated_segment(be, tmp_path, capsys):
    """step 512, and every reference holds its third window's call twice: unmutated in front, mutated in place.  The window fits the
    copy in front (the better score; on a tie the smaller end), out of order with its neighbours: the chain filter has to choose, and
    its choice -- every window's status -- must be the restatement's."""
    from radian_amd import label_build
    ids, raws, refs, fast5_dir, tsv, model = _job(tmp_path, be, seed=32, n_reads=4, duplicate=True)
    rows, kept = _expected(be, ids, raws, refs, 512, 0.0)
    out, man = str(tmp_path / "shards"), str(tmp_path / "windows.tsv")
    st = label_build.main([fast5_dir, tsv, "-o", out, "--manifest", man, "--sig-model", model, "--sig-config", "none", "--step-size", "512",
                           "--val-fraction", "0", "--batch-reads", "2"])
    capsys.readouterr()
    _compare(out, man, rows, kept, 50000)
    off = [k for k, v in rows.items() if v[0] == "off-chain"]
    with capsys.disabled():
        print(f"\n[label_build chain] {len(rows)} windows, {st['kept']} kept, off-chain: {off}")
    for rid in ids:   # window 4 at step 512 is window 2 at step 1024: it fits the copy in front exactly, before its neighbours' spans
        f = rows[(rid, 4)][1]
        m = sum(f["counts"][:3])
        assert f["counts"] == (m, 0, 0, 0) and f["score"] == 2 * m and f["ref_end"] <= 50 + m, (rid, f)
    assert off   # the inputs do exercise the chain filter
    assert kept["train"] and not kept["val"] and not os.listdir(os.path.join(out, "val"))


def test_zz_duration_of_this_file(capsys):
    """the file's share of the GPU suite's 900-s budget (the last test of the file)"""
    with capsys.disabled():
        print(f"\n[test_gpu_label_build] {time.perf_counter() - _T0:.1f} s for the whole file")
    assert time.perf_counter() - _T0 < 450
