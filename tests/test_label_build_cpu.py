"""No-GPU checks of training-shard building: the restatement of the fitting alignment (tests/_fit_ref.py) against brute force, the
TFRecord writer's round trip (the library's reader and an independent protobuf decoder), and label_build's host rules -- chain filter,
split, TSV parsing."""
import itertools
import os
import struct

import numpy as np
import pytest

import _fit_cases as fc
import _fit_ref as fr
import _tfrecord_writer as tw


# ---------------------------------------------------------------- the restatement of the contract
def _small_cases():
    rng = np.random.default_rng(14)
    cases = [([], [0]), ([], [1, 2, 3]), ([2], [2]), ([4], [0]), ([4, 4, 4], [0, 1]), ([0] * 12, [0] * 6), ([0, 1] * 6, [0, 1, 0, 1]),
             ([0, 1, 2, 3], [0, 1, 2, 3, 0, 1])]
    for _ in range(160):
        n, m = int(rng.integers(0, 13)), int(rng.integers(1, 7))
        alpha = int(rng.integers(1, 5))   # small alphabets make ties
        ref = [int(c) for c in rng.integers(0, alpha + 1, size=n)]
        if rng.random() < 0.3:
            ref = [4 if rng.random() < 0.2 else c for c in ref]
        cases.append((ref, [int(c) for c in rng.integers(0, min(alpha, 4), size=m)]))
    return cases


def test_restatement_against_brute_force_over_every_span():
    seen4 = 0
    for ref, q in _small_cases():
        assert len(ref) <= 12 and len(q) <= 6
        seen4 += 4 in ref
        got = fr.fit(ref, q)
        score, end = fr.brute(ref, q)
        assert got["score"] == score, (ref, q)
        assert got["ref_end"] == end, (ref, q)
        nm, ns, ni, nd = got["counts"]
        assert nm + ns + ni == len(q) and nm + ns + nd == got["ref_end"] - got["ref_start"] and 0 <= got["ref_start"] <= got["ref_end"]
        # the traced columns add up to the score
        assert fr._global(ref[got["ref_start"]:got["ref_end"]], q, fr.SCORES) == score
    assert seen4 >= 10


def test_restatement_every_reference_of_the_full_alphabet():
    """all of 0..4 on the reference side, exhaustively at n = 4, against brute force"""
    for ref in itertools.product(range(5), repeat=4):
        for q in ([0, 1], [2, 2, 3]):
            got = fr.fit(ref, q)
            assert (got["score"], got["ref_end"]) == fr.brute(ref, q), (ref, q)


def test_row_wise_restatement_equals_the_cell_wise_one():
    rng = np.random.default_rng(15)
    for k in range(60):
        n, m = int(rng.integers(0, 90)), int(rng.integers(1, 40))
        alpha = 1 if k % 10 == 0 else 2 if k % 10 == 1 else 4
        ref = rng.integers(0, alpha, size=n)
        if k % 3 == 0 and n:
            ref[rng.integers(0, n, size=3)] = 4
        q = rng.integers(0, alpha, size=m)
        assert fr.fit_rows(ref, q) == fr.fit(ref, q)


_SET_IDS = lambda sc: "_".join(str(v) for v in sc)


@pytest.mark.parametrize("sc", fr.ACCEPTED_SETS, ids=_SET_IDS)
def test_restatement_against_brute_force_under_every_accepted_score_set(sc):
    """gap_open <= gap_extend: the contract's recurrence is the stated gap cost (brute: every span, a three-matrix global alignment)"""
    rng = np.random.default_rng(16)
    for k in range(25):
        n, m = int(rng.integers(0, 14)), int(rng.integers(1, 9))
        alpha = 1 + k % 4
        ref = [int(c) for c in rng.integers(0, alpha, size=n)]
        if k % 5 == 0:
            ref = [4 if rng.random() < 0.25 else c for c in ref]
        q = [int(c) for c in rng.integers(0, alpha, size=m)]
        got = fr.fit(ref, q, sc)
        assert (got["score"], got["ref_end"]) == fr.brute(ref, q, sc), (ref, q, sc)
        nm, ns, ni, nd = got["counts"]
        assert nm + ns + ni == len(q) and nm + ns + nd == got["ref_end"] - got["ref_start"] and 0 <= got["ref_start"] <= got["ref_end"]


@pytest.mark.parametrize("sc", fr.ACCEPTED_SETS, ids=_SET_IDS)
def test_row_wise_restatement_equals_the_cell_wise_one_under_every_accepted_score_set(sc):
    rng = np.random.default_rng(17)
    for k in range(12):
        n, m = ((130, 70), (0, 5), (1, 70), (64, 64))[k] if k < 4 else (int(rng.integers(0, 131)), int(rng.integers(1, 71)))
        alpha = 1 if k % 6 == 4 else 2 if k % 6 == 5 else 4
        ref = rng.integers(0, alpha, size=n)
        if k % 3 == 0 and n:
            ref[rng.integers(0, n, size=3)] = 4
        q = rng.integers(0, alpha, size=m)
        assert fr.fit_rows(ref, q, sc) == fr.fit(ref, q, sc), (k, n, m, sc)


def test_open_above_extend_is_not_the_stated_gap_cost():
    """why rd_fit_batch refuses gap_open > gap_extend: the recurrence then differs from brute force over the stated cost model"""
    rng = np.random.default_rng(16)
    differ = 0
    for k in range(25):
        ref = [int(c) for c in rng.integers(0, 1 + k % 4, size=int(rng.integers(0, 14)))]
        q = [int(c) for c in rng.integers(0, 1 + k % 4, size=int(rng.integers(1, 9)))]
        got, want = fr.fit(ref, q, fr.REFUSED_SET)["score"], fr.brute(ref, q, fr.REFUSED_SET)[0]
        assert got >= want
        differ += got != want
    assert differ >= 1
    with pytest.raises(AssertionError):
        fr.fit_rows([0, 1], [0], fr.REFUSED_SET)


def test_gpu_cases_tell_a_flipped_tie_select_apart_under_every_score_set():
    """the cases tests/test_gpu_label_build.py runs under every score set: with the tie of extend and close inside a deletion run (E) or
    an insertion run (F) decided the other way, the restatement's result changes on at least one of them under every set -- so a kernel
    with `ee >= eo` or `fe >= fo` written `>` fails that test under every set, not only under some"""
    refs, queries, qref = fc.fit_cases_small()
    cases = [([int(c) for c in refs[r]], [int(c) for c in q]) for q, r in zip(queries, qref) if len(q) <= 130]   # (the long ones: seconds each)
    for sc in fr.SMALL_SETS:
        seen = set()
        for ref, q in cases:
            mats = fr._matrices_rows(ref, q, sc)
            want = fr._trace(*mats, ref, q, sc)
            seen |= {flip for flip in "EF" if fc.trace_tie_flipped(*mats, ref, q, sc, flip) != want}
        assert seen == {"E", "F"}, (sc, seen)


def test_row_wise_sentinel_lies_below_every_value_at_the_largest_scores():
    """fit_rows stores -inf as NEG32 = -2^29 in int32.  H(i, j) >= H(i, 0) + open + (j - 1) * extend >= -65535 * 1024 and E, F >= an H
    + open, so nothing reachable is below -65535 * 1026 > -2^27: the sentinel, and the sentinel plus a gap score, stay apart from every
    value.  Checked on the stored matrices and against the cell-wise restatement (whose -inf is -2^40) with the longest query."""
    sc = fr.ACCEPTED_SETS[-2]
    assert sc == (65535, -65535, -65535, -65535)
    rng = np.random.default_rng(18)
    for ref, q in ((rng.integers(0, 4, size=40), rng.integers(0, 4, size=1024)), (np.full(30, 4), rng.integers(0, 4, size=1024)),
                   (rng.integers(0, 2, size=300), rng.integers(2, 4, size=200))):
        H, E, F = fr._matrices_rows([int(c) for c in ref], [int(c) for c in q], sc)
        for X in (H, E[1:, 1:], F[:, 1:]):
            assert X.min() >= -65535 * 1026 > fr.NEG32 // 4
        assert (E[0] == fr.NEG32).all() and (E[:, 0] == fr.NEG32).all() and (F[:, 0] == fr.NEG32).all()
        assert fr.fit_rows(ref, q, sc) == fr.fit(ref, q, sc)


def test_code_4_matches_nothing_itself_included():
    assert fr._sub(4, 4, fr.SCORES) == fr.SCORES[1]
    got = fr.fit([0, 1, 4, 2, 3], [0, 1, 2, 3])
    assert got["counts"][0] == 4 and got["counts"][3] == 1 and (got["ref_start"], got["ref_end"]) == (0, 5)


# ---------------------------------------------------------------- writer round trip
def _decode_with_protobuf(data):
    """[(signal, label, signal_length, label_length)] by the protobuf classes of tests/_tfrecord_writer.py, both checksums checked"""
    Example = tw._classes(True)
    out, at = [], 0
    while at < len(data):
        (n,) = struct.unpack_from("<Q", data, at)
        assert struct.unpack_from("<I", data, at + 8)[0] == tw.masked_crc(data[at:at + 8])
        body = data[at + 12: at + 12 + n]
        assert struct.unpack_from("<I", data, at + 12 + n)[0] == tw.masked_crc(body)
        ex = Example.FromString(body)
        f = ex.features.feature
        assert sorted(f.keys()) == ["label", "label_length", "signal", "signal_length"]
        out.append((np.array(f["signal"].float_list.value, dtype=np.float32), list(f["label"].float_list.value),
                    list(f["signal_length"].int64_list.value), list(f["label_length"].int64_list.value)))
        at += 16 + n
    assert at == len(data)
    return out


def _records(rng):
    lens = [(0, 1), (1, 1024), (255, 1024), (17, 300), (60, 1)]   # (label length, signal_length)
    sig = rng.normal(size=(len(lens), 1024)).astype(np.float32)
    sig[0, 0], sig[1, 1] = np.float32(-0.0), np.float32(1e-42)   # a signed zero and a subnormal travel bit by bit
    labels = [rng.integers(0, 4, size=L).astype(np.uint8) for L, _ in lens]
    return sig, [s for _, s in lens], labels


def test_writer_round_trip_through_the_reader_and_protobuf(tmp_path):
    from radian_amd.backend import Backend, tfrecord_write
    from radian_amd.tfrecord import read_shard
    rng = np.random.default_rng(3)
    sig, il, labels = _records(rng)
    p = str(tmp_path / "a.tfrecords")
    Backend.tfrecord_write(p, sig, il, labels)
    sh = read_shard(p)
    assert len(sh) == len(il)
    assert sh.signals.tobytes() == sig.tobytes()
    assert list(sh.input_len) == il and list(sh.label_len) == [len(l) for l in labels]
    for i, l in enumerate(labels):
        assert np.array_equal(sh.label(i), l)
    recs = _decode_with_protobuf(open(p, "rb").read())
    assert len(recs) == len(il)
    for i, (s, lab, sl, ll) in enumerate(recs):
        assert s.tobytes() == sig[i].tobytes() and lab == [float(c) for c in labels[i]] and sl == [il[i]] and ll == [len(labels[i])]
    # byte-identical on rewrite
    first = open(p, "rb").read()
    tfrecord_write(p, sig, il, labels)
    assert open(p, "rb").read() == first
    # append mode: two calls make the file one call makes
    q = str(tmp_path / "b.tfrecords")
    tfrecord_write(q, sig[:2], il[:2], labels[:2])
    tfrecord_write(q, sig[2:], il[2:], labels[2:], append=True)
    assert open(q, "rb").read() == first
    # and an existing file is truncated without append
    tfrecord_write(q, sig[:1], il[:1], labels[:1])
    assert len(read_shard(q)) == 1
    # no record at all: an empty shard
    tfrecord_write(q, np.zeros((0, 1024), np.float32), [], [])
    assert os.path.getsize(q) == 0 and len(read_shard(q)) == 0


def test_writer_matches_the_independent_encoder_field_by_field(tmp_path):
    """the reader's view of this writer's shard == its view of the protobuf encoder's shard of the same records"""
    from radian_amd.backend import tfrecord_write
    from radian_amd.tfrecord import read_shard
    rng = np.random.default_rng(4)
    sig, il, labels = _records(rng)
    a, b = str(tmp_path / "a.tfrecords"), str(tmp_path / "b.tfrecords")
    tfrecord_write(a, sig, il, labels)
    tw.write_shard(b, [(sig[i], [int(c) for c in labels[i]], il[i], len(labels[i])) for i in range(len(il))])
    x, y = read_shard(a), read_shard(b)
    assert x.signals.tobytes() == y.signals.tobytes() and list(x.input_len) == list(y.input_len)
    assert x.labels.tobytes() == y.labels.tobytes() and list(x.label_off) == list(y.label_off)


def test_writer_refuses_bad_values(tmp_path):
    from radian_amd.backend import RadianHipError, tfrecord_write
    sig = np.zeros((1, 1024), np.float32)
    p = str(tmp_path / "x.tfrecords")
    for il, lab in (([0], [[1]]), ([1025], [[1]])):
        with pytest.raises(RadianHipError, match="signal_length"):
            tfrecord_write(p, sig, il, lab)
    with pytest.raises(ValueError):
        tfrecord_write(p, sig, [5], [[4]])
    assert not os.path.exists(p)
    with pytest.raises(OSError):
        tfrecord_write(str(tmp_path / "no" / "dir.tfrecords"), sig, [5], [[1]])


# ---------------------------------------------------------------- label_build's host rules
def test_chain_filter_hand_cases():
    from radian_amd.label_build import chain
    cases = {
        (): [],
        (5,): [0],
        (0, 10, 20, 30): [0, 1, 2, 3],
        (0, 10, 5, 20): [0, 1, 3],            # tie between dropping 10 and dropping 5: the earlier indices
        (0, 100, 10, 20, 30): [0, 2, 3, 4],   # a call that fitted a repeat further on
        (50, 0, 10, 20): [1, 2, 3],
        (30, 20, 10): [0],                    # every window alone: the first
        (7, 7, 7): [0, 1, 2],                 # equal starts do not decrease
        (10, 0, 20, 5, 30): [0, 2, 4],        # three chains of length 3: [0,2,4] < [1,2,4] < [1,3,4]
        (3, 1, 2, 1, 2): [1, 2, 4],           # [1,2,4] before [1,3,4]
    }
    for starts, want in cases.items():
        assert chain(list(starts)) == want, starts
        assert fr.chain(list(starts)) == want, starts
    rng = np.random.default_rng(8)
    for _ in range(300):   # against every subset, small
        s = [int(v) for v in rng.integers(0, 6, size=int(rng.integers(0, 9)))]
        best = []
        for r in range(len(s), 0, -1):
            ok = [c for c in itertools.combinations(range(len(s)), r) if all(s[c[k]] <= s[c[k + 1]] for k in range(r - 1))]
            if ok:
                best = list(min(ok))
                break
        assert chain(s) == best and fr.chain(s) == best, s


def test_split_function():
    from radian_amd.label_build import is_val
    from radian_amd.tfrecord import crc32c
    ids = [f"read-{k:04d}" for k in range(2000)]
    for rid in ids[:50]:
        assert is_val(rid, 0.05) == (tw.crc32c(rid.encode()) % 10000 < 500)
        assert crc32c(rid.encode()) == tw.crc32c(rid.encode())
    assert not any(is_val(r, 0.0) for r in ids) and all(is_val(r, 1.0) for r in ids)
    share = sum(is_val(r, 0.05) for r in ids) / len(ids)
    assert 0.03 < share < 0.07   # 2000 draws at p = 0.05: sd 0.005
    assert [is_val(r, 0.05) for r in ids] == [is_val(r, 0.05) for r in ids]
    assert all(is_val(r, 0.3) for r in ids if is_val(r, 0.05))   # a larger fraction only adds reads


def test_tsv_parsing(tmp_path):
    from radian_amd.label_build import encode_reference, read_ref_tsv
    p = tmp_path / "read_ref.tsv"
    p.write_text("read\ttxt\tseq\nr1\tENST1\tACGU\nr2\tENST2\tacgtNnRx-\nr1\tENST3\tTTGA\n")
    refs = read_ref_tsv(str(p))
    assert refs == {"r1": "TTGA", "r2": "acgtNnRx-"} and "r3" not in refs
    assert list(encode_reference("ACGU")) == [3, 2, 1, 0]            # reversed, not complemented; U = T
    assert list(encode_reference("acgtNnRx-")) == [4, 4, 4, 4, 4, 3, 2, 1, 0]
    assert list(encode_reference("")) == [] and encode_reference("AC").dtype == np.uint8
    p.write_text("read\ttxt\tseq\nr1\tENST1\tACGU\nr2 ENST2 ACGT\n")
    with pytest.raises(ValueError, match="line 3"):
        read_ref_tsv(str(p))
    p.write_text("read\ttxt\tseq\nr1\tENST1\tACGU\textra\n")
    with pytest.raises(ValueError, match="line 2"):
        read_ref_tsv(str(p))


def test_ctc_rows_and_selection_restatement_agree_on_statuses():
    from radian_amd.label_build import ctc_rows
    for lab in ([], [1], [1, 1], [0, 1, 1, 1, 2, 2], [3] * 255):
        assert ctc_rows(np.array(lab, dtype=np.uint8)) == fr.ctc_need(lab)
    assert ctc_rows(np.array([2, 2, 2], dtype=np.uint8)) == 5
