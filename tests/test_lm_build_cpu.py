"""No-GPU checks of the RNA-model builder's host side: the FASTA scanner (rd_fasta_scan) against tests/_lm_ref.read_fasta, the model
writer (rd_lm_json_write) against both readers, the command line's argument errors, and scanner + writer under the sanitizers."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import _lm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lm():
    from radian_amd import build, _lib, lm as lm_mod
    build.build()
    _lib.load()
    return lm_mod


GENCODE = ">ENST1|ENSG1|OTTHUMG1|OTTHUMT1|NAME-201|NAME|1500|protein_coding|"
LNC = ">ENST2|ENSG2|-|-|LNC-201|LNC|900|lncRNA|"

TEXTS = {
    "plain": b">a\nACGT\n>b\nTTGA\n",
    "multi_line": b">a desc\nACG\nTAC\nGG\n>b\nA\n",
    "crlf": b">a\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "no_final_newline": b">a\nACGT\n>b\nTTG",
    "lower_and_u": b">a\nacgu\nACGU\nuUtT\n",
    "iupac_breaks": b">a\nACNNGTRYKMACGT\n>b\nnnnn\n",
    "star_dash_space": b">a\nAC-GT*\n A C\tG T \n",
    "empty_records": b">a\n>b\n\n>c\nACGT\n>d\n",
    "blank_lines_first": b"\n\n>a\nAC\n\nGT\n",
    "header_only": b">a",
    "empty": b"",
    "gt_inside_header": b">a>b|c\nAC\n",
    "filtered": (GENCODE + "\nACGTAC\n" + LNC + "\nGGGG\n" + GENCODE + "\nTT\nAA\n").encode(),
}


def check_same(lm, tmp_path, name, data, field=None, value=None):
    path = tmp_path / (name + ".fa")
    path.write_bytes(data)
    codes, off, info = lm.read_fasta(str(path), field, value)
    rc, ro, ri = ref.read_fasta(data, field, value)
    assert info == ri, name
    assert codes.dtype == np.uint8 and off.dtype == np.int64
    assert np.array_equal(codes, rc) and np.array_equal(off, ro), name
    return codes, off, info


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_scanner_matches_the_restatement(lm, tmp_path, name):
    check_same(lm, tmp_path, name, TEXTS[name])


def test_scanner_rules_by_hand(lm, tmp_path):
    codes, off, info = check_same(lm, tmp_path, "iupac", TEXTS["iupac_breaks"])
    assert codes.tolist() == [0, 1, 255, 255, 2, 3, 255, 255, 255, 255, 0, 1, 2, 3, 255, 255, 255, 255] and off.tolist() == [0, 14, 18]
    codes, off, info = check_same(lm, tmp_path, "lower", TEXTS["lower_and_u"])
    assert codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 3, 3, 3, 3]
    codes, off, info = check_same(lm, tmp_path, "sds", TEXTS["star_dash_space"])
    assert codes.tolist() == [0, 1, 255, 2, 3, 255, 0, 1, 2, 3]
    codes, off, info = check_same(lm, tmp_path, "empty_records", TEXTS["empty_records"])
    assert off.tolist() == [0, 0, 0, 4, 4] and info == {"records": 4, "kept": 4, "bases": 4}
    codes, off, info = check_same(lm, tmp_path, "empty", TEXTS["empty"])
    assert len(codes) == 0 and off.tolist() == [0] and info["records"] == 0


def test_scanner_header_filter(lm, tmp_path):
    data = TEXTS["filtered"]
    codes, off, info = check_same(lm, tmp_path, "pc", data, 7, "protein_coding")
    assert info == {"records": 3, "kept": 2, "bases": 10} and off.tolist() == [0, 6, 10]
    codes, off, info = check_same(lm, tmp_path, "lnc", data, 7, "lncRNA")
    assert info["kept"] == 1 and codes.tolist() == [2, 2, 2, 2]
    assert check_same(lm, tmp_path, "f0", data, 0, "ENST2")[2]["kept"] == 1
    assert check_same(lm, tmp_path, "prefix", data, 7, "protein")[2]["kept"] == 0          # the whole field, not a prefix
    assert check_same(lm, tmp_path, "beyond", data, 40, "protein_coding")[2]["kept"] == 0  # a field the header does not have
    assert check_same(lm, tmp_path, "last_empty", data, 8, "")[2]["kept"] == 3             # the text after the last |
    with pytest.raises(ValueError):
        lm.read_fasta(str(tmp_path / "pc.fa"), 7, None)


def test_scanner_reads_gzip(lm, tmp_path):
    data = TEXTS["filtered"] * 50
    path = tmp_path / "t.fa.gz"
    path.write_bytes(gzip.compress(data))
    codes, off, info = lm.read_fasta(str(path), 7, "protein_coding")
    rc, ro, ri = ref.read_fasta(data, 7, "protein_coding")
    assert info == ri and np.array_equal(codes, rc) and np.array_equal(off, ro) and info["kept"] == 100


@pytest.mark.parametrize("data,record,line", [
    (b">a\nACGT\nAC1T\n", 1, 3),
    (b">a\nACGT\n>b\nAC\nGG\nA.C\n", 2, 6),
    (b">a\r\nAC\r\n>b\r\n>c\r\nA>C\r\n", 3, 5),
    (b">a\nAC\x00GT\n", 1, 2),
    (b">a\nAC\xc3\xa9\n", 1, 2),
    (b"ACGT\n>a\nAC\n", 0, 1),
    (b">a|x\nAC\n>b|y\nA;C\n", 2, 4),          # an error in a record the filter drops is still an error
])
def test_scanner_errors_name_record_and_line(lm, tmp_path, data, record, line):
    path = tmp_path / "bad.fa"
    path.write_bytes(data)
    with pytest.raises(ValueError) as ei:
        lm.read_fasta(str(path), 1, "x") if b"|" in data else lm.read_fasta(str(path))
    assert f"record {record}, line {line}:" in str(ei.value), str(ei.value)
    with pytest.raises(ValueError) as er:
        ref.read_fasta(data)
    assert f"record {record}, line {line}:" in str(er.value)


def random_tables(rng, k):
    n = 4 ** k
    t = rng.dirichlet([0.3] * 4, size=n)
    special = np.array([0.0, 1.0, 5e-324, 2.2250738585072014e-308, 1e-310, 0.1, 1.0 / 3.0, 0.30000000000000004, 1e-5, 1e22, 123456789012345680.0,
                        2.0 ** -1074 * 3, np.nextafter(1.0, 0.0), np.nextafter(0.25, 1.0), 5e-5, 1.7976931348623157e308])
    rows = rng.integers(0, n, size=min(n, 40))
    t[rows] = rng.choice(special, size=(len(rows), 4))
    t[rng.integers(0, n, size=min(n, 8))] = rng.random((min(n, 8), 4)) * 10.0 ** rng.integers(-300, 0, size=(min(n, 8), 1))
    return t


@pytest.mark.parametrize("k,sparse", [(1, False), (2, True), (3, False), (5, True), (6, False)])
def test_writer_round_trips_bit_for_bit_through_both_readers(lm, tmp_path, k, sparse):
    rng = np.random.default_rng(100 + k)
    t = random_tables(rng, k)
    if sparse:
        t[rng.random(4 ** k) < 0.3] = np.nan
        t[0] = 0.5                                          # (the native reader takes k from the first key: any first key will do)
    path = str(tmp_path / "m.json")
    rows, nbytes = lm.write_json(path, t, k)
    present = ~np.isnan(t[:, 0])
    assert rows == int(present.sum()) and nbytes == os.path.getsize(path)
    text = open(path).read()
    assert "NaN" not in text and "nan" not in text
    raw = json.load(open(path))                             # the reference's reader, basecall.py:48-57
    assert len(raw) == rows and all(len(key) == k for key in raw)
    assert list(raw) == sorted(raw)                         # row order
    back, kk = lm.table_from_dict(raw)
    assert kk == k and back.tobytes() == t.tobytes()        # (NaN rows: the same quiet NaN np.nan is)
    got = lm._load_json_native(path)
    assert got is not None, "the library's reader must take the writer's text"
    assert got[1] == k and np.array_equal(got[0].view(np.uint64)[present], t.view(np.uint64)[present]) and np.isnan(got[0][~present]).all()
    t2, k2 = lm.load_json(path, native=True)
    assert k2 == k and np.array_equal(np.isnan(t2), np.isnan(t)) and np.array_equal(t2[present], t[present])


def test_writer_refusals(lm, tmp_path):
    path = str(tmp_path / "m.json")
    t = np.full((16, 4), 0.25)
    for bad in (np.inf, -0.5, -0.0):
        u = t.copy()
        u[3, 2] = bad
        with pytest.raises(ValueError):
            lm.write_json(path, u, 2)
    u = t.copy()
    u[3, 2] = np.nan
    with pytest.raises(ValueError, match="mixes NaN"):
        lm.write_json(path, u, 2)
    with pytest.raises(ValueError):
        lm.write_json(path, t, 3)
    with pytest.raises(ValueError, match="cannot open"):
        lm.write_json(str(tmp_path / "no_such_dir" / "m.json"), t, 2)
    lm.write_json(path, np.full((4, 4), np.nan), 1)
    assert json.load(open(path)) == {}


def test_restatement_is_self_consistent():
    """the vectorised counts equal the contract's loop; marginals equal counting at the lower order wherever a window of k + 1 exists"""
    seqs = ref.markov_transcripts(3, 6, 300) + ["ACGTNNACGTACGTNACG", "AC", "", "NNNN"]
    codes, off = ref.encode(seqs)
    for k in (1, 3, 5):
        for aw in (False, True):
            C = ref.counts(codes, off, k, aw)
            assert np.array_equal(C, ref.counts_loop(codes, off, k, aw))
            M = ref.marginals(C, k)
            assert all(M[j].sum() == C.sum() for j in range(k + 1))
            tab, order = ref.table(C, k)
            assert not np.isnan(tab).any() and np.allclose(tab.sum(1), 1.0)
            assert (order == k).sum() == (C.sum(1) > 0).sum()
    # direction: the reversed count of t is the as-written count of reversed(t)
    rev = ref.encode([s[::-1] for s in seqs])
    assert np.array_equal(ref.counts(codes, off, 3), ref.counts(rev[0], rev[1], 3, True))
    # hand case, k = 1: t = "ACG" -> d = "GCA": windows (G -> C), (C -> A)
    c, o = ref.encode(["ACG"])
    C = ref.counts(c, o, 1)
    assert C[2, 1] == 1 and C[1, 0] == 1 and C.sum() == 2


@pytest.mark.parametrize("argv,word", [
    ([], "FASTA"),
    (["x.fa"], "--output"),
    (["x.fa", "-o", "m.json", "--context-len", "0"], "--context-len"),
    (["x.fa", "-o", "m.json", "--context-len", "14"], "--context-len"),
    (["x.fa", "-o", "m.json", "--field", "3"], "--value"),
    (["x.fa", "-o", "m.json", "--value", "s"], "--field"),
    (["x.fa", "-o", "m.json", "--field", "-1", "--value", "s"], "--field"),
    (["x.fa", "-o", "m.json", "--protein-coding", "--field", "2", "--value", "s"], "--protein-coding"),
    (["x.fa", "-o", "m.json", "--pseudocount", "-1"], "--pseudocount"),
    (["x.fa", "-o", "m.json", "--pseudocount", "nan"], "--pseudocount"),
    (["x.fa", "-o", "m.json", "--rna-threshold", "nan"], "--rna-threshold"),
    (["--score", "m.json"], "--heldout"),
    (["--score", "m.json", "--heldout", "h.fa", "-o", "n.json"], "--score"),
    (["x.fa", "--score", "m.json", "--heldout", "h.fa"], "--score"),
    (["/no/such/file.fa", "-o", "m.json"], "no such file"),
    (["--score", "/no/such/model.json", "--heldout", "h.fa"], "--score"),
])
def test_command_line_argument_errors(lm, argv, word):
    from radian_amd import lm_build
    with pytest.raises(SystemExit) as ei:
        lm_build.main(argv)
    assert isinstance(ei.value.code, str) and ei.value.code.startswith("lm_build: ") and word in ei.value.code, ei.value.code


def test_command_line_reports_scanner_errors_and_empty_selections(lm, tmp_path):
    from radian_amd import lm_build
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">a\nAC!T\n")
    with pytest.raises(SystemExit) as ei:
        lm_build.main([str(bad), "-o", str(tmp_path / "m.json")])
    assert "record 1, line 2" in ei.value.code
    ok = tmp_path / "ok.fa"
    ok.write_bytes(TEXTS["filtered"])
    with pytest.raises(SystemExit) as ei:
        lm_build.main([str(ok), "-o", str(tmp_path / "m.json"), "--field", "7", "--value", "tRNA"])
    assert "--field 7" in ei.value.code and not (tmp_path / "m.json").exists()
    with pytest.raises(SystemExit) as ei:
        lm_build.main([str(ok), "-o", str(tmp_path / "m.json"), "--unseen", "other"])
    assert ei.value.code == 2                               # argparse's own refusal of a choice


def test_fasta_scanner_and_model_writer_under_address_sanitizer(tmp_path):
    """csrc/lmbuild.hip's scanner and csrc/lmjson.hip's writer compiled for the CPU with -fsanitize=address,undefined (tests/asan_fasta.cpp):
    valid, mutated and truncated FASTA texts in exact-size heap buffers, count pass then fill pass into exact-size outputs; tables with NaN
    rows and extreme values written and read back."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_fasta"
    csrc = os.path.join(ROOT, "radian_amd", "csrc")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", os.path.join(csrc, "lmbuild.hip"), os.path.join(csrc, "lmjson.hip"),
                        os.path.join(ROOT, "tests", "asan_fasta.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "40000", str(tmp_path / "w.json")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-500:], r.stderr.decode()[-3000:])
    accepted = int(r.stdout.split()[0])
    assert 4000 < accepted < 39000          # the harness feeds both kinds
