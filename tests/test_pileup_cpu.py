"""No-GPU checks of the pileup: rd_pileup_host equals the restatement (tests/_pileup_ref.py) on every seeded case of
tests/_pileup_cases.py, every case is what its name says, the header's profile layout is the restatement's, the PAF reader's refusals and
skip counters, the SAM line invariants, the planted variant of the command line's data set, and the host code of pileup.hip under
AddressSanitizer + UBSan as a stand-alone program (tests/asan_pileup.cpp).  Every comparison of integers is for equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _pileup_cases as pc
import _pileup_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in (pc.length_grid(), pc.ops_cases(), pc.hot(), pc.disjoint(), pc.sparse()):
        c = dict(c)
        if c["ops"] is None:
            c["ops"], c["scores"] = ref.aligned(c["spans"], c["reads"])
        c["sites"], c["prof"], c["out"] = ref.pileup(c["ops"], c["spans"], c["reads"], c["site0"], c["n_sites"])
        out.append(c)
    return {c["name"]: c for c in out}


def test_host_twin_equals_the_restatement(cases):
    from radian_amd.backend import pileup_host
    for c in cases.values():
        pairs, sites, prof = pileup_host(c["ops"], c["spans"], c["reads"], c["site0"], c["n_sites"])
        assert np.array_equal(pairs.out, c["out"]), c["name"]
        assert np.array_equal(sites[:c["n_sites"]], c["sites"][:c["n_sites"]]), c["name"]
        assert np.array_equal(prof, c["prof"]), c["name"]
        # a second call adds into the same tables
        pileup_host(c["ops"], c["spans"], c["reads"], c["site0"], c["n_sites"], sites, prof)
        assert np.array_equal(sites[:c["n_sites"]], 2 * c["sites"][:c["n_sites"]]) and np.array_equal(prof, 2 * c["prof"])


def test_host_twin_refuses():
    from radian_amd.backend import RadianHipError, pileup_host
    ok = dict(ops=[b"MMI"], refs=[b"AC"], reads=[b"ACG"], site0=[3], n_sites=5)
    pileup_host(**ok)
    for change in (dict(ops=[b"MMS"]), dict(ops=[b"MM"]), dict(ops=[b"MMII"]), dict(ops=[b"MDI"]), dict(site0=[4]), dict(site0=[-1]), dict(n_sites=4),
                   dict(n_sites=(1 << 30) + 1)):
        with pytest.raises(RadianHipError):
            pileup_host(**dict(ok, **change))


def test_cases_are_what_their_names_say(cases):
    g = cases["length_grid"]
    lens = {len(o) for o in g["ops"]}
    assert {0, 64, 65, 200} <= lens and any(0 < L < 64 for L in lens) and any(L > 192 for L in lens)   # 0, < 64, 64, 65, several chunks
    assert {(len(s), len(r)) for s, r in zip(g["spans"], g["reads"])} == {(n, m) for n in pc.GRID for m in pc.GRID}
    assert (g["out"][:, 0] == ref.NO_BASE).any() and (g["out"][:, 0] == ref.OK).any()
    c = cases["ops_cases"]
    by = {n: k for k, n in enumerate(c["names"])}
    ops = lambda n: c["ops"][by[n]]
    out = lambda n: dict(zip(ref.FIELDS, (int(v) for v in c["out"][by[n]])))
    for kind, name in ((b"I", "ins_62_66"), (b"D", "del_62_66")):
        assert ops(name)[61:68] == b"M" + kind * 5 + b"M" and ops(name).index(kind) == 62          # columns 62 .. 66 straddle column 64
    assert ops("ins_run_70").count(b"I") == 70 and ops("del_run_64").count(b"D") == 64 and ops("ins_run_64").count(b"I") == 64
    assert c["prof"][ref.INS_LEN + 63] >= 3 and c["prof"][ref.DEL_LEN + 63] >= 3 and c["prof"][ref.INS_LEN + 62] >= 1       # 64+, 64+, 63
    assert ops("ins_from_col_64")[63:68] == b"MIIIM" and ops("ins_run_whole_chunk")[63:129] == b"M" + b"I" * 64 + b"M"
    assert out("lead_i")["clip_head"] == 3 and out("lead_i")["n_ins"] == 0 and out("trail_i")["clip_tail"] == 2
    assert out("lead_d")["ref_lo"] == 2 and out("lead_d")["n_del"] == 0 and out("trail_d")["ref_hi"] == 3 and len(c["spans"][by["trail_d"]]) == 5
    m = out("lead_trail_mixed")
    assert (m["ref_lo"], m["clip_head"], m["clip_tail"], m["n_del"], m["n_ins"]) == (2, 2, 2, 1, 1) and m["ref_hi"] == len(c["spans"][by["lead_trail_mixed"]]) - 2
    assert out("lead_70_mixed")["clip_head"] == 35 and out("lead_70_mixed")["ref_lo"] == 35
    assert b"DI" in ops("del_then_ins") and b"ID" in ops("ins_then_del")
    for name in ("all_i", "all_d", "all_i_d", "all_i_70", "empty"):
        assert out(name)["status"] == ref.NO_BASE and not set(ops(name)) & set(b"MX")
    assert out("all_i")["clip_head"] == 4 and out("all_d")["clip_head"] == 0
    assert out("single_m") == dict(zip(ref.FIELDS, (0, 0, 0, 1, 0, 0, 1, 0, 0, 0)))
    k = by["x_equal_bytes"]
    assert c["spans"][k] == c["reads"][k] and out("x_equal_bytes")["n_sub"] == 3
    k = by["non_acgt"]
    assert set(c["spans"][k]) - set(b"ACGT") and set(c["reads"][k]) - set(b"ACGT")
    solo, solo_prof, _ = ref.pileup([c["ops"][k]], [c["spans"][k]], [c["reads"][k]], [0], 20)
    assert solo[:, 4].sum() >= 1 and solo_prof[ref.CONF + 24: ref.CONF + 30].sum() >= 2 and solo_prof[ref.INS_BASE + 4] == 1
    k = by["contexts"]
    n = len(c["spans"][k])
    _, kp, _ = ref.pileup([c["ops"][k]], [c["spans"][k]], [c["reads"][k]], [0], n)
    subs = [i for i, o in enumerate(c["ops"][k]) if o == ord("X")]
    assert subs == [0, 1, 2, n - 3, n - 1] and kp[ref.KMER: ref.KMER + 4096].reshape(1024, 4)[:, 1].sum() == 2        # offsets 2 and n - 3 only
    assert kp[ref.CONF: ref.CONF + 30].sum() == n
    h = cases["hot"]
    assert len(h["ops"]) == 300 and len(set(h["site0"])) == 1 and len(h["spans"][0]) == 40 and h["sites"][5:45, :6].sum(axis=1).min() > 200
    d = cases["disjoint"]
    assert len(d["ops"]) == 300 and sorted(d["site0"]) == [40 * p for p in range(300)] and d["sites"][:, 7].sum() == 300 and d["sites"][:, 7].max() == 1
    s = cases["sparse"]
    assert s["n_sites"] == 10 ** 6 and int((s["sites"][:, :6].sum(axis=1) > 0).sum()) == 50


def test_header_layout_is_the_restatements():
    txt = open(os.path.join(ROOT, "include", "radian_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", txt).group(1))
    assert (val("RD_PILEUP_CONF"), val("RD_PILEUP_INS_BASE"), val("RD_PILEUP_KMER"), val("RD_PILEUP_INS_LEN"), val("RD_PILEUP_DEL_LEN"),
            val("RD_PILEUP_PROFILE_LEN")) == (ref.CONF, ref.INS_BASE, ref.KMER, ref.INS_LEN, ref.DEL_LEN, ref.PROFILE_LEN) == (0, 30, 35, 4131, 4195, 4259)
    assert (val("RD_PILEUP_OK"), val("RD_PILEUP_NO_BASE"), val("RD_PILEUP_TOO_LARGE"), val("RD_PILEUP_RES")) == (ref.OK, ref.NO_BASE, ref.TOO_LARGE, len(ref.FIELDS))
    from radian_amd import backend as b
    assert (b.PILEUP_CONF, b.PILEUP_INS_BASE, b.PILEUP_KMER, b.PILEUP_INS_LEN, b.PILEUP_DEL_LEN, b.PILEUP_PROFILE_LEN) == (0, 30, 35, 4131, 4195, 4259)
    assert b.PILEUP_FIELDS == ref.FIELDS and b.PILEUP_CHANNELS == ref.CHANNELS
    assert "analyse_alignment" in txt[txt.index("rd_pileup_open") - 6000: txt.index("int rd_pileup_open")]   # the header says the counts differ
    assert b.pileup_workspace_bytes(100, 80) == b.align_workspace_bytes(100, 80) + 48 + 256 and b.pileup_workspace_bytes(-1, 0) == -1


# ---------------------------------------------------------------------------------------------- the command line's reader and writers
def _transcripts(names, seqs):
    from radian_amd.map import Transcripts, encode_read
    codes = np.concatenate([encode_read(s) for s in seqs])
    return Transcripts(codes, np.concatenate([[0], np.cumsum([len(s) for s in seqs])]), names)


def test_paf_reader_refusals_and_skip_counters(tmp_path):
    from radian_amd import pileup as cli
    names, seqs, reads, paf, _ = pc.cli_case()
    tr = _transcripts(names, seqs)
    path = tmp_path / "map.paf"
    path.write_text("".join(l + "\n" for l in paf))
    first, counters = cli.read_paf(str(path), tr)
    assert counters == {"minus-strand": 1, "duplicate": 1}
    assert "read_017" not in first and "read_023" not in first and len(first) == len(reads) - 2
    assert first["read_031"][4] == 31 % 3 and first["read_031"][3] > 10          # the first line, not the second
    good = paf[0].split("\t")

    def refused(cols, word):
        bad = tmp_path / "bad.paf"
        bad.write_text(paf[1] + "\n" + "\t".join(str(c) for c in cols) + "\n")
        with pytest.raises(SystemExit) as ei:
            cli.read_paf(str(bad), tr)
        assert "line 2" in str(ei.value) and word in str(ei.value), str(ei.value)

    refused(good[:5] + ["tx_z"] + good[6:], "tx_z")
    refused(good[:6] + [int(good[6]) + 1] + good[7:], "length")
    refused(good[:8] + [int(good[6]) + 1] + good[9:], "out of range")
    refused(good[:7] + [int(good[8]) + 1] + good[8:], "out of range")
    refused(good[:3] + [int(good[1]) + 1] + good[4:], "out of range")
    refused(good[:2] + [-1] + good[3:], "out of range")
    refused(good[:4] + ["*"] + good[5:], "strand")
    refused(good[:5], "PAF")


@pytest.fixture(scope="module")
def cli_expected():
    names, seqs, reads, paf, alt = pc.cli_case()
    return names, seqs, reads, paf, alt, ref.cli_files(names, seqs, reads, paf)


def test_sam_line_invariants(cli_expected):
    from radian_amd import pileup as cli
    names, seqs, reads, paf, _, exp = cli_expected
    body = [l for l in exp["sam"].splitlines() if not l.startswith("@")]
    assert len(body) == int((exp["out"][:, 0] == ref.OK).sum()) == len(reads) - 2 and exp["skipped"] == 2
    by_name = dict(reads)
    clipped = 0
    for k, line in enumerate(body):
        c = line.split("\t")
        f = dict(zip(ref.FIELDS, (int(v) for v in exp["out"][k])))
        parts = re.findall(r"(\d+)([=XIDS])", c[5])
        assert "".join(n + o for n, o in parts) == c[5]
        use = lambda kinds: sum(int(n) for n, o in parts if o in kinds)
        assert use("=XIS") == len(by_name[c[0]]) == len(c[9]) and c[9] == by_name[c[0]]          # the read as written, all of it
        assert use("=XD") == f["ref_hi"] - f["ref_lo"]
        assert c[11] == f"NM:i:{f['n_sub'] + f['n_ins'] + f['n_del']}" == f"NM:i:{use('XID')}" and c[12] == f"AS:i:{f['score']}"
        assert c[1] == "0" and c[4] == "255" and c[10] == "*" and c[2] in names
        clipped += use("S") > 0
    assert clipped >= 10                                                                         # flanks outside [qstart, qend) reach the CIGAR
    # the product's writer gives the restatement's line
    rec_ops, _ = ref.aligned([seqs[0][5:60].encode()], [seqs[0][5:30].encode() + b"G" + seqs[0][31:60].encode()])
    sites, prof, out = ref.pileup(rec_ops, [seqs[0][5:60].encode()], [seqs[0][5:30].encode() + b"G" + seqs[0][31:60].encode()], [5], 900)
    read = "ac" + seqs[0][5:30] + "G" + seqs[0][31:60] + "u"
    assert cli.sam_line("r", read, names[0], 5, 2, len(read) - 1, rec_ops[0], out[0]) == ref.sam_rows(names, seqs, [("r", read, 0, 5, 2, len(read) - 1, rec_ops[0], out[0])])[-1] + "\n"
    assert "".join(cli.profile_lines(prof)) == "".join(r + "\n" for r in ref.profile_rows(prof))


def test_planted_site_is_the_only_substitution_variant(cli_expected):
    """the condition the command-line test on the GPU relies on, shown by the restatement alone"""
    names, seqs, reads, paf, alt, exp = cli_expected
    rows = [l.split("\t") for l in exp["variants"].splitlines()[1:]]
    t, pos = pc.PLANTED
    subs = [r for r in rows if r[3] == "sub"]
    assert subs and [(r[0], int(r[1]), r[2], r[4]) for r in subs] == [(names[t], pos, seqs[t][pos], alt)]
    assert 0.6 <= float(subs[0][6]) <= 0.95 and int(subs[0][5]) >= 30
    assert 100 <= len(reads) <= 130 and len(exp["profile"].splitlines()) == 1 + 30 + 5 + 4096 + 128
    conf = exp["profile"].splitlines()[1:31]
    total = sum(int(l.split("\t")[2]) for l in conf)
    diag = sum(int(l.split("\t")[2]) for l in conf if l.split("\t")[1][0] == l.split("\t")[1][2])
    assert 0.03 < 1 - diag / total < 0.12                                                        # errors at about 8 %


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_pileup_host(tmp_path):
    """tests/asan_pileup.cpp: the host side of pileup.hip (argument checks, the op validator, the rules, the host twin) built with
    AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_pileup"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_pileup.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 300 and int(last[2]) >= 3000          # "<n> accepted <m> refused"
