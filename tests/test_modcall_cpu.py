"""rd_modcall without a GPU (include/radian_hip.h): the LSE literal, the restatements against each other and against
hand-worked toys, rd_modcall_host against the restatement on every seeded case, the identity with rd_eventalign's path, the two
inequalities, the refusals, the workspace formula, the host code under the sanitizers, and the `eventalign --call` command on the host
twins."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _eventalign_cases as sc
import _eventalign_ref as fref
import _modcall_cases as mc
import _modcall_checks as chk
import _modcall_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def backend():
    from radian_amd import backend as b
    return b


def host_results(group, order=None):
    """rd_modcall_host on a group's cases as one batch -> {(case, job): dict of the fields}"""
    cases = mc.groups()[group]
    kw, flat = mc.call_args(cases, order)
    res = backend().modcall_host(model=mc.backend_model(group), flank=mc.GROUPS[group][1], **kw)
    return {key: {f: int(getattr(res, f)[j]) for f in ref.FIELDS} for j, key in enumerate(flat)}


# ---------------------------------------------------------------------------------------------- the table
def test_lse_literal_against_mpmath():
    """LSE[d] = floor(32 ln(1 + e^(-d/32)) + 1/2) at 50 digits: the header's literal, the restatement's list, and no entry within 1e-6 of
    a rounding tie; 134 entries, LSE[0] = 22, LSE[133] = 0 and the next one would be 0 too"""
    import mpmath as mp
    mp.mp.dps = 50
    text = open(os.path.join(ROOT, "radian_amd", "csrc", "modcall_rules.h")).read()
    body = re.search(r"#define MC_LSE_LITERAL(.*?)\nconstexpr", text, re.S).group(1)
    literal = [int(v) for v in re.findall(r"\d+", body.replace("\\", " "))]
    want = []
    for d in range(135):
        v = 32 * mp.log(1 + mp.exp(-mp.mpf(d) / 32)) + mp.mpf(1) / 2
        assert abs(v - mp.nint(v)) > mp.mpf(10) ** -6, d
        want.append(int(mp.floor(v)))
    assert literal == want[:134] == ref.LSE and len(literal) == 134
    assert want[0] == 22 and want[132] == 1 and want[133] == 0 and want[134] == 0


# ---------------------------------------------------------------------------------------------- the restatement
def test_toys_by_hand():
    """two states, three rows, a model whose cells cost their bias alone"""
    m = fref.Model(1, [0] * 4, [0] * 4, [10, 40, -7, 0], (0, 0, 0))
    raw = np.array([1, 2, 3], np.int16)
    # states A (10) then C (40); rows 0..2.  Row 0: (10, inf).  Row 1: (20, 50).  Row 2, state 1: 40 + min(50, 20) = 60;
    # fwd: 40 + 20 - LSE[30] = 60 - 11
    o = ref.job_plain(raw, [0, 1], 1200, 240, [0, 1], [0, 2], m, 1, [(0, 0, -7)], 1)
    assert o == dict(status=0, n_rows=3, n_states=2, vit_ref=60, fwd_ref=60 - ref.LSE[30], vit_alt=-7 + min(3, 20), fwd_alt=-7 + 3 - ref.LSE[17])
    assert ref.LSE[30] == 11 and ref.LSE[17] == 15
    # one state, two rows: no path to sum over
    o = ref.job_plain(raw, [2], 1200, 240, [1], [2], m, 0, [(0, 0, 5)], 0)
    assert o == dict(status=0, n_rows=2, n_states=1, vit_ref=-14, fwd_ref=-14, vit_alt=10, fwd_alt=10)
    # a real cell: zq = floor((2 * 512 * (2 * 660 - 1200) + 240) / 480) = 256; d = 256 - 100; w = 2^32 / 64: floor(156^2 / 64) = 380
    m2 = fref.Model(1, [100] * 4, [1 << 26] * 4, [3] * 4, (0, 0, 0))
    o = ref.job_plain(np.array([660], np.int16), [0], 1200, 240, [0], [0], m2, 0, [(256, 1 << 26, -3)], 0)
    assert (o["vit_ref"], o["vit_alt"]) == (383, -3) == (o["fwd_ref"], o["fwd_alt"])


def test_cases_meet_their_conditions_and_twin_equals_plain():
    n_small = 0
    for c in mc.all_cases():
        outs = mc.reference(c)
        assert c["cond"](outs), (c["name"], outs)
        if mc.is_small(c):
            assert mc.plain(c) == outs, c["name"]
            n_small += 1
    assert n_small >= 30
    rows = {o["n_rows"] for c in mc.all_cases() for o in mc.reference(c)}
    states = {o["n_states"] for c in mc.all_cases() for o in mc.reference(c)}
    assert {13, 14, 63, 64, 65, 127, 128, 129, 1000, 1 << 15} <= rows and {1, 2, 21, 62, 63} <= states
    assert {o["status"] for c in mc.all_cases() for o in mc.reference(c)} == {ref.OK, ref.NO_ANCHOR, ref.NO_PATH, ref.TOO_LONG}


def test_inequalities_and_alt_equal_ref():
    """fwd <= vit <= fwd + 22 (R - 1) for both hypotheses of every OK job; the bounds of the contract"""
    for c in mc.all_cases():
        for o in mc.reference(c):
            if o["status"] != ref.OK:
                assert all(o[f] == 0 for f in ref.FIELDS[1:])
                continue
            for h in ("ref", "alt"):
                assert o["fwd_" + h] <= o["vit_" + h] <= o["fwd_" + h] + 22 * (o["n_rows"] - 1), (c["name"], o)
                assert -(1 << 15) * 278 < o["fwd_" + h] and o["vit_" + h] <= (1 << 15) * 1280 < 3 << 28


# ---------------------------------------------------------------------------------------------- the host twin
@pytest.mark.parametrize("group", sorted(mc.GROUPS))
def test_host_equals_restatement(group):
    cases = mc.groups()[group]
    got = host_results(group)
    assert len(got) == sum(len(c["jobs"]) for c in cases)
    for (ci, ji), o in got.items():
        assert o == mc.reference(cases[ci])[ji], (cases[ci]["name"], ji)


def test_host_does_not_depend_on_the_order_of_jobs():
    n = sum(len(c["jobs"]) for c in mc.groups()["k3"])
    order = np.random.default_rng(5).permutation(n)
    assert host_results("k3", order) == host_results("k3")


def test_vit_ref_is_the_cost_of_eventaligns_path():
    """first / last from rd_eventalign_host on the same scale: vit_ref equals the summed cell cost of that path over the window's rows; from
    rd_eventalign_events_host's steps (events of three samples, no skips) it is at most that sum"""
    b = backend()
    raws, seqs = chk.identity_reads()
    model = mc.backend_model("k3")
    n = len(raws)
    ea = b.eventalign_host(raws, seqs, model, m2=[2 * sc.MEDIAN] * n, d4=[sc.D4] * n)
    assert (ea.status == 0).all()
    chk.check_against_path(ea.first_step, ea.last_step, raws, seqs, b.modcall_host, exact=True)
    events = []
    for x in raws:
        x = x.astype(np.int64)
        start = np.arange(0, len(x), 3, dtype=np.int32)
        events.append(dict(start=start, sum=np.add.reduceat(x, start), sumsq=np.add.reduceat(x * x, start),
                           min=np.minimum.reduceat(x, start).astype(np.int16), max=np.maximum.reduceat(x, start).astype(np.int16)))
    ev = b.eventalign_events_host(events, [len(x) for x in raws], seqs, model, [2 * sc.MEDIAN] * n, [sc.D4] * n, skip_pen=-1)
    assert (ev.status[:2] == 0).all()
    ok = [r for r in range(n) if int(ev.status[r]) == 0]
    firsts = [ev.events.start[r] for r in ok]
    lasts = [ev.events.end[r] - 1 for r in ok]
    _, n_strict = chk.check_against_path(firsts, lasts, [raws[r] for r in ok], [seqs[r] for r in ok], b.modcall_host, exact=False)
    assert n_strict >= 1      # the event path is not the sample rows' best one everywhere: "at most" is not "equal"


# ---------------------------------------------------------------------------------------------- the refusals
def test_refusals():
    b = backend()
    cases = [c for c in mc.groups()["k3"] if c["name"] in ("anchors", "short")]
    kw, _ = mc.call_args(cases)
    model = mc.backend_model("k3")
    assert len(b.modcall_host(model=model, flank=6, **kw).status) == 8

    def refused(**change):
        with pytest.raises(b.RadianHipError):
            b.modcall_host(model=model, **{**kw, "flank": 6, **change})

    refused(flank=-1)
    refused(flank=28)
    refused(d4=[0, 240])
    refused(d4=[240, (1 << 20) + 1])
    refused(m2=[(1 << 17) + 1, 1200])
    refused(job_read=[2] + kw["job_read"][1:])
    refused(job_read=[-1] + kw["job_read"][1:])
    refused(alt_first=[-1] + kw["alt_first"][1:])
    refused(alt_first=[30] + kw["alt_first"][1:])          # alt_first + n_alt > L = 30
    one = kw["alts"][0]
    ten = tuple(np.repeat(a, 10) for a in one)
    refused(alts=[ten] + kw["alts"][1:], alt_first=[0] + kw["alt_first"][1:])
    refused(alts=[tuple(a[:0] for a in one)] + kw["alts"][1:])
    refused(alts=[(np.array([1 << 14], np.int32), one[1], one[2])] + kw["alts"][1:])
    refused(alts=[(one[0], one[1], np.array([257], np.int32))] + kw["alts"][1:])
    refused(seqs=[np.full(30, 4, np.uint8), kw["seqs"][1]])
    bad = b.EvalModel(3, np.full(64, 1 << 14), np.zeros(64), np.zeros(64), (0, 0, 0))
    with pytest.raises(b.RadianHipError):
        b.modcall_host(model=bad, flank=6, **kw)
    # no jobs, and no reads: fine
    none = b.modcall_host(kw["raws"], kw["seqs"], kw["m2"], kw["d4"], kw["firsts"], kw["lasts"], model, [], [], [], flank=6)
    assert len(none.status) == 0
    assert len(b.modcall_host([], [], [], [], [], [], model, [], [], [], flank=0).status) == 0


def test_workspace_formula():
    b = backend()
    up = lambda v: (v + 255) // 256 * 256
    for n, L, nj, na in ((0, 0, 0, 0), (1, 1, 1, 1), (1000, 30, 4, 4), (1000, 30, 5, 45), (1 << 20, 4000, 1000, 9000), (127, 31, 8, 9), (129, 33, 9, 21)):
        assert b.modcall_workspace_bytes(n, L, nj, na) == up(2 * n) + up(8 * L) + up(64 * nj) + up(32 * nj) + up(12 * na)
    assert b.modcall_workspace_bytes(-1, 0, 0, 0) == -1 and b.modcall_workspace_bytes(0, 0, 0, -1) == -1


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_modcall_host(tmp_path):
    """tests/asan_modcall.cpp: the host side of rd_modcall (argument checks, the rules, the host twin) built with AddressSanitizer + UBSan
    as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_modcall"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_modcall.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 300 and int(last[2]) >= 3000


# ---------------------------------------------------------------------------------------------- the command on the host twins
@pytest.mark.parametrize("kind", ["clean", "smeared"])
def test_accuracy_on_the_host_twins(tmp_path, monkeypatch, kind):
    """at the three clean sites `call` is wrong on at most one read more than compare --split's cluster (which is wrong on none); at the two
    smeared sites the measured counts are recorded in _modcall_e2e.MEASURED and `call` is wrong on no more reads than the cluster"""
    import _modcall_e2e as e2e
    e2e.on_the_host(monkeypatch)
    got = chk.check_accuracy(tmp_path, kind)
    m = e2e.MEASURED[kind]      # on the host twins the figures are the recorded ones exactly
    assert tuple(g[0] for g in got) == m["jobs"] and tuple(g[2] for g in got) == m["wrong_call"] and tuple(g[3] for g in got) == m["wrong_cluster"]


def test_command_on_the_host_twins(tmp_path, monkeypatch):
    """calls.tsv equals the restatement's composition; a run without --call writes and prints the bytes a run with --call does, less the
    calls; a read the PAF lacks is counted; the refusals of the options"""
    import _modcall_e2e as e2e
    from radian_amd import eventalign
    log = []
    e2e.on_the_host(monkeypatch, log)
    dirs, files, text = chk.check_command(tmp_path, log, (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7"])))
    sim, f5 = dirs["a"]
    import contextlib
    import io
    plain, summ = str(tmp_path / "plain"), str(tmp_path / "plain_summary.tsv")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eventalign.main([f5, os.path.join(sim, "read_ref.tsv"), "--model-seed", "7", "--bounds", os.path.join(sim, "truth.tsv"), "-o", plain, "--summary", summ])
    assert out.getvalue() == "".join(ln + "\n" for ln in text.splitlines() if not ln.startswith("calls:")) and "calls" not in out.getvalue()
    assert open(summ, "rb").read() == files["summary"]
    assert sorted(os.listdir(plain)) == sorted(f for f in files if f.endswith(".events.tsv"))
    for f in os.listdir(plain):
        assert open(os.path.join(plain, f), "rb").read() == files[f]
    # a PAF without the first read
    paf = os.path.join(sim, "truth.paf")
    lines = open(paf).read().splitlines(True)
    short = str(tmp_path / "short.paf")
    open(short, "w").write("".join(lines[1:]))
    first = lines[0].split("\t")[0]
    base = [f5, os.path.join(sim, "read_ref.tsv"), "--model-seed", "7", "--bounds", os.path.join(sim, "truth.tsv"), "-o", str(tmp_path / "x")]
    calls = str(tmp_path / "calls_short.tsv")
    with contextlib.redirect_stdout(out):
        eventalign.main(base + ["--call", str(tmp_path / "sites.tsv"), "--paf", short, "--calls-out", calls])
    assert "reads without a PAF line: 1 of 24" in out.getvalue()
    assert open(calls).read() == "".join(ln for ln in files["calls"].decode().splitlines(True) if not ln.startswith(first + "\t"))
    # refusals
    noshift = str(tmp_path / "noshift.tsv")
    open(noshift, "w").write("t0\t207\n")
    for more in (["--call", noshift, "--paf", paf, "--calls-out", calls], ["--paf", paf], ["--call", noshift, "--calls-out", calls],
                 ["--call", noshift, "--paf", paf, "--calls-out", calls, "--call-flank", "28"]):
        with pytest.raises(SystemExit):
            eventalign.main(base + more)
    # an alt table: one M per k-mer or refused; an entry it holds moves the site's k-mers, the others are kept and counted
    alt = str(tmp_path / "alt.tsv")
    head = "kmer\tn_events\tlevel_mean\tlevel_sd\tdwell_mean\n"
    open(alt, "w").write(head + "AMMCG\t1\t0.5\t0.2\t10\n")
    with pytest.raises(SystemExit):
        eventalign.main(base + ["--call", noshift, "--paf", paf, "--calls-out", calls, "--alt-table", alt])
    open(alt, "w").write(head + "ACMCG\t1\t0.5\t0.2\t10\n")
    never = str(tmp_path / "never.tsv")
    with pytest.raises(SystemExit):      # t0:207 is G, not the --mod-base A: refused before a read is aligned or a file written
        eventalign.main(base[:-1] + [str(tmp_path / "never")] + ["--call", noshift, "--paf", paf, "--calls-out", never, "--alt-table", alt])
    assert not os.path.exists(never) and not os.listdir(tmp_path / "never")
    codes = e2e.e2e.transcripts()[0]
    kmer = "".join("ACGT"[c] for c in codes[205:210])
    assert kmer[2] == "G"
    open(alt, "w").write(head + f"{kmer[:2]}M{kmer[3:]}\t1\t1.5\t0.2\t10\n")
    del log[:]
    with contextlib.redirect_stdout(out):
        eventalign.main(base + ["--call", noshift, "--paf", paf, "--calls-out", calls, "--alt-table", alt, "--mod-base", "G"])
    rows = [ln.split("\t") for ln in open(calls).read().splitlines()[1:]]
    assert len(rows) >= 8 and [tuple(r[4:]) for r in rows] == e2e.composed_rows(log) and all(r[5] == "17" for r in rows if r[4] == "ok")
    assert f"alt entries kept canonical: {4 * len(rows)}" in out.getvalue()
    assert all(len(a[0]) == 5 for call in log for a in call[0][9])
    # M off the centre: the transcript's k-mer round position 206 holds the site at its fourth letter.  Pore order runs the other way, so
    # of the job's five entries (bases 209 down to 205) the fourth alone moves, to rint(2.5 * 1024 * 1.4826 / 4) = 949
    kmer = "".join("ACGT"[c] for c in codes[204:209])
    assert kmer[3] == "G"
    open(alt, "w").write(head + f"{kmer[:3]}M{kmer[4:]}\t1\t2.5\t0.2\t10\n")
    del log[:]
    with contextlib.redirect_stdout(out):
        eventalign.main(base + ["--call", noshift, "--paf", paf, "--calls-out", calls, "--alt-table", alt, "--mod-base", "G"])
    n_jobs = 0
    for (raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts), flank, res in log:
        for r, a, e in zip(job_read, alt_first, alts):
            canonical = [int(model.lvl[fref.kmer(seqs[r], a + j, 5)]) for j in range(5)]
            assert int(seqs[r][a + 2]) == 2 and [int(v) for v in e[0]] == canonical[:3] + [949] + canonical[4:] and canonical[3] != 949
            n_jobs += 1
    assert n_jobs == len(rows)
