"""No-GPU checks of transcript quantification: every seeded case of tests/_quant_cases.py is what its name says
(asserted with the restatement, tests/_quant_ref.py), rd_quant_em_host equals the restatement on every case and under a permutation of
the reads, every refusal leaves the outputs untouched, the accuracy condition on the generator's four settings, and the host code of
quant.hip under AddressSanitizer + UBSan as a stand-alone program (tests/asan_quant.cpp).  Every comparison of integers is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _map_ref as mr
import _quant_cases as qc
import _quant_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in qc.em_cases():
        trace = []
        count, shares, iters, last = ref.em(c["reads"], c["n_tx"], c["max_iter"], c["tol_q20"], trace)
        out.append(dict(c, count=count, shares=shares, iters=iters, last=last, trace=trace))
    return out


def _host(reads, n_tx, max_iter, tol, with_share=True):
    from radian_amd.backend import quant_em_host
    return quant_em_host(*ref.csr(reads), n_tx, max_iter, tol, with_share=with_share)


def test_every_case_is_what_its_name_says(cases):
    for c in cases:
        assert c["cond"](c, c["trace"]), c["name"]
    by_name = {c["name"]: c for c in cases}
    assert max(s for _, s in by_name["the shift: 5000 single reads"]["trace"]) >= 1
    assert max(s for _, s in by_name["the shift: 140000 single reads"]["trace"]) >= 5
    assert by_name["a count that reaches 0"]["count"][1] == 0
    assert by_name["stops by tol before max_iter"]["last"] <= 4096 and by_name["stops by tol before max_iter"]["iters"] < 1000
    assert by_name["does not stop by tol"]["last"] > 0 and by_name["does not stop by tol"]["iters"] == 7


def test_host_twin_equals_the_restatement_on_every_case(cases):
    for c in cases:
        res = _host(c["reads"], c["n_tx"], c["max_iter"], c["tol_q20"])
        ref.assert_em_equal(res, c, "host twin")
        # the counts are the sums of the shares, and fewer units are lost than there are slots
        sums = [0] * c["n_tx"]
        for (t, _), s in zip([p for r in c["reads"] for p in r], res.share):
            sums[t] += int(s)
        assert sums == [int(v) for v in res.count], c["name"]
        assert 0 <= res.stats["lost"] < max(res.stats["slots"], 1), c["name"]
        # without the shares: the same counts
        assert np.array_equal(_host(c["reads"], c["n_tx"], c["max_iter"], c["tol_q20"], with_share=False).count, res.count), c["name"]


def test_permuting_the_reads_leaves_the_counts(cases):
    rng = np.random.default_rng(5)
    for c in cases:
        perm = rng.permutation(len(c["reads"]))
        res = _host([c["reads"][i] for i in perm], c["n_tx"], c["max_iter"], c["tol_q20"])
        assert [int(v) for v in res.count] == c["count"], c["name"]
        assert res.stats["iterations"] == c["iters"] and res.stats["last_delta"] == c["last"], c["name"]


def test_every_refusal_leaves_the_outputs_untouched():
    from radian_amd import _lib
    assert ref.check_refusals(_lib.load().rd_quant_em_host) >= 15


def test_workspace_bytes():
    from radian_amd.backend import quant_workspace_bytes
    assert quant_workspace_bytes(0, 0, 0) == 12 * 64 + 4096
    assert quant_workspace_bytes(1000, 10, 50) == 12 * (2000 + 64) + 24 * 50 + 4096
    assert quant_workspace_bytes(-1, 0, 0) == -1


# ---------------------------------------------------------------------------------------------- the accuracy condition
def accuracy_run(mode, seed, em_fn=None):
    """the generator's setting through the restatement's candidates (map defaults, min_frac_q10 = 922, K = 16, equal weights) and an EM
    (em_fn(reads, n_tx, max_iter, tol) -> counts; the restatement's by default) -> dict of the table's figures"""
    P = ref.ACCURACY_PARAMS
    transcripts, reads, truth, true = ref.accuracy_set(mode, seed)
    index = mr.build_index(transcripts, 14, 8)
    lengths = [len(t) for t in transcripts]
    cand = [ref.candidates(r, index, lengths, max_cand=P["max_cand"], min_frac_q10=P["min_frac_q10"], max_3p=P["max_3p"]) for r in reads]
    qreads = [[(row[0], 1) for row in c["rows"]] for c in cand]
    if em_fn is None:
        count, _, iters, last = ref.em(qreads, len(transcripts), P["max_iter"], P["tol_q20"])
    else:
        count, iters = em_fn(qreads, len(transcripts), P["max_iter"], P["tol_q20"])
    l1_hit, l1_em = ref.l1_errors(true, count, [c["rows"][0][0] for c in cand if c["rows"]])
    with_c = sum(1 for r in qreads if r)
    return dict(multi=sum(1 for c in cand if c["n_cand"] > 1), iters=iters, l1_hit=l1_hit, l1_em=l1_em, lost=with_c * ref.ONE - sum(count),
                qreads=qreads, count=count, n_tx=len(transcripts))


@pytest.mark.parametrize("mode,seed", ref.ACCURACY_SETTINGS)
def test_the_em_halves_the_best_hit_error(mode, seed):
    """The accuracy condition (a condition on the method): on each of the generator's settings the EM's L1 error against the true
    counts is at most half the L1 error of counting best hits.  The host twin gives the restatement's counts on the same candidates."""
    a = accuracy_run(mode, seed)
    print(f"{mode} seed {seed}: multi-candidate reads {a['multi']}, iterations {a['iters']}, L1 best-hit {a['l1_hit']}, L1 EM {a['l1_em']:.1f}, "
          f"lost units {a['lost']}")
    assert a["multi"] > 50
    assert 2 * a["l1_em"] <= a["l1_hit"], (a["l1_em"], a["l1_hit"])
    res = _host(a["qreads"], a["n_tx"], ref.ACCURACY_PARAMS["max_iter"], ref.ACCURACY_PARAMS["tol_q20"])
    assert [int(v) for v in res.count] == a["count"] and res.stats["iterations"] == a["iters"]


def test_candidate_cases_are_what_their_names_say():
    """70 copies: n_qual = 70 > K for K = 64, 2, 1 and the kept candidates are the smallest t; the edge set: a read whose only chain fails
    the 3' filter, d3 = 0, a negative d3, a read with several candidates"""
    transcripts, reads = qc.copies_case()
    index = mr.build_index(transcripts, 14, 8)
    for K in (64, 2, 1):
        c = ref.candidates(reads[0], index, [len(t) for t in transcripts], max_cand=K)
        assert c["n_qual"] == 70 and c["n_cand"] == K and [r[0] for r in c["rows"]] == list(range(K))
    transcripts, reads = qc.edge_case()
    index = mr.build_index(transcripts, 14, 8)
    lengths = [len(t) for t in transcripts]
    run = lambda **p: [ref.candidates(r, index, lengths, **p) for r in reads]
    off = run(max_3p=-1)
    assert off[0]["status"] == mr.OK and off[0]["n_qual"] == 1 and off[0]["rows"][0][7] > 50
    assert run(max_3p=50)[0]["status"] == mr.NO_CHAIN and run(max_3p=0)[0]["status"] == mr.NO_CHAIN
    assert off[1]["rows"][0][7] == 0 and run(max_3p=0)[1]["status"] == mr.OK
    assert off[2]["rows"][0][7] == -60
    assert off[3]["n_qual"] == 3 and off[6]["status"] == mr.NO_SEED
    assert any(c["n_qual"] > run(min_frac_q10=1024)[i]["n_qual"] for i, c in enumerate(run(min_frac_q10=0)))


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_quant_host(tmp_path):
    """tests/asan_quant.cpp: the host side of quant.hip (argument check, the rules, the packer, the host twin) built with AddressSanitizer
    + UBSan as a stand-alone executable, on exact-size heap buffers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_quant"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "radian_amd", "csrc", "quant.hip"),
                        os.path.join(ROOT, "tests", "asan_quant.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 200 and int(last[2]) >= 1000          # "<n> accepted <m> refused"
