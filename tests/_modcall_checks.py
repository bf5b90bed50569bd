"""TEST INFRASTRUCTURE: the checks that tests/test_modcall_cpu.py runs on the host twins and tests/test_gpu_modcall.py on the GPU: vit_ref
against the cost of an alignment's own path, the accuracy chain's bounds, and the `eventalign --call` command against the restatement's
composition."""
import numpy as np

import _eventalign_cases as sc
import _modcall_cases as mc
import _modcall_e2e as e2e
import _modcall_ref as ref


def identity_reads():
    """reads of the k = 3 model aligned by rd_eventalign_host on a given scale, a job at every third base"""
    rng = np.random.default_rng(320)
    raws, seqs = [], []
    for L, T in ((40, 400), (75, 700), (9, 60)):
        codes = rng.integers(0, 4, L).astype(np.uint8)
        raws.append(sc.signal(rng, codes, T, 20, 15))
        seqs.append(codes)
    return raws, seqs


def check_against_path(firsts, lasts, raws, seqs, res_of, exact):
    """vit_ref of a job at every third base against the summed cell cost of the path the steps describe, where every base of the window has
    rows: equal (exact) or at most that -> (the result, the jobs strictly below the sum)"""
    m, F = mc.GROUPS["k3"]
    job_read = [r for r in range(len(raws)) for _ in range(0, len(seqs[r]), 3)]
    alt_first = [b for r in range(len(raws)) for b in range(0, len(seqs[r]), 3)]
    alts = [(np.array([mc.shifted(m, seqs[r], b)[0]], np.int32), np.array([mc.shifted(m, seqs[r], b)[1]], np.uint64).astype(np.uint32),
             np.array([mc.shifted(m, seqs[r], b)[2]], np.int32)) for r, b in zip(job_read, alt_first)]
    res = res_of(raws, seqs, [2 * sc.MEDIAN] * len(raws), [sc.D4] * len(raws), firsts, lasts, mc.backend_model("k3"), job_read, alt_first, alts, flank=F)
    n_ok = n_strict = 0
    for j, (r, b) in enumerate(zip(job_read, alt_first)):
        L = len(seqs[r])
        a0, a1 = max(0, b - F), min(L - 1, b + F)
        if int(res.status[j]) != ref.OK or any(int(firsts[r][a]) < 0 or int(lasts[r][a]) < int(firsts[r][a]) for a in range(a0, a1 + 1)):
            continue
        total = ref.path_cost(raws[r], seqs[r], 2 * sc.MEDIAN, sc.D4, firsts[r], lasts[r], m, a0, a1)
        assert int(res.vit_ref[j]) == total if exact else int(res.vit_ref[j]) <= total, (j, r, b, int(res.vit_ref[j]), total)
        n_ok += 1
        n_strict += int(res.vit_ref[j]) < total
    assert n_ok >= 20
    return res, n_strict


def check_accuracy(tmp_path, kind):
    """the chain of tests/_modcall_e2e.py at the clean or the smeared sites (shared with the GPU test); prints what it measured"""
    sites, alpha = (e2e.CLEAN_SITES, 0.05) if kind == "clean" else (e2e.SMEARED_SITES, 1.0)
    got = e2e.accuracy_chain(str(tmp_path), sites, alpha)
    print(kind, "per site (jobs, not ok, wrong calls, wrong clusters, clustered reads):", got)
    m = e2e.MEASURED[kind]
    for i, (jobs, not_ok, wrong_call, wrong_cluster, clustered) in enumerate(got):
        assert jobs >= 50 and 20 * not_ok <= jobs, (sites[i], "more than 5 % of the jobs are not ok: the test proves nothing")
        assert clustered == jobs, (sites[i], "compare --split wrote no cluster for some of the reads")
        if kind == "clean":     # the reference is compare --split on the same run, one read the margin
            assert wrong_call <= wrong_cluster + e2e.WRONG_READS, (sites[i], wrong_call, wrong_cluster)
        else:
            assert wrong_call <= m["wrong_call"][i] + e2e.WRONG_READS and wrong_call <= wrong_cluster, (sites[i], wrong_call, wrong_cluster)
            assert wrong_cluster <= m["wrong_cluster"][i] + e2e.WRONG_READS, (sites[i], wrong_cluster)
    return got


CALL_ONLY = (("t1", 5), ("t9", 3))      # a site hardly a fragment reaches, and a transcript no read maps to


def simulate_for_command(tmp_path):
    return e2e.simulate_pair(str(tmp_path), e2e.CLEAN_SITES, reads=24, call_only=CALL_ONLY)


def check_command(tmp_path, log, variants, extra=(), prefix="", sim=None):
    """`eventalign --call` on 24 simulated reads: calls.tsv is the restatement's composition on what modcall was asked, row for row and in
    the contract's order; every file is the same bytes under every variant of --batch-reads / --budget-bytes"""
    from radian_amd import eventalign
    tmp = str(tmp_path)
    sites = e2e.CLEAN_SITES + CALL_ONLY
    dirs, sites_file = sim or simulate_for_command(tmp_path)
    del log[:]
    ev, files, text = e2e.call_command(tmp, dirs, sites_file, "a", prefix + "base", extra)
    rows = [ln.split("\t") for ln in files["calls"].decode().splitlines()]
    composed = e2e.composed_rows(log)
    keys = e2e.expected_keys(dirs["a"][0], ev, sites)
    assert rows[0] == list(eventalign.CALL_COLUMNS)
    assert len(rows) - 1 == len(composed) == len(keys) >= 30
    for row, key, tail in zip(rows[1:], keys, composed):
        assert tuple(row) == key + tail
    n_ok = sum(r[4] == "ok" for r in rows[1:])
    assert f"calls: {len(keys)} jobs over {len(sites)} sites; ok: {n_ok};" in text and "transcripts no read maps to: t9" in text
    assert "reads without a PAF line: 0 of 24" in text
    site_rows = [ln.split("\t") for ln in files["callsites"].decode().splitlines()]
    assert [r[:2] for r in site_rows[1:]] == [[n, str(p)] for n, p in sites] and site_rows[-1][2:] == ["-", "0", "0", "0", "nan", "nan"]
    for (name, pos), r in zip(sites, site_rows[1:]):
        mine = [row for row in rows[1:] if (row[1], row[2]) == (name, str(pos))]
        ok = [row for row in mine if row[4] == "ok"]
        assert [int(r[3]), int(r[4]), int(r[5])] == [len(mine), len(ok), sum(row[12] == "1" for row in ok)]
        if ok:
            assert r[7] == f"{sum(int(row[9]) - int(row[10]) for row in ok) / (32.0 * len(ok)):.6f}"
    for tag, more in variants:
        _, again, _ = e2e.call_command(tmp, dirs, sites_file, "a", prefix + tag, list(extra) + list(more))
        assert again == files, tag
    return dirs, files, text
