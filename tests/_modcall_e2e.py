"""TEST INFRASTRUCTURE: the chain simulate -> eventalign --call -> compare --split --reads-out on tests/_sitesplit_e2e.py's two samples,
shared by tests/test_modcall_cpu.py (on the host twins) and tests/test_gpu_modcall.py (on the GPU, which equals the twins bit for bit).
Sample A is simulated with --modify at the given sites (half of the reads, the level moved by 1.0 z) and --mods-out, sample B without.
`eventalign --call` takes A's --modify file as its sites file, for either sample; truth is --mods-out for A and "unmodified" for B.

Two pairs: the three CLEAN sites of _sitesplit_e2e.MOD_SITES, and the two SMEARED sites that file names, t0:262 and t1:201, where the moved
level comes close to a neighbour's and the Viterbi path gives the neighbour the samples.

Also: a Backend on the host twins that has modcall, a recorder of modcall's calls, and the composition of calls.tsv from the restatement."""
import contextlib
import io
import os

import _modcall_ref as ref
import _sitesplit_e2e as e2e

CLEAN_SITES = e2e.MOD_SITES
SMEARED_SITES = (("t0", 262), ("t1", 201))
# measured on the host twins (tests/test_modcall_cpu.py prints them): per site, the reads of both samples whose `call` at the default
# threshold is not the truth, and those whose `compare --split` cluster (--alpha 1 at the smeared sites) is not
MEASURED = {
    "clean": {"jobs": (59, 59, 69), "wrong_call": (0, 0, 0), "wrong_cluster": (0, 0, 0)},
    "smeared": {"jobs": (63, 65), "wrong_call": (1, 0), "wrong_cluster": (57, 13)},
}
WRONG_READS = 1     # the floor: the measured value and one read per site


class CallHostBackend(e2e.HostBackend):
    """_sitesplit_e2e's Backend on the host twins, with modcall"""

    def modcall(self, *a, budget_bytes=0, allow_too_large=False, **kw):
        from radian_amd.backend import modcall_host
        return modcall_host(*a, **kw)


def recording(cls, log):
    """cls with a modcall that appends (positional arguments, flank, result) to log"""
    class Recording(cls):
        def modcall(self, *a, **kw):
            res = super().modcall(*a, **kw)
            log.append((a, kw["flank"], res))
            return res
    return Recording


def on_the_host(monkeypatch, log=None):
    from radian_amd import compare, eventalign, simulate
    cls = CallHostBackend if log is None else recording(CallHostBackend, log)
    for mod in (compare, eventalign, simulate):
        monkeypatch.setattr(mod, "Backend", cls)


def simulate_pair(tmp, sites, reads=e2e.READS, call_only=()):
    """both samples' fast5 and truth -> {"a": (sim dir, fast5 dir), "b": ...}, the sites file of --call: sample A's --modify file, and
    behind its rows those of the sites in call_only, which nothing is modified at"""
    from radian_amd import simulate
    fa, _ = e2e.write_inputs(tmp)
    mod, call = os.path.join(tmp, "modify_sites.tsv"), os.path.join(tmp, "sites.tsv")
    for path, rows in ((mod, sites), (call, tuple(sites) + tuple(call_only))):
        with open(path, "w") as f:
            for name, pos in rows:
                f.write(f"{name}\t{pos}\t{e2e.SHIFT}\t1.0\t{e2e.FRACTION}\n")
    dirs = {}
    for name, seed, more in (("a", 11, ["--modify", mod, "--mods-out", os.path.join(tmp, "mods_a.tsv")]), ("b", 12, [])):
        sim, f5 = os.path.join(tmp, f"sim_{name}"), os.path.join(tmp, f"fast5_{name}")
        with contextlib.redirect_stdout(io.StringIO()):
            simulate.main([fa, "-o", sim, "--reads", str(reads), "--seed", str(seed), "--length-median", "250", "--length-sigma", "0.15", "--min-length",
                           "200", "--tail", "60", "--model-seed", "7"] + more)
        os.makedirs(f5)
        for f in sorted(os.listdir(sim)):
            if f.endswith(".fast5"):
                os.rename(os.path.join(sim, f), os.path.join(f5, f))
        dirs[name] = (sim, f5)
    return dirs, call


def call_command(tmp, dirs, sites_file, sample, tag, extra=()):
    """eventalign --call on one sample -> (events dir, {file: bytes} of calls, call sites, summary and every events file, the printed text)"""
    from radian_amd import eventalign
    sim, f5 = dirs[sample]
    ev = os.path.join(tmp, f"events_{sample}_{tag}")
    paths = {k: os.path.join(tmp, f"{k}_{sample}_{tag}.tsv") for k in ("calls", "callsites", "summary")}
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        eventalign.main([f5, os.path.join(sim, "read_ref.tsv"), "--model-seed", "7", "--bounds", os.path.join(sim, "truth.tsv"), "-o", ev, "--summary",
                         paths["summary"], "--call", sites_file, "--paf", os.path.join(sim, "truth.paf"), "--calls-out", paths["calls"], "--call-sites-out",
                         paths["callsites"]] + list(extra))
    files = {k: open(p, "rb").read() for k, p in paths.items()}
    files.update({f: open(os.path.join(ev, f), "rb").read() for f in sorted(os.listdir(ev))})
    return ev, files, text.getvalue()


def accuracy_chain(tmp, sites, alpha):
    """-> per site (jobs, jobs that are not ok, reads whose call is wrong, reads whose compare --split cluster is wrong, reads compare clustered)"""
    from radian_amd import compare
    dirs, sites_file = simulate_pair(tmp, sites)
    ev, calls = {}, {}
    for s in "ab":
        ev[s], files, _ = call_command(tmp, dirs, sites_file, s, "acc")
        calls[s] = files["calls"].decode()
    out_sites, out_reads = os.path.join(tmp, "cmp_sites.tsv"), os.path.join(tmp, "cmp_reads.tsv")
    with contextlib.redirect_stdout(io.StringIO()):
        compare.main(["--a", ev["a"], "--a-paf", os.path.join(dirs["a"][0], "truth.paf"), "--b", ev["b"], "--b-paf", os.path.join(dirs["b"][0], "truth.paf"),
                      "-o", out_sites, "--split", "--split-min-frac", str(e2e.MIN_FRAC), "--reads-out", out_reads, "--alpha", str(alpha)])
    truth = {}
    for ln in open(os.path.join(tmp, "mods_a.tsv")).read().splitlines()[1:]:
        rid, name, pos, hit = ln.split("\t")
        truth[(rid, name, int(pos))] = int(hit)
    want = lambda sample, rid, name, pos: truth[(rid, name, pos)] if sample == "a" else 0
    res = {s: [0, 0, 0, 0, 0] for s in sites}
    for sample in "ab":
        for ln in calls[sample].splitlines()[1:]:
            c = ln.split("\t")
            r = res[(c[1], int(c[2]))]
            r[0] += 1
            if c[4] != "ok":
                r[1] += 1
            else:
                r[2] += int(c[12]) != want(sample, c[0], c[1], int(c[2]))
    for ln in open(out_reads).read().splitlines()[1:]:
        rid, sample, name, pos, ch, _, cluster = ln.split("\t")
        if ch == "level" and (name, int(pos)) in res:
            res[(name, int(pos))][3] += int(cluster) != want(sample, rid, name, int(pos))
            res[(name, int(pos))][4] += 1
    return [tuple(res[s]) for s in sites]


def composed_rows(log, threshold=0.0):
    """the nine columns from status on of every job modcall was asked, in the order asked, from the restatement (tests/_modcall_ref.py) on
    the recorded inputs; also asserts that what modcall answered is what the restatement says"""
    from _eventalign_ref import Model
    rows = []
    for (raws, seqs, m2, d4, firsts, lasts, model, job_read, alt_first, alts), flank, res in log:
        m = Model(model.k, model.lvl.tolist(), model.w.tolist(), model.bias.tolist(), model.bg)
        for j, (r, a, e) in enumerate(zip(job_read, alt_first, alts)):
            entries = [(int(e[0][i]), int(e[1][i]), int(e[2][i])) for i in range(len(e[0]))]
            o = ref.job_numpy(raws[r], seqs[r], int(m2[r]), int(d4[r]), firsts[r], lasts[r], m, int(a), entries, flank)
            ref.assert_job_equal(res, j, o, "the command's job")
            if o["status"] != ref.OK:
                rows.append((ref.STATUS_NAMES[o["status"]],) + ("-",) * 8)
                continue
            num = o["fwd_ref"] - o["fwd_alt"]
            rows.append(("ok", str(o["n_states"]), str(o["n_rows"]), str(o["vit_ref"]), str(o["vit_alt"]), str(o["fwd_ref"]), str(o["fwd_alt"]),
                         f"{num / 32:.5f}", "1" if num > 32 * threshold else "0"))
    return rows


def expected_keys(sim_dir, events_dir, sites):
    """(read_id, ref_name, pos, base) of every row calls.tsv must hold: the reads in input order (the order of their first event rows), then
    the sites file's order, a site making a row where the read's span covers it"""
    spans = {}
    for ln in open(os.path.join(sim_dir, "read_ref.tsv")).read().splitlines()[1:]:
        rid, _, seq = ln.split("\t")
        spans[rid] = seq
    paf = {}
    for ln in open(os.path.join(sim_dir, "truth.paf")).read().splitlines():
        c = ln.split("\t")
        paf[c[0]] = (c[5], int(c[7]))
    order = []
    for f in sorted(os.listdir(events_dir)):
        if f.endswith(".events.tsv"):
            for ln in open(os.path.join(events_dir, f)).read().splitlines()[1:]:
                rid = ln.split("\t", 1)[0]
                if not order or order[-1] != rid:
                    order.append(rid)
    assert len(set(order)) == len(order)
    keys = []
    for rid in order:
        tname, start = paf[rid]
        for name, pos in sites:
            if name == tname and 0 <= pos - start < len(spans[rid]):
                keys.append((rid, name, str(pos), spans[rid][pos - start].upper().replace("U", "T")))
    return keys
