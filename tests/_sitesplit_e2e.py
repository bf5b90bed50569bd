"""TEST INFRASTRUCTURE: the chain simulate -> eventalign --bounds truth.tsv -> compare --split --reads-out on two small samples, shared by
tests/test_sitesplit_cpu.py (on the host twins: rd_sim_signal_host, rd_eventalign_host, rd_site_compare_host, rd_site_split_host) and
tests/test_gpu_sitesplit.py (on the GPU, which equals the twins bit for bit).  Sample A is simulated with --modify at three sites (half of
the reads, the level moved by 1.0 z, the dwell untouched) and --mods-out, sample B without; the stand-in table of seed 7.

Depth: READS = 64 reads per sample over two transcripts of 300 and 320 bases, fragments of 200 bases and more anchored at the 3' end: every
read covers its transcript's sites.  At 24 reads per sample (about 12 per site and sample) the G-test of the best possible table, 6 + 6
against 0 + 12, gives p = 1.3e-3, and with some 600 tested sites no Benjamini-Hochberg q reaches 0.05: the depth is chosen so that the
host chain recovers the three sites (measured at 24 reads: split_q 0.026, 0.24 and 0.0010).

Sites: eventalign smears a modified base whose moved level comes close to a neighbour's: the Viterbi path gives the neighbour its samples
(measured at t0:262, level -0.38 z beside 0.44 z: the modified reads' events shrink to a median dwell of 7 samples against 26 and their
levels fall on the wrong side; t1:201 likewise).  The three sites here are ones whose level moved by SHIFT stays at least 2.5 z away from
the model levels of the two bases on either side (`level_margin`, asserted by the CPU test).

The floors are measured on the host twins and recorded here, each less one read per site (MEASURED below)."""
import io
import os
import types

import numpy as np

import _sitecmp_ref as cmp_ref
import _sitesplit_ref as ref

READS = 64
LENGTHS = (300, 320)
MOD_SITES = (("t0", 207), ("t0", 237), ("t1", 246))          # (transcript, 0-based position); every fragment of 200 bases covers them
SHIFT, FRACTION, MIN_FRAC, ALPHA = 1.0, 0.5, 0.1, 0.05

# measured on the host twins (tests/test_sitesplit_cpu.py prints them): per site of MOD_SITES, sample A's reads at the site, the reads
# --mods-out says are modified, the reads above the cut (frac_hi_a times the reads), and the reads of both samples whose cluster is not
# their `modified`
MEASURED = {"n_a": (28, 28, 36), "modified": (17, 12, 24), "above": (17, 12, 24), "wrong": (0, 0, 0), "split_q": (2.0e-6, 6.7e-4, 2.4e-8)}
# the floors: the measured value and one read per site
FRAC_TOLERANCE_READS = 1          # |frac_hi_a n_a - modified reads| <= measured (0) + 1 at every site
WRONG_READS = 1                   # reads of either sample in the wrong cluster <= measured (0) + 1 at every site


class HostBackend:
    """the commands' Backend on the host twins: what simulate, eventalign and compare call, no GPU and no budget"""

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def sim_lengths(self, *a, budget_bytes=0, **kw):
        from radian_amd.backend import sim_lengths_host
        return sim_lengths_host(*a, **kw)

    def sim_signal(self, *a, n_samples=None, budget_bytes=0, allow_too_large=False, **kw):
        from radian_amd.backend import sim_signal_host
        return sim_signal_host(*a, **kw)

    def eventalign(self, raws, seqs, model, budget_bytes=0, allow_too_large=False, **kw):
        from radian_amd.backend import eventalign_host
        return eventalign_host(raws, seqs, model, **kw)

    def site_compare(self, site, cond, value, n_sites, budget_bytes=0, capacity=None, allow_too_large=False):
        from radian_amd.backend import site_compare_host
        return site_compare_host(site, cond, value, n_sites, capacity)

    def site_split(self, site, cond, value, n_sites, min_frac_q16=0, budget_bytes=0, capacity=None, allow_too_large=False):
        from radian_amd.backend import site_split_host
        return site_split_host(site, cond, value, n_sites, min_frac_q16, capacity)


def on_the_host(monkeypatch):
    """put the host twins in the place of the three commands' Backend"""
    from radian_amd import compare, eventalign, simulate
    for mod in (compare, eventalign, simulate):
        monkeypatch.setattr(mod, "Backend", HostBackend)


def transcripts():
    """the two transcripts' codes (seed 7), as write_inputs writes them"""
    rng = np.random.default_rng(7)
    return [rng.integers(0, 4, n) for n in LENGTHS]


def level_margin(name, pos):
    """the least distance in z between the site's stand-in level moved by SHIFT and the levels of the two bases on either side"""
    from radian_amd import eventalign, simulate
    codes = transcripts()[int(name[1:])].astype(np.uint8)
    lv = (simulate.standin_tables(5, 7)[0] / 1024.0)[eventalign.kmer_indices(codes[::-1], 5)][::-1]
    return min(abs(lv[pos] + SHIFT - lv[q]) for q in (pos - 2, pos - 1, pos + 1, pos + 2))


def write_inputs(tmp):
    """the FASTA and sample A's --modify file"""
    fa = os.path.join(tmp, "tr.fa")
    with open(fa, "w") as f:
        for i, codes in enumerate(transcripts()):
            f.write(f">t{i}\n{''.join('ACGT'[c] for c in codes)}\n")
    mod = os.path.join(tmp, "modify.tsv")
    with open(mod, "w") as f:
        for name, pos in MOD_SITES:
            f.write(f"{name}\t{pos}\t{SHIFT}\t1.0\t{FRACTION}\n")
    return fa, mod


def run_chain(tmp, budgets=(0,), extra_simulate=()):
    """simulate and eventalign both samples, then compare --split --reads-out once per entry of budgets.  -> [(sites.tsv bytes, reads.tsv
    bytes, the summary's text) per entry] and the directories.  The commands' own Backend does the work (the CPU test puts the host twins in its place)."""
    import contextlib
    from radian_amd import compare, eventalign, simulate
    fa, mod = write_inputs(tmp)
    dirs = {}
    sink = io.StringIO()
    for name, seed, more in (("a", 11, ["--modify", mod, "--mods-out", os.path.join(tmp, "mods_a.tsv")]), ("b", 12, [])):
        sim, f5, ev = (os.path.join(tmp, f"{kind}_{name}") for kind in ("sim", "fast5", "events"))
        with contextlib.redirect_stdout(sink):
            simulate.main([fa, "-o", sim, "--reads", str(READS), "--seed", str(seed), "--length-median", "250", "--length-sigma", "0.15", "--min-length",
                           "200", "--tail", "60", "--model-seed", "7"] + more + list(extra_simulate))
            os.makedirs(f5)
            for f in sorted(os.listdir(sim)):
                if f.endswith(".fast5"):
                    os.rename(os.path.join(sim, f), os.path.join(f5, f))
            eventalign.main([f5, os.path.join(sim, "read_ref.tsv"), "--model-seed", "7", "--bounds", os.path.join(sim, "truth.tsv"), "-o", ev])
        dirs[name] = (sim, ev)
    outs = []
    for k, budget in enumerate(budgets):
        sites, reads = os.path.join(tmp, f"sites_{k}.tsv"), os.path.join(tmp, f"reads_{k}.tsv")
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            compare.main(["--a", dirs["a"][1], "--a-paf", os.path.join(dirs["a"][0], "truth.paf"), "--b", dirs["b"][1], "--b-paf",
                          os.path.join(dirs["b"][0], "truth.paf"), "-o", sites, "--split", "--split-min-frac", str(MIN_FRAC), "--reads-out", reads,
                          "--alpha", str(ALPHA), "--budget-bytes", str(budget)])
        outs.append((open(sites, "rb").read(), open(reads, "rb").read(), text.getvalue()))
    return outs, dirs


def expected_tables(dirs, tmp):
    """the two files as the command's own formulas write them from the restatements' integers (tests/_sitecmp_ref.py, _sitesplit_ref.py)"""
    from radian_amd import compare
    args = compare.build_parser().parse_args(["--a", dirs["a"][1], "--a-paf", os.path.join(dirs["a"][0], "truth.paf"), "--b", dirs["b"][1], "--b-paf",
                                              os.path.join(dirs["b"][0], "truth.paf"), "-o", "x", "--split", "--reads-out", "y"])
    names, offsets, n_sites, bases, site, cond, values, sample_st = compare.load(args)
    reads = sample_st.pop("reads")
    q16 = int(np.rint(MIN_FRAC * 65536))
    results = {ch: types.SimpleNamespace(**cmp_ref.as_arrays(cmp_ref.compare(site, cond, values[ch]))) for ch in compare.CHANNELS}
    splits = {ch: types.SimpleNamespace(**ref.as_arrays(ref.split(site, cond, values[ch], q16))) for ch in compare.CHANNELS}
    table, rows = io.StringIO(), io.StringIO()
    st = compare.write_table(table, names, offsets, bases, results, 10, ALPHA, splits)
    compare.write_reads(rows, names, offsets, reads, site, cond, values, list(compare.CHANNELS), st["split"])
    return table.getvalue(), rows.getvalue(), st


def recovery(sites_tsv, reads_tsv, mods_tsv):
    """per site of MOD_SITES: (level_split_q, sample A's reads, reads --mods-out calls modified, frac_hi_a times the reads, reads of either
    sample whose cluster differs from `modified`)"""
    rows = [ln.split("\t") for ln in sites_tsv.splitlines()]
    col = {c: i for i, c in enumerate(rows[0])}
    by = {(r[0], int(r[1])): r for r in rows[1:]}
    truth = {}
    for ln in mods_tsv.splitlines()[1:]:
        rid, name, pos, hit = ln.split("\t")
        truth[(rid, name, int(pos))] = int(hit)
    calls = {}
    for ln in reads_tsv.splitlines()[1:]:
        rid, sample, name, pos, ch, _, cluster = ln.split("\t")
        if ch == "level":
            calls.setdefault((name, int(pos)), []).append((rid, sample, int(cluster)))
    out = []
    for name, pos in MOD_SITES:
        r = by[(name, pos)]
        n_a = int(r[col["n_a"]])
        modified = sum(hit for (rid, nm, p), hit in truth.items() if (nm, p) == (name, pos))
        wrong = sum(cluster != (truth[(rid, name, pos)] if sample == "a" else 0) for rid, sample, cluster in calls.get((name, pos), []))
        out.append((float(r[col["level_split_q"]]), n_a, modified, float(r[col["level_frac_hi_a"]]) * n_a, wrong, len(calls.get((name, pos), []))))
    return out
