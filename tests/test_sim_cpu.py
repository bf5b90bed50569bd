"""No-GPU checks of the signal simulation: Philox's known answers, rd_sim_*_host against the plain restatement of
the contract (tests/_sim_ref.py) on every seeded case (tests/_sim_cases.py) and every refusal, the moments of the noise and of the dwell,
the host side of radian_amd/simulate.py (the k-mer table loader, the truth files through the readers of the commands that take them, the
poly(A) search on simulated tails), and the host code of sim.hip under AddressSanitizer + UBSan as a stand-alone program
(tests/asan_sim.cpp).  Every comparison of integers is for equality."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _sim_cases as sc
import _sim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope="module")
def groups():
    gs = sc.all_groups()
    for g in gs:
        g["exp"] = sc.expect(g)
    return gs


class HostBackend:
    """radian_amd.simulate's backend on the host twins"""

    def sim_lengths(self, *a, budget_bytes=0, **kw):
        from radian_amd.backend import sim_lengths_host
        return sim_lengths_host(*a, **kw)

    def sim_signal(self, *a, n_samples=None, budget_bytes=0, allow_too_large=False, **kw):
        from radian_amd.backend import sim_signal_host
        return sim_signal_host(*a, **kw)


# ---------------------------------------------------------------------------------------------- the generator
def test_philox_known_answers_in_the_restatement_and_through_the_host_twin():
    """The three vectors in both forms of the restatement.  The C ABI reaches counters (i, 0 or 1, 0, 0) only, so through it: a model
    whose dwell is the cdf's index (dwell_q8 2^14 and cdf[i] = 1024 i give d = i) shows w0 >> 22 of counter 0 under key 0, 0x6627e8d5 >> 22
    = 408; the three vectors themselves are checked on sim_rules.h's function by tests/asan_sim.cpp."""
    from radian_amd.backend import SimModel, sim_lengths_host
    for counter, key, out in KNOWN:
        assert tuple(ref.philox_scalar(counter, key)) == out
        assert tuple(int(w[0]) for w in ref.philox(*counter, *key)) == out
    cdf = np.arange(1024) * 1024
    cdf[0] = 0
    m = SimModel(1, [0] * 4, [0] * 4, [1 << 14] * 4, cdf)
    assert 0x6627e8d5 >> 22 == 408
    assert sim_lengths_host([np.zeros(1, np.uint8)], m, 0, 0, 0, 0, 1024, np.zeros((1, 2), np.uint32)).tolist() == [408]
    # base 1 under another key: counter (1, 0, 0, 0)
    w0 = ref.philox_scalar((1, 0, 0, 0), (7, 9))[0]
    got = sim_lengths_host([np.zeros(2, np.uint8)], m, 5, 0, 0, 0, 1024, np.array([[7, 9]], np.uint32))
    assert got.tolist() == [5 + max(ref.philox_scalar((0, 0, 0, 0), (7, 9))[0] >> 22, 1) + max(w0 >> 22, 1)]


def test_the_fixed_group_has_the_lengths_it_is_built_for(groups):
    g = groups[0]
    exp = sc.fixed_expect(g)
    S = sc.S
    for r, (n, bf) in enumerate(exp):
        assert g["exp"][r][0] == n and np.array_equal(g["exp"][r][1], bf), r
    ns = [n for n, _ in exp]
    assert ns[:6] == [0, 1, S - 1, S, S + 1, 2 * S + 1] and ns[6] == 32767 > 15 * S and g["exp"][0][3] == ref.EMPTY
    assert exp[8][1].tolist() == [S - 30, S, S + 30]                                   # a base start on a tile edge
    assert ns[9] == 3 * S + 5 and np.array_equal(exp[9][1], np.arange(3 * S + 5))      # a tile of S base starts
    assert ns[10:13] == [S - 1, S, S + 1] and exp[13][1][0] == 2 * S + 77 and exp[14][1][0] == S and exp[15][1][0] == 2 * S
    total = sum(e[0] for gg in groups for e in gg["exp"])
    assert total < 2_000_000


def test_the_cases_reach_both_clamps_and_every_k(groups):
    by = {g["name"]: g for g in groups}
    assert {"fixed", "k1", "k5", "k9", "clamp", "many"} == set(by)
    raws = np.concatenate([e[2] for e in by["clamp"]["exp"]])
    assert (raws == 32767).any() and (raws == -32768).any()
    for k in (1, 5, 9):
        g = by[f"k{k}"]
        assert g["model"]["k"] == k and {0, 1, max(k // 2, 1)} <= {len(s) for s in g["seqs"]}
        assert min(int(x.min()) for x in g["shift"] if len(x)) == -32768 and max(int(x.max()) for x in g["shift"] if len(x)) == 32767
        assert min(int(x.min()) for x in g["dscale"] if len(x)) == 1 and max(int(x.max()) for x in g["dscale"] if len(x)) == 4096
    assert (by["clamp"]["model"]["sd_q10"] == 0).any() and (by["fixed"]["model"]["sd_q10"] == 0).any()


# ---------------------------------------------------------------------------------------------- the host entry points
def test_sim_host_equals_the_restatement(groups):
    from radian_amd.backend import sim_lengths_host, sim_signal_host
    for g in groups:
        a, kw = sc.call_args(g)
        n = len(g["seqs"])
        assert sim_lengths_host(*a, **kw).tolist() == [e[0] for e in g["exp"]], g["name"]
        got = sim_signal_host(*a, **kw)
        for r in range(n):
            sc.same(got, r, g["exp"][r], g["name"])
        if g["name"] == "many":
            continue
        a, kw = sc.call_args(g, range(n - 1, -1, -1))
        rev = sim_signal_host(*a, **kw)
        for r in range(n):
            sc.same(rev, n - 1 - r, g["exp"][r], g["name"] + " reversed")
    g = groups[2]
    for r in range(len(g["seqs"])):
        a, kw = sc.call_args(g, [r])
        sc.same(sim_signal_host(*a, **kw), 0, g["exp"][r], "alone")


def test_sim_host_refuses_bad_arguments_and_writes_nothing():
    from radian_amd import _lib
    L = _lib.load()
    good, bad = sc.refusal_cases()
    assert len(bad) >= 40
    from radian_amd.backend import _p

    def outs():
        return np.full(int(good["raw_off"][-1]) + 1, 77, np.int16), np.full(len(good["codes"]) + 1, 77, np.int32), np.full(good["n_reads"] + 1, 77, np.int32)

    raw, bf, st = outs()
    assert L.rd_sim_signal_host(*sc.raw_args(good), _p(good["raw_off"]), _p(raw), _p(bf), _p(st)) == 0
    assert (st[:-1] != 77).all() and st[-1] == 77 and raw[-1] == 77 and bf[-1] == 77
    for name, a in bad:
        raw, bf, st = outs()
        assert L.rd_sim_signal_host(*sc.raw_args(a), _p(a["raw_off"]), _p(raw), _p(bf), _p(st)) == -1, name   # RD_ERR_ARG
        assert (raw == 77).all() and (bf == 77).all() and (st == 77).all(), name
        if not name.startswith(("raw_off", "null raw_off")):
            ns = np.full(good["n_reads"] + 1, 77, np.int64)
            assert L.rd_sim_lengths_host(*sc.raw_args(a), _p(ns)) == -1 and (ns == 77).all(), name
    raw, bf, st = outs()
    assert L.rd_sim_signal_host(*sc.raw_args(good), _p(good["raw_off"]), _p(raw), None, _p(st)) == 0          # base_first may be null
    assert L.rd_sim_signal_host(*sc.raw_args(good), _p(good["raw_off"]), None, _p(bf), _p(st)) == -1
    assert L.rd_sim_signal_host(*sc.raw_args(good), _p(good["raw_off"]), _p(raw), _p(bf), None) == -1
    assert L.rd_sim_signal_host(*sc.raw_args(dict(good, n_reads=0, codes=None, seq_off=None)), None, None, None, None) == 0    # n_reads == 0 is RD_OK
    assert L.rd_sim_workspace_bytes(1000, 30000) == 32 * 1000 + 2 * 30000 + 128 and L.rd_sim_workspace_bytes(-1, 0) == -1


# ---------------------------------------------------------------------------------------------- moments
def test_noise_moments():
    """2^18 samples of one key, a lead alone at level 0, sd 1.0, median 0 and one DAQ unit per 1/1024 z (scale 2^20): raw is z itself.
    z has mean 0 and sd sqrt(2^20 - 1); the bounds are five standard errors: 5 * 1024 / 512 = 10 for the mean, 5 * 1024 / sqrt(2 * 2^18) = 7
    for the sd.  (The figures are printed: with the stream in the counter's second word, as the contract has it, key (12345, 678) gives
    -4.51 and 1023.24; -1.73 and 1023.86 belong to a counter with the stream in its third word.)"""
    from radian_amd.backend import SimModel, sim_signal_host
    m = SimModel(1, [0] * 4, [0] * 4, [256] * 4, [65536] * 1024)
    n = 1 << 18
    res = sim_signal_host([np.zeros(0, np.uint8)], m, n, 0, 1024, 0, 1 << 20, np.array([[12345, 678]], np.uint32))
    z = res.raw[0].astype(np.int64)
    assert len(z) == n and np.array_equal(z, ref.noise_z(n, (12345, 678))) and np.abs(z).max() <= 6138
    mean, sd = float(z.mean()), float(z.std())
    print(f"noise: mean {mean:.2f}, sd {sd:.2f}")
    assert abs(mean) <= 10 and abs(sd - 1024) <= 7


def test_dwell_mean():
    """2^16 bases of one k-mer: the mean dwell lies within five standard errors of the table's own expectation, the mean of
    clamp((m t_i + 2^23) >> 24) over the 1024 quantiles, computed exactly; the standard error comes from the same 1024 values"""
    from radian_amd.backend import SimModel, sim_signal_host
    cdf = sc.exp_cdf(0.2)
    m = SimModel(1, [0] * 4, [0] * 4, [256, 30 * 256, 1 << 23, 7777], cdf)
    n = 1 << 16
    for code, scale in ((1, 256), (3, 700)):
        res = sim_signal_host([np.full(n, code, np.uint8)], m, 0, 0, 0, 0, 1024, np.array([[99, 100 + code]], np.uint32),
                              dwell_scale=[np.full(n, scale, np.uint16)])
        d = np.diff(np.concatenate([res.base_first[0].astype(np.int64), [len(res.raw[0])]]))
        mm = (int(m.dwell_q8[code]) * scale) >> 8
        vals = [min(max((mm * int(t) + (1 << 23)) >> 24, 1), 32767) for t in cdf]
        expect = sum(vals) / 1024
        se = math.sqrt((sum(v * v for v in vals) / 1024 - expect * expect) / n)
        print(f"dwell: code {code}: mean {d.mean():.4f}, expectation {expect:.4f}, standard error {se:.4f}")
        assert d.min() >= 1 and abs(float(d.mean()) - expect) <= 5 * se


# ---------------------------------------------------------------------------------------------- the command's host side
def _transcripts(rng, lengths):
    from radian_amd.map import Transcripts
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lengths]
    return Transcripts(np.concatenate(seqs), np.concatenate([[0], np.cumsum(lengths)]), [f"tr{i}|x" for i in range(len(lengths))])


def test_kmer_table_loader_reverses_the_kmers_and_fills(tmp_path):
    from radian_amd import simulate
    p = tmp_path / "k.tsv"
    rows = ["kmer\tn_events\tlevel_mean\tlevel_sd\tdwell_mean"]
    letters = "ACGT"
    for i in range(64):
        kmer = letters[i // 16] + letters[i // 4 % 4] + letters[i % 4]            # written 5'->3'
        rows.append(f"{kmer}\t{i + 1}\t{(i - 32) / 32:.6f}\t{0.1 + i / 640:.6f}\t{10 + i:.4f}")
    p.write_text("\n".join(rows) + "\n")
    k, level, sd, dwell = simulate.read_kmer_table(str(p))
    assert k == 3
    for i in range(64):
        a, b, c = i // 16, i // 4 % 4, i % 4
        pore = c * 16 + b * 4 + a                                                 # the pore sees the last written base first
        assert level[pore] == round((i - 32) / 32 * 1024) and sd[pore] == round(float(f"{0.1 + i / 640:.6f}") * 1024) and dwell[pore] == (10 + i) * 256
    # ACG (i = 6) and TTT are missing: an error that names the k-mer as the file would write it
    p.write_text("\n".join(r for r in rows if not r.startswith(("ACG\t", "TTT\t"))) + "\n")
    with pytest.raises(SystemExit) as ei:
        simulate.read_kmer_table(str(p))
    assert "ACG" in str(ei.value) and "2 of 64" in str(ei.value)
    k, level, sd, dwell = simulate.read_kmer_table(str(p), fill_missing=True)
    w = np.array([i + 1 for i in range(64) if i not in (6, 63)], dtype=np.float64)
    lv = np.array([(i - 32) / 32 for i in range(64) if i not in (6, 63)])
    assert level[2 * 16 + 1 * 4 + 0] == level[63] == round(float((w * lv).sum() / w.sum()) * 1024)
    assert level[0] == -1024                                                       # the others are as before
    # the stand-in: levels within +-1.5 z, the all-A k-mer quiet
    level, sd, dwell = simulate.standin_tables(5, 3)
    assert level.min() >= -1536 and level.max() <= 1536 and len(set(level.tolist())) > 500 and sd[0] == 41 and (sd[1:] == 307).all() and (dwell == 7680).all()
    assert not np.array_equal(level, simulate.standin_tables(5, 4)[0])
    cdf = simulate.dwell_cdf(0.2)
    assert np.array_equal(cdf, sc.exp_cdf(0.2)) and (np.diff(cdf.astype(np.int64)) >= 0).all() and cdf.max() <= 1 << 20


def _run(tmp_path, argv, plans_fn=None, tr=None):
    from radian_amd import simulate
    args = simulate.build_parser().parse_args(["x.fa", "-o", str(tmp_path)] + argv)
    simulate.check_args(args)
    model = simulate.build_model(args)
    plans = plans_fn(args) if plans_fn else simulate.draw_reads(args, tr, np.random.Generator(np.random.PCG64(args.seed)))
    st = simulate.run(args, HostBackend(), tr, model, plans)
    return args, model, plans, st


def test_truth_files_round_trip_through_their_readers(tmp_path):
    from radian_amd import compare, fast5, polya, simulate
    from radian_amd.label_build import encode_reference, read_ref_tsv
    tr = _transcripts(np.random.default_rng(8), [900, 150, 2500])
    tr.codes[int(tr.offsets[1]) + 20] = 255                       # an N: fragments over it are drawn again
    out = tmp_path / "a"
    args, model, plans, st = _run(out, ["--reads", "9", "--seed", "4", "--batch-reads", "4", "--reads-per-file", "5", "--min-length", "100",
                                        "--length-median", "400"], tr=tr)
    assert st["reads"] == 9 and st["files"] == 2 and sorted(f for f in os.listdir(out) if f.endswith(".fast5")) == ["sim_0000.fast5", "sim_0001.fast5"]
    assert "reads: 9;" in simulate.summary(st) and "median dwell:" in simulate.summary(st)
    reads = {r.read_id: r.get_raw_data() for f in ("sim_0000.fast5", "sim_0001.fast5") for r in fast5.iter_reads(str(out / f))}
    truth = [ln.split("\t") for ln in open(out / "truth.tsv").read().splitlines()]
    assert truth[0] == ["read_id", "ref_name", "ref_start", "ref_end", "n_samples", "lead", "tail_nt", "tail_start", "tail_end"] and len(truth) == 10
    refs, paf, moves = read_ref_tsv(str(out / "read_ref.tsv")), compare.read_paf(str(out / "truth.paf")), polya.read_moves(str(out / "truth_moves.tsv"))
    adapter = simulate.encode(args.adapter, "")
    for p, row in zip(plans, truth[1:]):
        rid = p.read_id
        assert row[0] == rid and len(reads[rid]) == int(row[4]) and row[1] == tr.names[p.t] and (int(row[2]), int(row[3])) == (p.ref_start, p.ref_end)
        assert p.ref_end == tr.length(p.t) and p.ref_end - p.ref_start >= 100
        assert refs[rid] == tr.letters(p.t, p.ref_start, p.ref_end) and "N" not in refs[rid]
        assert paf[rid] == (tr.names[p.t], tr.length(p.t), p.ref_start)
        assert all(len(ln.split("\t")) == 12 for ln in open(out / "truth.paf").read().splitlines())
        # the same read again, alone: the files hold what the entry point gives
        res, seqs = simulate.simulate_batch(HostBackend(), model, [p], tr, adapter, args)
        assert np.array_equal(res.raw[0], reads[rid])
        assert np.array_equal(seqs[0][len(adapter) + p.tail:], encode_reference(refs[rid]))     # the fragment in decode order
        first, last = moves[rid]
        F = p.ref_end - p.ref_start
        bf = res.base_first[0]
        assert len(first) == F and np.array_equal(first[::-1], bf[len(adapter) + p.tail:]) and last[0] == len(reads[rid]) - 1
        assert (first <= last).all() and np.array_equal(last[1:] + 1, first[:-1])
        h = model.k // 2
        if p.tail > 2 * h:
            assert (int(row[7]), int(row[8])) == (bf[len(adapter) + h], bf[len(adapter) + p.tail - h]) and int(row[6]) == p.tail
    # the same run with other batches: the same bytes
    out2 = tmp_path / "b"
    _run(out2, ["--reads", "9", "--seed", "4", "--batch-reads", "9", "--reads-per-file", "5", "--min-length", "100", "--length-median", "400"], tr=tr)
    for f in sorted(os.listdir(out)):
        assert open(out / f, "rb").read() == open(out2 / f, "rb").read(), f
    # modified sites: the base's level moves and its dwell stretches, nothing else changes place
    sites = tmp_path / "sites.tsv"
    sites.write_text(f"{tr.names[2]} 2400 0.5 2.0 1.0\n{tr.names[2]} 2450 -0.25 1.0 0.0\n")
    got = simulate.read_sites(str(sites), tr)
    assert got == {2: [(2400, 512, 512, 1.0), (2450, -256, 256, 0.0)]}
    args.reads = 30
    mod = simulate.draw_reads(args, tr, np.random.Generator(np.random.PCG64(1)), got)
    hit = [p for p in mod if p.t == 2 and p.ref_start <= 2400]
    assert hit and all(p.mods == [(2400, 512, 512)] for p in hit) and all(not p.mods for p in mod if p not in hit)
    codes, shift, scale = simulate.compose(hit[0], tr, adapter)
    b = len(adapter) + hit[0].tail + (hit[0].ref_end - 1 - 2400)
    assert codes[b] == tr.codes[int(tr.offsets[2]) + 2400] and shift[b] == 512 and scale[b] == 512 and np.count_nonzero(shift) == 1


def test_window_labels_follow_the_truth():
    from radian_amd import simulate
    args = simulate.build_parser().parse_args(["x", "-o", "y", "--reads", "1", "--step-size", "512", "--max-label-len", "40"])
    # 10 bases before the fragment (first sample 0 .. 900), fragment bases every 50 samples from 1000; 3000 samples
    bf = np.concatenate([np.arange(10) * 100, 1000 + 50 * np.arange(40)]).astype(np.int32)
    codes = np.concatenate([np.zeros(10, np.uint8), (np.arange(40) % 4).astype(np.uint8)])
    kept, dropped = simulate.window_labels(np.arange(3000, dtype=np.float32), codes, bf, 10, args)
    # windows start at 0, 512, 1024, 1536 and 2048 (952 samples): the first two start before sample 1000 (edge)
    assert dropped == {"edge": 2, "empty": 0, "too-long": 0, "infeasible": 0} and len(kept) == 3
    assert kept[0][1] == 1024 and kept[0][2].tolist() == [j % 4 for j in range(1, 21)]           # [1024, 2048): bases at 1050 .. 2000
    assert kept[1][1] == 1024 and kept[1][2].tolist() == [j % 4 for j in range(11, 32)]          # [1536, 2560): bases at 1550 .. 2550
    assert kept[2][1] == 952 and kept[2][2].tolist() == [j % 4 for j in range(21, 40)]           # [2048, 3000): bases at 2050 .. 2950
    assert kept[2][0][:952].tolist() == list(range(2048, 3000)) and (kept[2][0][952:] == 0).all()
    args.max_label_len = 19
    kept2, dropped2 = simulate.window_labels(np.arange(3000, dtype=np.float32), codes, bf, 10, args)
    assert dropped2 == {"edge": 2, "empty": 0, "too-long": 2, "infeasible": 0} and len(kept2) == 1
    # a label that needs more rows than the window has samples: 50 equal bases in a last window of 76 samples (99 rows)
    bf3 = np.concatenate([[0], 1030 + np.arange(50)]).astype(np.int32)
    args.max_label_len, args.step_size = 255, 1024
    kept3, dropped3 = simulate.window_labels(np.arange(1100, dtype=np.float32), np.array([1] + [0] * 50, np.uint8), bf3, 0, args)
    assert dropped3 == {"edge": 0, "empty": 0, "too-long": 0, "infeasible": 1} and len(kept3) == 1 and kept3[0][2].tolist() == [1]


def test_polya_finds_the_simulated_tails(tmp_path):
    """40 reads: a 30-base adapter, 30 .. 149 A, 600 .. 1199 random bases, 300 samples of lead; the stand-in model at median 600, MAD 60;
    rd_sim_signal_host, then rd_polya_segment_host at its defaults (min_samples 480).  Every read is ok and both ends lie within
    (max_gap + 2) win = 128 samples of truth.tsv's tail: the search joins flat windows over max_gap others and a window straddles each end."""
    from radian_amd import fast5, simulate
    from radian_amd.backend import POLYA_OK, PolyaParams, polya_segment_host
    rng = np.random.default_rng(2024)
    lengths = rng.integers(600, 1200, 40)
    tr = _transcripts(rng, lengths)
    tails = rng.integers(30, 150, 40)

    def plans(args):
        return [simulate.ReadPlan(f"r{i:03d}", i, 0, int(lengths[i]), int(tails[i]), rng.integers(0, 1 << 32, 2, dtype=np.uint64).astype(np.uint32))
                for i in range(40)]

    args, model, pl, st = _run(tmp_path, ["--reads", "40", "--lead-samples", "300", "--median", "600", "--mad", "60", "--batch-reads", "16"], plans, tr)
    assert len(args.adapter) == 30 and model.k == 5
    reads = {r.read_id: r.get_raw_data() for r in fast5.iter_reads(str(tmp_path / "sim_0000.fast5"))}
    truth = [ln.split("\t") for ln in open(tmp_path / "truth.tsv").read().splitlines()][1:]
    p = PolyaParams()
    assert p.min_samples == 480 and (p.max_gap + 2) * p.win == 128
    got = polya_segment_host([reads[row[0]] for row in truth], p)
    worst = [0, 0]
    for r, row in enumerate(truth):
        a, e, n = int(row[7]), int(row[8]), int(row[4])
        assert int(row[6]) == tails[r] and 0 < a < e and (e - a) < 0.4 * n
        assert got.status[r] == POLYA_OK, (row[0], int(got.status[r]))
        worst = [max(worst[0], abs(int(got.tail_start[r]) - a)), max(worst[1], abs(int(got.tail_end[r]) - e))]
    print(f"polya on simulated tails: worst start error {worst[0]}, worst end error {worst[1]}")
    assert worst[0] <= 128 and worst[1] <= 128


# ---------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_asan_sim_host(tmp_path):
    """tests/asan_sim.cpp: the host side of sim.hip (argument check, the rules, the plain loops) and the budget cut it uses, built with
    AddressSanitizer + UBSan as a stand-alone executable, on exact-size heap buffers; Philox's known answers; every refusal"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_sim"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "asan_sim.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "60"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"no sanitizer report" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
    last = r.stdout.decode().splitlines()[-1].split()
    assert int(last[0]) >= 60 and int(last[2]) >= 25          # "<n> accepted <m> refused"
