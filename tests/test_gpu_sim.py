"""GPU checks of the signal simulation (rd_sim_lengths / rd_sim_signal, radian_amd/csrc/sim.hip) against the plain restatement of its contract
(tests/_sim_ref.py) and against rd_sim_signal_host, and of `python -m radian_amd.simulate`.  Everything is compared for EXACT equality.

Sizes follow the sample kernel (tests/_sim_cases.py; the cases' defining conditions are asserted in tests/test_sim_cpu.py): a workgroup
takes a tile of S = 2048 samples of one read -- reads of 0, 1, S - 1, S, S + 1 and 2 S + 1 samples, a base of 32767 samples over 16 tiles,
base starts and lead ends on tile edges, a tile of S base starts, leads of 0 and over 2 S, L = 0, 1 and k / 2, k = 1, 5 and 9, per-base
shifts and scales at their limits, both clamps, sd 0, and 70 reads cut into more than 5 launches.  All cases together stay under 2 10^6
samples."""
import os

import numpy as np
import pytest

import _sim_cases as sc
import _sim_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    gs = sc.all_groups()
    for g in gs:
        g["exp"] = sc.expect(g)
    return gs


def _need(g):
    from radian_amd.backend import sim_workspace_bytes
    return [sim_workspace_bytes(len(s), e[0]) for s, e in zip(g["seqs"], g["exp"])]


def test_device_equals_the_host_twin_and_the_restatement(be, groups):
    from radian_amd.backend import sim_signal_host
    for g in groups:
        a, kw = sc.call_args(g)
        assert be.sim_lengths(*a, **kw).tolist() == [e[0] for e in g["exp"]], g["name"]
        got, host = be.sim_signal(*a, **kw), sim_signal_host(*a, **kw)
        for r in range(len(g["seqs"])):
            sc.same(got, r, g["exp"][r], g["name"])
            sc.same(host, r, g["exp"][r], g["name"] + " host")
    assert {ref.OK, ref.EMPTY} == {e[3] for e in groups[0]["exp"]}


def test_a_read_does_not_depend_on_order_batch_or_budget(be, groups):
    from radian_amd.backend import sim_launch_bytes
    for g in groups[:5]:
        n = len(g["seqs"])
        a, kw = sc.call_args(g, range(n - 1, -1, -1))
        rev = be.sim_signal(*a, **kw)
        for r in range(n):
            sc.same(rev, n - 1 - r, g["exp"][r], g["name"] + " reversed")
    g = groups[0]
    for r in range(len(g["seqs"])):                       # one read alone
        a, kw = sc.call_args(g, [r])
        sc.same(be.sim_signal(*a, **kw), 0, g["exp"][r], "alone")
    # 70 reads under a budget that holds a dozen of them: more than 5 launches (the greedy cut, done again here)
    g = groups[5]
    need = _need(g)
    budget = sim_launch_bytes(5) + sorted(need)[-1] * 6
    launches, acc = 1, 0
    for b in need:
        if acc + b > budget - sim_launch_bytes(5):
            launches, acc = launches + 1, 0
        acc += b
    assert len(need) == 70 and launches > 5
    a, kw = sc.call_args(g)
    cut = be.sim_signal(*a, budget_bytes=budget, **kw)
    for r in range(70):
        sc.same(cut, r, g["exp"][r], "cut")
    assert be.sim_lengths(*a, budget_bytes=sim_launch_bytes(5) + sorted(need)[-1], **kw).tolist() == [e[0] for e in g["exp"]]
    # the fixed group under a budget of its largest read: one launch per large read
    g = groups[0]
    a, kw = sc.call_args(g)
    cut = be.sim_signal(*a, budget_bytes=sim_launch_bytes(1) + max(_need(g)), **kw)
    for r in range(len(g["seqs"])):
        sc.same(cut, r, g["exp"][r], "fixed cut")


def test_a_budget_that_excludes_exactly_one_read(be, groups):
    from radian_amd import RadianHipError
    from radian_amd.backend import SIM_TOO_LARGE, sim_launch_bytes
    g = groups[2]
    need = _need(g)
    big = int(np.argmax(need))
    budget = sim_launch_bytes(5) + need[big] - 1
    assert sorted(need)[-2] < need[big]
    a, kw = sc.call_args(g)
    ns = [e[0] for e in g["exp"]]
    with pytest.raises(RadianHipError) as ei:
        be.sim_signal(*a, n_samples=ns, budget_bytes=budget, **kw)
    assert f"read {big} " in str(ei.value) and "1 read(s) not simulated" in str(ei.value)
    got = be.sim_signal(*a, n_samples=ns, budget_bytes=budget, allow_too_large=True, **kw)
    for r in range(len(need)):
        if r == big:
            assert got.status[r] == SIM_TOO_LARGE and not got.raw[r].any() and not got.base_first[r].any()
        else:
            sc.same(got, r, g["exp"][r], "budget")


def test_signal_refuses_bad_arguments_before_anything_is_written(be):
    from radian_amd.backend import _p
    L, h = be._L, be._h
    good, bad = sc.refusal_cases()

    def outs():
        return np.full(int(good["raw_off"][-1]) + 1, 77, np.int16), np.full(len(good["codes"]) + 1, 77, np.int32), np.full(good["n_reads"] + 1, 77, np.int32)

    raw, bf, st = outs()
    assert L.rd_sim_signal(h, *sc.raw_args(good), _p(good["raw_off"]), 0, _p(raw), _p(bf), _p(st)) == 0
    assert (st[:-1] != 77).all() and st[-1] == 77 and raw[-1] == 77 and bf[-1] == 77
    for name, a in bad:
        raw, bf, st = outs()
        assert L.rd_sim_signal(h, *sc.raw_args(a), _p(a["raw_off"]), 0, _p(raw), _p(bf), _p(st)) == -1, name   # RD_ERR_ARG
        assert (raw == 77).all() and (bf == 77).all() and (st == 77).all(), name
        if not name.startswith(("raw_off", "null raw_off")):
            ns = np.full(good["n_reads"] + 1, 77, np.int64)
            assert L.rd_sim_lengths(h, *sc.raw_args(a), 0, _p(ns)) == -1 and (ns == 77).all(), name
    raw, bf, st = outs()
    assert L.rd_sim_signal(h, *sc.raw_args(good), _p(good["raw_off"]), -1, _p(raw), _p(bf), _p(st)) == -1              # a negative budget
    assert L.rd_sim_signal(None, *sc.raw_args(good), _p(good["raw_off"]), 0, _p(raw), _p(bf), _p(st)) == -1            # a null context
    assert (raw == 77).all() and (bf == 77).all() and (st == 77).all()
    assert L.rd_sim_signal(h, *sc.raw_args(good), _p(good["raw_off"]), 0, _p(raw), None, _p(st)) == 0                  # base_first may be null
    assert L.rd_sim_signal(h, *sc.raw_args(dict(good, n_reads=0, codes=None, seq_off=None)), None, 0, None, None, None) == 0


def _run_cli(argv, capsys):
    from radian_amd import simulate
    simulate.main(argv)
    return capsys.readouterr().out


def test_command_on_three_transcripts(be, tmp_path, capsys):
    """12 reads of 3 transcripts: the fast5 files hold sim_signal's samples; every file is bit-identical across two --batch-reads and two
    budgets; --shards' records carry the labels the truth implies; polya on the output (tails of 70 A) finds the tails within (max_gap + 2) win = 128"""
    from radian_amd import fast5, polya, simulate, tfrecord
    from radian_amd.label_build import is_val
    from radian_amd.map import Transcripts
    rng = np.random.default_rng(12)
    fa = tmp_path / "tr.fa"
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in (700, 1500, 420)]
    fa.write_text("".join(f">t{i}|a|b\n{s}\n" for i, s in enumerate(seqs)))
    common = [str(fa), "--reads", "12", "--seed", "3", "--length-median", "500", "--tail", "70", "--reads-per-file", "7",
              "--val-fraction", "0.3", "--windows-per-shard", "40"]
    runs = {}
    for name, extra in (("a", ["--batch-reads", "5"]), ("b", ["--batch-reads", "12", "--budget-bytes", "600000"])):
        out = tmp_path / name
        text = _run_cli(common + ["-o", str(out), "--shards", str(out / "shards")] + extra, capsys)
        assert "reads: 12;" in text and "fast5 files: 2" in text
        runs[name] = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}
    assert sorted(runs["a"]) == sorted(runs["b"]) and {"sim_0000.fast5", "sim_0001.fast5", "truth.tsv", "read_ref.tsv", "truth.paf", "truth_moves.tsv"} <= set(runs["a"])
    for f in runs["a"]:
        assert runs["a"][f] == runs["b"][f], f
    out = tmp_path / "a"
    # the same plans through the entry point
    args = simulate.build_parser().parse_args(common + ["-o", str(out)])
    simulate.check_args(args)
    tr = Transcripts.read(str(fa))
    model = simulate.build_model(args)
    plans = simulate.draw_reads(args, tr, np.random.Generator(np.random.PCG64(3)))
    adapter = simulate.encode(args.adapter, "")
    res, codes = simulate.simulate_batch(be, model, plans, tr, adapter, args)
    reads = {r.read_id: r.get_raw_data() for f in ("sim_0000.fast5", "sim_0001.fast5") for r in fast5.iter_reads(str(out / f))}
    assert list(reads) == [p.read_id for p in plans]
    for r, p in enumerate(plans):
        assert np.array_equal(reads[p.read_id], res.raw[r]), p.read_id
    # the shards: every kept window, in read order within its split, with the truth's label
    norm, status = be.normalise_reads(res.raw, args.outlier_clip)
    exp = {"train": [], "val": []}
    for r, p in enumerate(plans):
        assert status[r] == 0
        kept, _ = simulate.window_labels(norm[r], codes[r], res.base_first[r], len(adapter) + p.tail, args)
        exp["val" if is_val(p.read_id, 0.3) else "train"] += kept
    assert exp["train"] and exp["val"]
    for split in ("train", "val"):
        files = sorted(f for f in os.listdir(out / "shards" / split))
        assert len(files) == (len(exp[split]) + 39) // 40
        shards = [tfrecord.read_shard(str(out / "shards" / split / f)) for f in files]
        got = [(sh.signals[i], int(sh.input_len[i]), sh.label(i)) for sh in shards for i in range(len(sh))]
        assert len(got) == len(exp[split])
        for (sig, n, label), (win, sl, lab) in zip(got, exp[split]):
            assert n == sl and np.array_equal(label, lab) and np.array_equal(sig, win.astype(np.float32))
    # polya on the output
    polya.main([str(out), "-o", str(tmp_path / "polya.tsv")])
    capsys.readouterr()
    rows = {ln.split("\t")[0]: ln.split("\t") for ln in open(tmp_path / "polya.tsv").read().splitlines()[1:]}
    truth = [ln.split("\t") for ln in open(out / "truth.tsv").read().splitlines()][1:]
    assert len(rows) == 12
    for t in truth:
        row = rows[t[0]]
        assert row[1] == "ok" and abs(int(row[3]) - int(t[7])) <= 128 and abs(int(row[4]) - int(t[8])) <= 128, (t, row)
