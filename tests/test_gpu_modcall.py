"""GPU checks of modcall: rd_modcall against the restatement of its contract (tests/_modcall_ref.py) on the seeded
cases (tests/_modcall_cases.py; their defining conditions are asserted in tests/test_modcall_cpu.py) and against rd_modcall_host, one job
per call and the batch reversed, the identity with rd_eventalign on the device, the budget, the refusals, and `python -m
radian_amd.eventalign --call` on small `simulate` runs.  Every output field is compared for EXACT equality.

Sizes follow the kernel: one wave per job, state i in lane i (S = 1, 2, 21, 62 and 63 states), tiles of 64 rows (R on both sides of 64 and
128, R = S, 1000 and 2^15 at the value bounds, 2^15 + 1 refused), four jobs of a read to a workgroup (reads of 1, 2, 3 and 6 jobs, and
none), the last window of a batch ending on the block's last sample."""
import numpy as np
import pytest

import _eventalign_cases as sc
import _modcall_cases as mc
import _modcall_checks as chk
import _modcall_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from radian_amd import Backend
    b = Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def groups():
    gs = mc.groups()
    for cases in gs.values():
        for c in cases:
            mc.reference(c)
    return gs


def _call(be, group, cases, order=None, **kw):
    args, flat = mc.call_args(cases, order)
    return be.modcall(model=mc.backend_model(group), flank=mc.GROUPS[group][1], **args, **kw), flat


def _fields(res, j):
    return {f: int(getattr(res, f)[j]) for f in ref.FIELDS}


@pytest.fixture(scope="module")
def whole(be, groups):
    return {g: _call(be, g, cases) for g, cases in groups.items()}


def test_the_batches_equal_the_restatement_and_the_host(groups, whole):
    """every case of a group in one call: every status sits between jobs that are done, and none of them is affected"""
    from radian_amd.backend import modcall_host
    seen = set()
    for g, cases in groups.items():
        res, flat = whole[g]
        args, _ = mc.call_args(cases)
        host = modcall_host(model=mc.backend_model(g), flank=mc.GROUPS[g][1], **args)
        for j, (ci, ji) in enumerate(flat):
            assert _fields(res, j) == mc.reference(cases[ci])[ji] == _fields(host, j), (cases[ci]["name"], ji)
            seen.add(int(res.status[j]))
    assert seen == {ref.OK, ref.NO_ANCHOR, ref.NO_PATH, ref.TOO_LONG}


def test_one_job_per_call_reversed_and_shuffled(be, groups, whole):
    for g, cases in groups.items():
        res, flat = whole[g]
        for j, (ci, ji) in enumerate(flat):
            c = dict(cases[ci], jobs=[cases[ci]["jobs"][ji]])
            one, _ = _call(be, g, [c])
            assert _fields(one, 0) == _fields(res, j), (c["name"], ji)
        rev, rflat = _call(be, g, cases[::-1])
        back = {(len(cases) - 1 - ci, ji): j for j, (ci, ji) in enumerate(rflat)}
        order = np.random.default_rng(7).permutation(len(flat))
        shuf, sflat = _call(be, g, cases, order)
        where = {key: j for j, key in enumerate(sflat)}
        for j, key in enumerate(flat):
            assert _fields(rev, back[key]) == _fields(res, j) == _fields(shuf, where[key]), (g, key)


def test_identity_with_eventalign_on_the_device(be):
    """first / last from Backend.eventalign on a given scale: vit_ref is the summed cell cost of that path over the window's rows"""
    raws, seqs = chk.identity_reads()
    n = len(raws)
    ea = be.eventalign(raws, seqs, mc.backend_model("k3"), m2=[2 * sc.MEDIAN] * n, d4=[sc.D4] * n)
    assert (ea.status == 0).all()
    chk.check_against_path(ea.first_step, ea.last_step, raws, seqs, be.modcall, exact=True)


def _need(cases):
    from radian_amd.backend import modcall_workspace_bytes
    return [modcall_workspace_bytes(len(c["raw"]), len(c["codes"]), len(c["jobs"]), sum(len(a) for _, a in c["jobs"])) if c["jobs"] else 0 for c in cases]


def test_budget_from_the_workspace_formula(be, groups, whole):
    """a budget of exactly the largest read's block: every job is done, over several launches; one byte less: that read's jobs alone are
    TOO_LARGE, the call names the read with RD_ERR_NOMEM and the others are as before"""
    from radian_amd.backend import MC_TOO_LARGE, RadianHipError
    cases = groups["k3"]
    res0, flat = whole["k3"]
    need = _need(cases)
    big = int(np.argmax(need))
    assert sum(need) > 3 * need[big] and sorted(need)[-2] < need[big] and len(cases[big]["jobs"]) >= 1
    res, _ = _call(be, "k3", cases, budget_bytes=need[big])
    for j in range(len(flat)):
        assert _fields(res, j) == _fields(res0, j)
    with pytest.raises(RadianHipError) as ei:
        _call(be, "k3", cases, budget_bytes=need[big] - 1)
    assert f"read {big} " in str(ei.value) and "1 read(s) not done" in str(ei.value)
    res, _ = _call(be, "k3", cases, budget_bytes=need[big] - 1, allow_too_large=True)
    for j, (ci, ji) in enumerate(flat):
        if ci == big:
            assert _fields(res, j) == dict(status=MC_TOO_LARGE, n_rows=0, n_states=0, vit_ref=0, vit_alt=0, fwd_ref=0, fwd_alt=0)
        else:
            assert _fields(res, j) == _fields(res0, j)
    # a small budget: many launches, and every read over it is reported
    small = sorted(v for v in need if v)[len(need) // 3]
    res, _ = _call(be, "k3", cases, budget_bytes=small, allow_too_large=True)
    n_large = 0
    for j, (ci, ji) in enumerate(flat):
        if need[ci] <= small:
            assert _fields(res, j) == _fields(res0, j)
        else:
            assert int(res.status[j]) == MC_TOO_LARGE
            n_large += 1
    assert 0 < n_large < len(flat)


def test_refusals(be, groups):
    from radian_amd.backend import RadianHipError
    cases = [c for c in groups["k3"] if c["name"] in ("anchors", "short")]
    args, _ = mc.call_args(cases)
    model = mc.backend_model("k3")

    def refused(**change):
        with pytest.raises(RadianHipError):
            be.modcall(model=model, **{**args, "flank": 6, **change})

    refused(flank=28)
    refused(d4=[0, 240])
    refused(job_read=[2] + args["job_read"][1:])
    refused(alt_first=[30] + args["alt_first"][1:])
    refused(alts=[tuple(np.repeat(a, 10) for a in args["alts"][0])] + args["alts"][1:], alt_first=[0] + args["alt_first"][1:])
    refused(alts=[(np.array([1 << 14], np.int32), args["alts"][0][1], args["alts"][0][2])] + args["alts"][1:])
    refused(budget_bytes=-1)
    assert len(be.modcall(args["raws"], args["seqs"], args["m2"], args["d4"], args["firsts"], args["lasts"], model, [], [], [], flank=6).status) == 0


def test_command_on_a_simulated_run(tmp_path, monkeypatch):
    """24 reads of `simulate` with --call under plain, --events and --events --refine: every file is bit-identical across --batch-reads 1 / 7
    / all and two budgets, and calls.tsv is the restatement's composition on what rd_modcall was asked (and what it answered is what the
    restatement and the host twin say)"""
    from radian_amd import Backend, eventalign
    from radian_amd.backend import (eventalign_banded_workspace_bytes, eventalign_events_workspace_bytes, eventalign_workspace_bytes,
                                    modcall_workspace_bytes, segment_max_events)
    import _modcall_e2e as e2e
    log = []
    monkeypatch.setattr(eventalign, "Backend", e2e.recording(Backend, log))
    sim = chk.simulate_for_command(tmp_path)
    truth = [ln.split("\t") for ln in open(tmp_path / "sim_a" / "truth.tsv").read().splitlines()[1:]]
    need = 0
    for r in truth:
        n, L, T = int(r[4]), int(r[3]) - int(r[2]), int(r[4]) - max(0, int(r[8]) - 32)
        need = max(need, eventalign_workspace_bytes(T, L), eventalign_events_workspace_bytes(segment_max_events(T, 4), L),
                   eventalign_banded_workspace_bytes(T, L), modcall_workspace_bytes(n, L, 5, 5))
    variants = (("b1", ["--batch-reads", "1"]), ("b7", ["--batch-reads", "7", "--budget-bytes", str(need)]),
                ("all", ["--batch-reads", "24", "--budget-bytes", str(3 * need)]))
    seen = {}
    for mode, extra in (("plain", []), ("events", ["--events"]), ("refine", ["--events", "--refine"])):
        _, files, text = chk.check_command(tmp_path, log, variants, extra, prefix=mode + "_", sim=sim)
        assert "too-large: 0" in text
        seen[mode] = files["calls"]
    assert seen["plain"] != seen["events"] != seen["refine"]


@pytest.mark.parametrize("kind", ["clean", "smeared"])
def test_accuracy_on_the_device(tmp_path, kind):
    """the accuracy chain of tests/_modcall_e2e.py on the GPU: the same bounds as on the host twins"""
    chk.check_accuracy(tmp_path, kind)
