"""No-GPU checks of the C-ABI boundary: the library builds/loads and exports every symbol
include/radian_hip.h (the boundary) and include/radian_hip_diag.h (measurement entry points) declare; without a GPU the product fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from radian_amd import build, _lib
    build.build()
    return _lib.load()


def declared_symbols(header="radian_hip.h"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_all_exported(lib):
    from radian_amd import _lib
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"libradian_hip.so does not export {n}"
    # and the ctypes table binds exactly the declared set
    assert sorted(_lib.SIGNATURES) == names


def test_diag_header_holds_the_measurement_entry_points_and_the_product_header_none(lib):
    """Round 6: include/radian_hip.h lists what a RADIAN maintainer binds; launch-shape switches, kernel timers and
    pipeline read-outs live in include/radian_hip_diag.h (same library).  Both headers together == the library's exported rd_ symbols ==
    the two ctypes tables; the command-line route (basecall / launch / dist and the readers) calls no diagnostic entry point."""
    import subprocess
    from radian_amd import _lib
    diag = declared_symbols("radian_hip_diag.h")
    prod = declared_symbols()
    assert sorted(_lib.DIAG_SIGNATURES) == diag and len(diag) == 14
    assert not set(diag) & set(prod)
    for n in diag:
        assert hasattr(lib, n), f"libradian_hip.so does not export {n}"
    for word in ("rd_timer_", "rd_set_conv_shape", "rd_set_conv_fuse", "rd_set_decode_form", "rd_split3", "rd_pipe_stats", "rd_pipe_policy_read", "rd_set_trie_budget", "rd_map_diag_", "rd_diag_score_math", "RD_SM_", "RD_TIMER_"):
        assert word not in open(os.path.join(ROOT, "include", "radian_hip.h")).read(), word
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if re.search(r"\s[TW]\s+rd_[a-z0-9_]+$", ln)})
    assert exported == sorted(prod + diag), sorted(set(exported) ^ set(prod + diag))
    # the command line's modules never reach a diagnostic wrapper of Backend
    wrappers = ("set_conv_shape", "set_conv_fuse", "split3", "set_decode_form", "pipe_policy_read", "pipe_stats", "timer_enable", "timer_read", "timer_read_launches", "set_trie_budget", "map_diag_minimizers", "map_diag_chain", "score_math", "score_math_host")
    pkg = os.path.join(ROOT, "radian_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f not in ("backend.py", "_lib.py"):
            src = open(os.path.join(pkg, f)).read()
            for w in wrappers:
                assert not re.search(r"\b" + w + r"\(", src), (f, w)
    # INTEGRATION.md binds the product header only
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in diag:
        assert n not in integ, n


def test_version_and_limits(lib):
    assert lib.rd_version() == 1
    assert lib.rd_decode_max_width() >= 25


def test_no_cpu_fallback_without_gpu(lib):
    n = ctypes.c_int(-1)
    lib.rd_device_count(ctypes.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is present")
    from radian_amd import Backend, RadianHipError
    with pytest.raises(RadianHipError) as ei:
        Backend(0)
    assert "no CPU fallback" in str(ei.value)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under radian_amd/ may reference it."""
    pkg = os.path.join(ROOT, "radian_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.lower(), f"{f} mentions the oracle"


def test_weight_blob_roundtrip():
    import numpy as np
    from radian_amd import weights
    assert weights.n_params() == 2200581
    flat = weights.synthetic_weights(seed=1)
    blob = weights.pack_blob(flat)
    back, dil = weights.unpack_blob(blob)
    assert dil == weights.DEFAULT_DILATIONS
    assert np.array_equal(back, flat)


def test_no_experiment_branches_in_the_product_sources():
    """the ablation / measurement hooks (RD_BF3_*, RD_CLOCK_STAMPS, RD_EXPERIMENTS, RD_X_* environment switches) left the
    product sources in round 5 -- no conditional compilation on an RD_ macro and no environment switch inside the library: a wrong -D or
    a stray variable cannot change what the shipped kernels compute.  (Their measurements: profiles/, DESIGN_LOG.md.)"""
    import glob
    import re
    csrc = os.path.join(ROOT, "radian_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) >= 15
    for f in files:
        text = open(f).read()
        for ln in text.split("\n"):
            s = ln.strip()
            if s.startswith("#") and re.match(r"#\s*(if|ifdef|ifndef|elif)\b", s):
                assert not re.search(r"\bRD_[A-Z0-9_]+", s), (os.path.basename(f), s)
        assert "getenv(\"RD_" not in text and "getenv(\"RADIAN_" not in text, os.path.basename(f)
    build_py = open(os.path.join(ROOT, "radian_amd", "build.py")).read()
    assert "RD_EXPERIMENTS" not in build_py
