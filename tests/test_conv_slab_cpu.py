"""No-GPU check of the slab-tile classification the exact-fp32 conv kernel and the planner share (rd_slab_tile in radian_amd/csrc/common.h,
the counts of radian_amd/csrc/plan.hip): tests/asan_conv_slab.cpp, built with AddressSanitizer + UBSan, on random models,
read sets, chunk and step."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_tiles_properties_and_asan(tmp_path):
    """A tile qualifies exactly when its 128 rows are consecutive interior rows of one segment with no row redirected to the read's stream
    (stated row by row in tests/asan_conv_slab.cpp); every row its region holds at any dilation up to 32 is the segment's own row inside
    the tensors; the planner's counts are the qualifying tiles of the list and of a packed launch's stream prefix; the mixed tile never
    qualifies.  A tile that qualified wrongly would read rows of another segment on the GPU."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_conv_slab"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "radian_amd", "csrc", "plan.hip"),
                        os.path.join(ROOT, "tests", "asan_conv_slab.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "400"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"every property holds" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
