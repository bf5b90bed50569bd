"""No-GPU check of the packed window heads the planner builds beside the tile lists (radian_amd/csrc/plan.hip, PackLayer in common.h;
DESIGN.md 4.7): tests/asan_headpack.cpp, built with AddressSanitizer + UBSan, on random models, read sets, chunk and step."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_heads_properties_and_asan(tmp_path):
    """Every head row is packed exactly once and maps back into its head, every row a packed row reads or writes lies inside the tensors, the
    taps a class leaves out lie before the window, the classes tile the launch behind the stream tiles, and the tile lists are byte for byte
    what they are without packing (tests/asan_headpack.cpp).  A violated property would be an out-of-bounds access or a wrong row on the GPU."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "asan_headpack"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "radian_amd", "csrc", "plan.hip"),
                        os.path.join(ROOT, "tests", "asan_headpack.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([str(exe), "600"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"every property holds" in r.stdout, (r.stdout.decode()[-800:], r.stderr.decode()[-3000:])
