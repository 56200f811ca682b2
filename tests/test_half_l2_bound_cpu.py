"""The error bound of the half-precision Euclidean selection path, on the CPU: `velesdb_amd/csrc/vdb_half_l2.hpp` (host arithmetic, the
text the library compiles) must dominate the observed error of a selection score for three f32 summation orders at dims 128 - 4 096 on
N(0,1), large-norm and near-duplicate data (tests/half_l2_bound_model.cpp, built stand-alone with ASan + UBSan); and the new kernel bit
is the same shift in the header, the ctypes binding and the Rust constants (it is not a decimal literal: the ABI tests do not see it)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_delta_dominates_every_summation_order(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "half_l2_bound_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "half_l2_bound_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)   # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["failed_checks"] == 0 and line["cases"] == 5 * 2 * 3 * 40 * 3
    assert line["worst_err_over_delta"] < 0.5          # the factor 8 of l2_rerank_verify's slack leaves room


def test_kernel_bit_is_one_shift_everywhere():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "velesdb_hip.h")).read()
    rs = open(os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")).read()
    assert re.search(r"#define\s+VDB_KERNEL_SELECT_HALF_L2\s+\(1u << 23\)", hdr)
    assert re.search(r"pub const VDB_KERNEL_SELECT_HALF_L2: i32 = 1 << 23;", rs)
    assert va.KERNEL_SELECT_HALF_L2 == _ffi.VDB_KERNEL_SELECT_HALF_L2 == 1 << 23 == 2 * _ffi.VDB_KERNEL_HYBRID_FUSE
