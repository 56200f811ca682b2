"""The gathered four-bit tier of filtered search over packed bits, on the CPU: the new kernel bit in every binding, the
launch plan at its boundaries (csrc/vdb_filter_route.hpp bits_gather_plan through tests/bits_gather_plan_model.cpp, built stand-alone
with ASan + UBSan), and the instances' resources in the built library."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_the_bit_in_every_binding():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "velesdb_hip.h")).read()
    rs = open(os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")).read()
    assert re.search(r"#define\s+VDB_KERNEL_BITS_GATHERED\s+\(1u << 25\)", hdr)
    assert "pub const VDB_KERNEL_BITS_GATHERED: i32 = 1 << 25;" in rs
    assert va.KERNEL_BITS_GATHERED == _ffi.VDB_KERNEL_BITS_GATHERED == 1 << 25 == 2 * _ffi.VDB_KERNEL_GEMM_HALF_GATHERED


def test_plan_boundaries(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import velesdb_amd as va
    exe = str(tmp_path / "bits_gather_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "bits_gather_plan_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)   # the binary links its own sanitizer runtime

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=100, env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return json.loads(r.stdout.strip().splitlines()[-1])
    line = run()
    assert line["failed_checks"] == 0 and line["cases"] > 5_000 and 64 < line["first_k_16"] < line["first_k_none"]
    kn = line["first_k_none"]
    for k, count, nq, n_cus in [(10, 1000, 1024, 256), (64, 65, 130, 256), (kn - 1, 1500, 3, 256), (kn, 1500, 3, 256), (500, 9000, 17, 1)]:
        want, got = run(k, count, nq, n_cus), va.bits_gather_plan(k, count, nq, n_cus)   # (the package's restatement, used by the GPU test)
        assert (got is None) if want["blocks"] == 0 else (got == {key: want[key] for key in got}), (k, count, nq, n_cus)


def test_instances_hold_no_scratch_no_spill_no_dynamic_stack():
    pytest.importorskip("msgpack")
    import kernel_resources as kr
    if not os.path.exists(kr.LIB):
        pytest.skip("library not built")
    ks = [k for k in kr.kernels() if kr.family(k["name"]) == "sweep_topk_bits_gathered"]
    assert sorted(re.search(r"<(.*)>", k["name"]).group(1) for k in ks) == sorted("%d, %d" % (m, tn) for m in (3, 4) for tn in (16, 128))
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"] and k["waves_per_simd"] >= 2, k
