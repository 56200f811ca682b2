"""The gathered matrix-core tier of filtered Cosine / DotProduct calls over a half image, on the CPU: its launch plan
(csrc/vdb_filter_route.hpp half_gather_plan, through tests/half_gather_plan_model.cpp built stand-alone with ASan + UBSan), the Python
restatement of that plan, the new constants in every binding, and the instances' resources in the built library."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hg") / "half_gather_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "half_gather_plan_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)   # the binary links its own sanitizer runtime

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=100, env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return json.loads(r.stdout.strip().splitlines()[-1])
    return run


def test_plan_boundaries(model):
    line = model()
    assert line["failed_checks"] == 0 and line["cases"] > 10_000
    assert 64 < line["first_k_16"] < line["first_k_none"]


@pytest.mark.parametrize("dim,k,count,nq,n_cus", [(768, 10, 1000, 1024, 256), (64, 64, 65, 130, 256), (200, 1, 1, 1, 256), (72, 10, 3000, 17, 1),
                                                  (768, 112, 100_000, 64, 256), (768, 500, 0xFFFFFE00, 5000, 256), (768, 10, 63, 63, 0),
                                                  (768, 1119, 500, 3, 256), (768, 1120, 500, 3, 256), (768, 0, 500, 3, 256)])
def test_python_restatement_follows_the_header(model, dim, k, count, nq, n_cus):
    import velesdb_amd as va
    want, got = model(dim, k, count, nq, n_cus), va.half_gather_plan(dim, k, count, nq, n_cus)
    if want["blocks"] == 0:
        assert got is None
    else:
        assert got == {key: want[key] for key in got} and want["blocks"] == got["spans"] * got["qtiles"]


def test_constants_in_every_binding():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "velesdb_hip.h")).read()
    rs = open(os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")).read()
    assert re.search(r"#define\s+VDB_KERNEL_GEMM_HALF_GATHERED\s+\(1u << 24\)", hdr)
    assert "pub const VDB_KERNEL_GEMM_HALF_GATHERED: i32 = 1 << 24;" in rs
    assert va.KERNEL_GEMM_HALF_GATHERED == _ffi.VDB_KERNEL_GEMM_HALF_GATHERED == 1 << 24 == 2 * _ffi.VDB_KERNEL_SELECT_HALF_L2
    assert (va.FILTER_ROUTE_AUTO, va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK, va.FILTER_ROUTE_GATHERED) == (0, 1, 2, 3)


def test_instances_hold_no_scratch_and_keep_two_waves_per_simd():
    pytest.importorskip("msgpack")
    import kernel_resources as kr
    if not os.path.exists(kr.LIB):
        pytest.skip("library not built")
    ks = [k for k in kr.kernels() if kr.family(k["name"]) == "sweep_topk_half_gathered"]
    assert sorted(re.search(r"<(.*)>", k["name"]).group(1) for k in ks) == sorted(
        "%d, %s, %d" % (m, f, tn) for m in (0, 2) for f in ("true", "false") for tn in (16, 128))
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"] and k["waves_per_simd"] >= 2, k
    if os.path.exists(kr.OBJDUMP):
        objs = kr.code_objects()
        for oi in {k["obj"] for k in ks}:
            funcs = kr.disassemble(objs[oi])
            for k in (k for k in ks if k["obj"] == oi):
                ins = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0 and kr.count(ins, "v_mfma_f32_16x16x32") > 0, k["name"]
