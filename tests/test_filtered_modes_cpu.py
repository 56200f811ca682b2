"""Filtered exact search over the SQ8 / Binary / half images (vdb_hip_index_search_batch_filtered_mode), the part that
needs no GPU: the new entry point agrees between the header, the ctypes table and the Rust raw bindings and is exported; the route
rule and the plan of the listed passes (velesdb_amd/csrc/vdb_filter_route.hpp, compiled stand-alone under ASan + UBSan) hold at their
boundaries; the Python wrappers validate their arguments before they reach the library."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "velesdb_hip.h")
RUST_SYS = os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")
RUST_LIB = os.path.join(ROOT, "velesdb-hip", "src", "lib.rs")
NAME = "vdb_hip_index_search_batch_filtered_mode"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_entry_point_is_declared_bound_and_exported():
    from velesdb_amd import _ffi
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in velesdb_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["vdb_hip_index* idx", "const void* f", "int32_t mode", "const float* queries_rowmajor", "uint32_t nq", "uint32_t k",
                    "uint64_t* out_ids", "float* out_scores", "uint32_t* out_n"]
    res, argtypes = _ffi.SIGNATURES[NAME]
    assert res is C.c_int32 and len(argtypes) == len(args)
    for decl, at in zip(args, argtypes):
        if "*" in decl:
            assert at is C.c_void_p or issubclass(at, C._Pointer), (decl, at)
        else:
            assert at is {"int32_t": C.c_int32, "uint32_t": C.c_uint32}[decl.split()[0]], (decl, at)
    assert hasattr(C.CDLL(_ffi.LIB_PATH), NAME)
    rs = re.search(r"pub fn " + NAME + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
    assert rs, "sys.rs does not declare the entry point"
    assert [a.split(":")[1].strip() for a in rs.group(1).split(",")] == ["*mut VdbHipIndex", "*const c_void", "i32", "*const f32", "u32", "u32",
                                                                         "*mut u64", "*mut f32", "*mut u32"]
    lib = open(RUST_LIB).read()
    assert "sys::" + NAME in lib and "pub fn search_batch_filtered_mode" in lib


def test_null_arguments_are_refused_without_a_device():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _ffi.lib()
    q, out_n = np.zeros(8, np.float32), np.full(1, 7, np.uint32)
    rc = L.vdb_hip_index_search_batch_filtered_mode(None, None, va.MODE_BRUTE_SQ8, q.ctypes.data_as(C.c_void_p), 1, 1, None, None,
                                                    out_n.ctypes.data_as(C.c_void_p))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != "" and out_n[0] == 7


def test_python_wrappers_validate_before_they_call():
    """A handle-less HnswIndex object (no device needed): the wrappers refuse a wrong filter object, a wrong query shape, a negative k
    and the F32 precision before anything reaches the library (the null handle would be refused there)."""
    import velesdb_amd as va
    ix = object.__new__(va.HnswIndex)
    ix._h, ix._dimension = None, 8
    flt = va.Filter(None, 0)
    good = np.zeros((2, 8), np.float32)
    for call in (ix.search_batch_filtered_sq8, ix.search_batch_filtered_binary, lambda q, k, f: ix.search_batch_filtered_half(q, k, f, va.VectorPrecision.F16),
                 lambda q, k, f: ix.search_batch_filtered_half(q, k, f, va.VectorPrecision.BF16)):
        with pytest.raises(TypeError):
            call(good, 3, None)
        with pytest.raises(TypeError):
            call(good, 3, "not a filter")
        with pytest.raises(AssertionError, match="dimension mismatch"):
            call(np.zeros((2, 7), np.float32), 3, flt)
        with pytest.raises(AssertionError, match="dimension mismatch"):
            call(np.zeros(9, np.float32), 3, flt)
        with pytest.raises(ValueError):
            call(np.zeros((2, 2, 8), np.float32), 3, flt)
        with pytest.raises(ValueError):
            call(good, -1, flt)
    with pytest.raises(ValueError):
        ix.search_batch_filtered_half(good, 3, flt, va.VectorPrecision.F32)


@pytest.mark.timeout(120)
def test_route_rule_and_listed_plan_at_their_boundaries(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filter_mode_route_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "filter_mode_route_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 10000
