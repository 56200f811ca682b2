"""One filter per query in one graph call (vdb_hip_index_search_graph_filters), the part that needs no GPU: the entry
point agrees between the header, the ctypes table and the Rust raw bindings; the library exports it; the safe Rust wrapper and the
Python method reach it; without a device the call fails with a status; and the launch plan (filters_plan_round /
filters_walk_ladders in velesdb_amd/csrc/vdb_filter_route.hpp, compiled stand-alone) keeps every query on the ladder it climbs alone
— and runs a call whose queries all share one filter as the one-filter call's own host loop ran it."""
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
NAME = "vdb_hip_index_search_graph_filters"
C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RUST_TYPES = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_args():
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in velesdb_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_signature_agrees_in_header_ctypes_and_rust():
    from velesdb_amd import _ffi
    args = _header_args()
    assert [a.split()[-1].lstrip("*") for a in args] == ["idx", "filters", "n_filters", "filter_of_query", "queries_rowmajor", "nq", "k", "ef",
                                                         "mode", "route", "max_list", "out_ids", "out_scores", "out_n", "out_route"]
    assert args[1] == "void** filters"  # (the pointer shape the ABI tests' header parser understands)
    res, argtypes = _ffi.SIGNATURES[NAME]
    assert res is C.c_int32 and len(argtypes) == len(args)
    m = re.search(r"pub fn " + NAME + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
    assert m, "sys.rs does not declare the entry point"
    rust = [a.split(":")[1].strip() for a in m.group(1).split(",")]
    assert len(rust) == len(args)
    for decl, at, rt in zip(args, argtypes, rust):
        if "**" in decl:
            assert at is C.c_void_p and rt == "*mut *mut c_void", (decl, at, rt)
        elif "*" in decl:
            assert at is C.c_void_p or issubclass(at, C._Pointer), (decl, at)
            assert rt.startswith("*const ") == ("const" in decl) and rt.startswith(("*const ", "*mut ")), (decl, rt)
        else:
            t = decl.rsplit(" ", 1)[0]
            assert at is C_TYPES[t] and rt == RUST_TYPES[t], (decl, at, rt)


def test_no_new_option_and_no_new_kernel_bit():
    from velesdb_amd import _ffi
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", _header()))
    assert enums["VDB_OPT_COUNT_"] == 9
    bits = sorted(v for k, v in enums.items() if k.startswith("VDB_KERNEL_"))
    assert bits[-1] == _ffi.VDB_KERNEL_FILTER_RANK == 262144  # the per-query kernels report the two existing families' bits


def test_library_exports_the_entry_point():
    from velesdb_amd import _ffi
    assert hasattr(C.CDLL(_ffi.LIB_PATH), NAME)


def test_wrappers_reach_the_entry_point():
    lib = open(RUST_LIB).read()
    assert NAME in set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    for item in ("pub fn search_batch_with_filters", "filters: &[Option<&HipFilter>]", "does not match filters count"):
        assert item in lib, item
    import velesdb_amd as va
    assert callable(va.HnswIndex.search_batch_with_filters)


def test_call_without_a_device_is_a_status():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _ffi.lib()
    q, out_n, fq = np.zeros(8, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    rc = L.vdb_hip_index_search_graph_filters(None, None, 0, fq.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), 1, 1, 0, 2, 0, 0,
                                              None, None, out_n.ctypes.data_as(C.c_void_p), None)
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != ""


@pytest.mark.timeout(180)
def test_launch_plan_keeps_every_query_on_its_own_ladder(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filters_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "filters_plan_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=150, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 10000
    # the generated calls reached what the plan is for: rounds of several launches, launches whose queries differ in list capacity,
    # re-runs, and calls that fail as a whole
    assert min(line["split_rounds"], line["mixed_launches"], line["rerun_rounds"], line["failed_calls"]) > 1000, line
    # ... and the calls with every query on one filter — held to the host loop the one-filter call once had — reached re-runs, exact
    # passes behind the largest list, whole-call exact passes and refusals
    assert line["one_filter_cases"] > 10000, line
    assert min(line["one_filter_rerun_rounds"], line["one_filter_exact_after_walk"], line["one_filter_exact_calls"],
               line["one_filter_failed_calls"]) > 1000, line
