"""The fused searches with one optional filter per query over every rows form (vdb_hip_index_hybrid_search_filters,
vdb_hip_index_multi_query_search_filters), the part that needs no GPU: the two entry points agree between the header, the
ctypes table and the Rust raw bindings; enum vdb_walk_rows is the same in all of them; the library exports the symbols and the
wrappers reach them; without a device a call answers a status and leaves its outputs alone; and the plan of the two phases
(fused_phases_plan in velesdb_amd/csrc/vdb_filter_route.hpp, compiled stand-alone with ASan + UBSan) holds at its boundaries."""
import ctypes as C
import inspect
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
HYBRID, MULTI = "vdb_hip_index_hybrid_search_filters", "vdb_hip_index_multi_query_search_filters"
PARAMS = {
    HYBRID: ["idx", "rows", "oversampling_ratio", "filters", "n_filters", "filter_of_query", "queries_rowmajor", "nq", "k", "text_ids", "text_n",
             "text_stride", "vector_weights", "out_ids", "out_scores", "out_n"],
    MULTI: ["idx", "rows", "oversampling_ratio", "filters", "n_filters", "filter_of_group", "queries_rowmajor", "group_sizes", "n_groups", "top_k",
            "strategy", "rrf_k", "weights", "out_ids", "out_scores", "out_n"],
}
C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RUST_TYPES = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}
ROWS = {"VDB_WALK_ROWS_F32": 0, "VDB_WALK_ROWS_F16": 1, "VDB_WALK_ROWS_BF16": 2, "VDB_WALK_ROWS_INT8": 3, "VDB_WALK_ROWS_F16_RESCORE": 4,
        "VDB_WALK_ROWS_BF16_RESCORE": 5}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", [HYBRID, MULTI])
def test_signature_agrees_in_header_ctypes_and_rust(name):
    from velesdb_amd import _ffi
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in velesdb_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == PARAMS[name]
    assert args[3] == "void** filters"  # the table's shape is vdb_hip_index_search_graph_filters's
    assert name in _ffi.SIGNATURES, "the ctypes table does not declare the entry point"
    res, argtypes = _ffi.SIGNATURES[name]
    assert res is C.c_int32 and len(argtypes) == len(args)
    r = re.search(r"pub fn " + name + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
    assert r, "sys.rs does not declare the entry point"
    rust = [a.split(":")[1].strip() for a in r.group(1).split(",")]
    assert len(rust) == len(args)
    for decl, at, rt in zip(args, argtypes, rust):
        if "**" in decl:
            assert at is C.c_void_p and rt == "*mut *mut c_void", (decl, at, rt)
        elif "*" in decl:
            assert at is C.c_void_p, (decl, at)
            assert rt.startswith("*const ") == ("const" in decl) and rt.startswith(("*const ", "*mut ")), (decl, rt)
        else:
            t = decl.rsplit(" ", 1)[0]
            assert at is C_TYPES[t] and rt == RUST_TYPES[t], (decl, at, rt)


def test_walk_rows_are_the_same_everywhere():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_WALK_ROWS_[A-Z0-9_]+)\s*=\s*(\d+)", _header()))
    assert enums == ROWS
    rs = dict((k, int(v)) for k, v in re.findall(r"pub const (VDB_WALK_ROWS_[A-Z0-9_]+): i32 = (\d+);", open(RUST_SYS).read()))
    assert rs == ROWS
    for name, v in ROWS.items():
        assert getattr(_ffi, name) == v and getattr(va, name[4:]) == v, name
    # ... and they are the library's internal numbering of the filtered walks
    hpp = open(os.path.join(ROOT, "velesdb_amd", "csrc", "vdb_index.hpp")).read()
    internal = re.search(r"enum FiltersRows : int \{([^}]*)\}", hpp).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", internal)] == sorted(ROWS.values())


def test_library_exports_the_entry_points_and_the_wrappers_reach_them():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    L = C.CDLL(_ffi.LIB_PATH)
    lib = open(RUST_LIB).read()
    used = set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    for name in (HYBRID, MULTI):
        assert hasattr(L, name), name
        assert name in used, name
    for item in ("pub fn hybrid_search_batch_filters", "pub fn multi_query_search_batch_filters"):
        assert item in lib, item
    assert list(inspect.signature(va.HnswIndex.hybrid_search_batch_filters).parameters)[1:] == [
        "queries", "text_hits", "k", "vector_weight", "filters", "rows", "oversampling"]
    assert list(inspect.signature(va.HnswIndex.multi_query_search_batch_filters).parameters)[1:] == [
        "groups", "top_k", "fusion", "filters", "rows", "oversampling"]


def test_the_one_filter_kernel_and_the_rule_header_keep_their_names():
    """hybrid_fuse_kernel and vdb_hybrid.hpp's functions are what tests/hybrid_model.cpp and tests/test_hybrid_cpu.py compile and name;
    the per-query kernel shares the body instead of copying it."""
    src = open(os.path.join(ROOT, "velesdb_amd", "csrc", "hybrid.hip")).read()
    assert re.search(r"__global__ void __launch_bounds__\(1024\) hybrid_fuse_kernel\(const HybridArgs a\)", src)
    assert re.search(r"__global__ void __launch_bounds__\(1024\) hybrid_fuse_filters_kernel\(const HybridFiltersArgs fa\)", src)
    assert src.count("hybrid::fuse_run(") == 1 and src.count("hybrid_fuse_block(") == 3  # one body, two callers
    rule = open(os.path.join(ROOT, "velesdb_amd", "csrc", "vdb_hybrid.hpp")).read()
    for fn in ("weight_valid", "clamp_weight", "text_weight", "term", "text_ranked", "rec_of", "fuse_run", "fused_of", "fused_score_bits",
               "fused_less", "fused_pad"):
        assert re.search(r"\b" + fn + r"\(", rule), fn


def test_calls_without_a_device_are_statuses():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _ffi.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    q, out_n, fq, tn = np.zeros(8, np.float32), np.full(1, 77, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    rc = L.vdb_hip_index_hybrid_search_filters(None, 0, 0, None, 0, vp(fq), vp(q), 1, 0, None, vp(tn), 0, None, None, None, vp(out_n))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != "" and out_n[0] == 77
    sizes = np.ones(1, np.uint32)
    rc = L.vdb_hip_index_multi_query_search_filters(None, 0, 0, None, 0, vp(fq), vp(q), vp(sizes), 1, 0, 2, 60, None, None, None, vp(out_n))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != "" and out_n[0] == 77


@pytest.mark.timeout(180)
def test_plan_of_the_two_phases_holds_at_its_boundaries(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hybrid_filters_plan_model")
    # (the sanitizer runtimes are linked into the program: it runs in whatever environment the suite runs in)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "hybrid_filters_plan_model.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=150, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 8000
    # the tables reached what the plan is for: calls past the limit, calls with an empty phase, calls with both phases
    assert line["over"] > 500 and line["empty_phases"] > 1000 and line["mixed"] > 500, line
