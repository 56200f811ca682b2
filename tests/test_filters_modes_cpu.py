"""One filter per query over the SQ8 codes, the sign bits and the half images (vdb_hip_index_search_batch_filters_mode),
the part that needs no GPU: the entry point agrees between the header, the ctypes table and the Rust raw bindings; the library
exports it and the wrappers reach it; without a device the call answers a status; the header carries the contract; no option and
no kernel bit was added; and the plan (filters_mode_groups / mode_groups_plan in velesdb_amd/csrc/vdb_filter_route.hpp, compiled
stand-alone with ASan + UBSan) gives every listed query exactly the passes the one-filter plan gives its group."""
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
NAME = "vdb_hip_index_search_batch_filters_mode"
C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RUST_TYPES = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_signature_agrees_in_header_ctypes_and_rust():
    from velesdb_amd import _ffi
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in velesdb_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["idx", "filters", "n_filters", "filter_of_query", "mode", "queries_rowmajor", "nq", "k",
                                                         "out_ids", "out_scores", "out_n"]
    assert args[1] == "void** filters"  # the table's shape is vdb_hip_index_search_batch_filters's
    res, argtypes = _ffi.SIGNATURES[NAME]
    assert res is C.c_int32 and len(argtypes) == len(args)
    r = re.search(r"pub fn " + NAME + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
    assert r, "sys.rs does not declare the entry point"
    rust = [a.split(":")[1].strip() for a in r.group(1).split(",")]
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


def test_header_carries_the_contract():
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    at = text.index("One filter PER QUERY over the SQ8 codes")
    doc = text[at:text.index("int32_t " + NAME, at)]
    for phrase in ("vdb_hip_index_search_batch_filtered_mode returns for that query ALONE",
                   "what the one-filter mode call returns for its GROUP",
                   "never depends on the query's companions outside its group",
                   "out_n = 0 behind the merge's padding",
                   "posts no selection verdicts, for its unfiltered job too",
                   "VDB_KERNEL_SWEEP_LISTED_GROUPS when a grouped launch ran",
                   "sweep_topk_sq8_listed_groups", "sweep_topk_half_l2_listed_groups",
                   "checked before an empty filter's out_n = 0"):
        assert phrase in doc, phrase
    # the diagnostics name the new call and the new families
    assert "vdb_hip_index_search_batch_filters or vdb_hip_index_search_batch_filters_mode call" in text
    bit = text[text.index("sweep_topk_listed_groups / sweep_topk_listed_groups_m ran"):text.index("#define VDB_KERNEL_SWEEP_LISTED_GROUPS")]
    assert "sweep_topk_sq8_listed_groups" in bit and "sweep_topk_half_l2_listed_groups" in bit


def test_no_new_option_and_no_new_kernel_bit():
    from velesdb_amd import _ffi
    h = _header()
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", h))
    assert enums["VDB_OPT_COUNT_"] == 9 and _ffi.VDB_OPT_COUNT_ == 9
    defines = dict((k, int(v)) for k, v in re.findall(r"#define\s+(VDB_[A-Z0-9_]+)\s+(\d+)", h))
    bits = sorted(v for k, v in list(enums.items()) + list(defines.items()) if k.startswith("VDB_KERNEL_"))
    assert defines["VDB_KERNEL_SWEEP_LISTED_GROUPS"] == 2097152 and max(bits) == defines["VDB_KERNEL_HYBRID_FUSE"] == 4194304


def test_library_exports_the_entry_point_and_the_wrappers_reach_it():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    assert hasattr(C.CDLL(_ffi.LIB_PATH), NAME)
    lib = open(RUST_LIB).read()
    assert NAME in set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    for item in ("pub fn search_batch_with_filters_mode", "pub fn search_batch_brute_force_with_filters", "filters: &[Option<&HipFilter>], mode: i32"):
        assert item in lib, item
    for name in ("search_batch_with_filters_mode", "search_batch_with_filters_sq8", "search_batch_with_filters_binary",
                 "search_batch_brute_force_with_filters_half"):
        assert callable(getattr(va.HnswIndex, name)), name
    # the graph walk over a half image keeps its name and its signature (mode, ef, route, max_list)
    import inspect
    assert list(inspect.signature(va.HnswIndex.search_batch_with_filters_half).parameters)[1:5] == ["queries", "k", "filters", "mode"]


def test_call_without_a_device_is_a_status():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _ffi.lib()
    q, out_n, fq = np.zeros(8, np.float32), np.full(1, 77, np.uint32), np.zeros(1, np.uint32)
    rc = L.vdb_hip_index_search_batch_filters_mode(None, None, 0, fq.ctypes.data_as(C.c_void_p), va.MODE_BRUTE_SQ8, q.ctypes.data_as(C.c_void_p), 1, 1, None, None, out_n.ctypes.data_as(C.c_void_p))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != "" and out_n[0] == 77


@pytest.mark.timeout(180)
def test_plan_gives_every_listed_query_the_passes_of_the_one_filter_plan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mode_groups_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "mode_groups_plan_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=150, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 3000
    # the generated tables reached what the plan is for: groups on both routes, many work items, launches held by the list cap, calls
    # with all three pass widths, tables of one pass (held to mode_listed_plan)
    assert min(line["listed_groups"], line["dense_groups"]) > 10000 and line["items"] > 100000 and line["capped"] > 50, line
    assert line["three_launches"] > 100 and line["one_pass"] > 20, line
