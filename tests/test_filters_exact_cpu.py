"""One filter per query on the exact sweep (vdb_hip_index_search_batch_filters), the part that needs no GPU: the
entry point and its diagnostic agree between the header, the ctypes table and the Rust raw bindings; the library exports them and
the wrappers reach the call; without a device the call answers a status; no option was added and the new kernel bit is the macro
2097152; the grouped kernel families are in the built library without scratch, spills or FLAT accesses, at the resource bars the
plan assumes; and the plan (filters_exact_groups / listed_groups_plan in velesdb_amd/csrc/vdb_filter_route.hpp, compiled
stand-alone with ASan + UBSan) covers every (query, list position) exactly once."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "velesdb_hip.h")
RUST_SYS = os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")
RUST_LIB = os.path.join(ROOT, "velesdb-hip", "src", "lib.rs")
NAME = "vdb_hip_index_search_batch_filters"
DIAG = "vdb_hip_index_last_filters_exact_plan"
C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RUST_TYPES = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in velesdb_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,want", [
    (NAME, ["idx", "filters", "n_filters", "filter_of_query", "queries_rowmajor", "nq", "k", "mode", "out_ids", "out_scores", "out_n"]),
    (DIAG, ["idx", "out"])])
def test_signature_agrees_in_header_ctypes_and_rust(name, want):
    from velesdb_amd import _ffi
    args = _header_args(name)
    assert [a.split()[-1].lstrip("*") for a in args] == want
    if name == NAME:
        assert args[1] == "void** filters"  # the table's shape is vdb_hip_index_search_graph_filters's
    res, argtypes = _ffi.SIGNATURES[name]
    assert res is C.c_int32 and len(argtypes) == len(args)
    m = re.search(r"pub fn " + name + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
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


def test_no_new_option_and_the_new_kernel_bit_is_a_macro():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    h = _header()
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", h))
    assert enums["VDB_OPT_COUNT_"] == 9 and _ffi.VDB_OPT_COUNT_ == 9
    assert "VDB_KERNEL_SWEEP_LISTED_GROUPS" not in enums  # beside the enum: VDB_KERNEL_FILTER_RANK stays its last member
    defines = dict((k, int(v)) for k, v in re.findall(r"#define\s+(VDB_[A-Z0-9_]+)\s+(\d+)", h))
    assert defines["VDB_KERNEL_SWEEP_LISTED_GROUPS"] == 2097152
    rs = dict((k, int(v)) for k, v in re.findall(r"pub const (VDB_[A-Z0-9_]+): (?:i32|usize) = (-?\d+);", open(RUST_SYS).read()))
    assert rs["VDB_KERNEL_SWEEP_LISTED_GROUPS"] == 2097152 and rs["VDB_OPT_COUNT_"] == 9
    assert _ffi.VDB_KERNEL_SWEEP_LISTED_GROUPS == 2097152 and va.KERNEL_SWEEP_LISTED_GROUPS == 2097152
    bits = [v for k, v in list(enums.items()) + list(defines.items()) if k.startswith("VDB_KERNEL_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)  # a bit of its own


def test_library_exports_the_entry_points():
    from velesdb_amd import _ffi
    L = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(L, NAME) and hasattr(L, DIAG)


def test_wrappers_reach_the_entry_point():
    lib = open(RUST_LIB).read()
    used = set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    assert NAME in used and DIAG in used
    for item in ("pub fn search_batch_brute_force_with_filters", "pub fn last_filters_exact_plan", "filters: &[Option<&HipFilter>]"):
        assert item in lib, item
    import velesdb_amd as va
    assert callable(va.HnswIndex.search_batch_brute_force_with_filters) and callable(va.HnswIndex.last_filters_exact_plan)


def test_call_without_a_device_is_a_status():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _ffi.lib()
    q, out_n, fq = np.zeros(8, np.float32), np.full(1, 77, np.uint32), np.zeros(1, np.uint32)
    rc = L.vdb_hip_index_search_batch_filters(None, None, 0, fq.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), 1, 1, 1, None, None,
                                              out_n.ctypes.data_as(C.c_void_p))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != "" and out_n[0] == 77
    plan = (C.c_uint32 * 6)()
    assert L.vdb_hip_index_last_filters_exact_plan(None, plan) == _ffi.VDB_ERR_INVALID_ARG


def _kernels():
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    return kr, kr.kernels()


def test_grouped_kernels_hold_no_scratch_and_spill_nothing():
    kr, allk = _kernels()
    ks = [k for k in allk if kr.family(k["name"]) in ("sweep_topk_listed_groups", "sweep_topk_listed_groups_m")]
    # 3 metrics x B in (1, 4, 8) x CPL in (0 .. 4) mode-C instances, Cosine and DotProduct mode-M instances — families of their own:
    # the one-filter families keep their instance counts (tests/test_filtered_cpu.py)
    assert sum(kr.family(k["name"]) == "sweep_topk_listed_groups" for k in ks) == 45
    assert sum(kr.family(k["name"]) == "sweep_topk_listed_groups_m" for k in ks) == 2
    assert sum(kr.family(k["name"]) == "sweep_topk_listed" for k in allk) == 45
    assert sum(kr.family(k["name"]) == "sweep_topk_listed_m" for k in allk) == 2
    for k in ks:
        assert k["block"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and not k["dynamic_stack"], k
        assert k["vgpr"] <= kr.REGS_PER_LANE, k
    if os.path.exists(kr.OBJDUMP):  # the work-item table is read with plain loads, everything written goes through vector stores
        objs = kr.code_objects()
        for oi in {k["obj"] for k in ks}:
            funcs = kr.disassemble(objs[oi])
            for k in ks:
                if k["obj"] == oi:
                    ins = [x for _, b in funcs[k["symbol"]] for x in b]
                    assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                    assert kr.count(ins, "global_load") > 0 and kr.count(ins, "global_store") > 0, k["name"]


def test_mode_m_grouped_kernel_stays_at_the_one_filter_kernels_registers():
    """mode M: at or under the VGPR count of the one-filter mode-M kernel (98 when this route was written), four blocks per CU,
    and the LDS is the launch's dynamic allocation only (the 160 KB budget is the plan's: listed_m_lds_bytes)"""
    kr, allk = _kernels()
    one = {k["name"].split("<")[1]: k for k in allk if kr.family(k["name"]) == "sweep_topk_listed_m"}
    grp = {k["name"].split("<")[1]: k for k in allk if kr.family(k["name"]) == "sweep_topk_listed_groups_m"}
    assert sorted(one) == sorted(grp) and len(grp) == 2
    for inst, k in grp.items():
        assert k["vgpr"] <= one[inst]["vgpr"] <= 98, (k, one[inst])
        assert k["waves_per_simd"] >= 4 and k["lds"] == 0, k


def _mode_c_instances():
    kr, allk = _kernels()
    one = {k["name"].split("<")[1]: k for k in allk if kr.family(k["name"]) == "sweep_topk_listed"}
    grp = {k["name"].split("<")[1]: k for k in allk if kr.family(k["name"]) == "sweep_topk_listed_groups"}
    assert sorted(one) == sorted(grp) and len(grp) == 45
    return one, grp


def test_mode_c_grouped_kernels_are_never_below_their_one_filter_instance():
    """the two families share one arithmetic body: resident blocks per CU (= waves per SIMD at 256 threads) of a grouped instance
    are at least those of the one-filter instance <METRIC, B, CPL>, and its VGPR count is within two of it"""
    one, grp = _mode_c_instances()
    for inst, k in sorted(grp.items()):
        assert k["waves_per_simd"] >= one[inst]["waves_per_simd"] and k["vgpr"] <= one[inst]["vgpr"] + 2, (k, one[inst])


def test_mode_c_grouped_kernels_keep_the_occupancy_the_plan_assumes():
    """mode C: resident 256-thread blocks per CU at or above what sweep_listed_plan / listed_groups_plan size their launches by —
    4, 3, 2 for B = 1, 4, 8.

    Six instances would sit under it with the 4 rows in flight of the one-filter kernels (as their one-filter instances do:
    <0, 1, 4>, <2, 1, 4>, <1, 1, 2>, <1, 1, 3>, <1, 1, 4> at 3 blocks, <1, 4, 4> at 2); the grouped kernels fetch 2 rows (1 for
    <1, 4, 4>) at a time there — the chains are the same — and reach it without scratch (listed_rows_in_flight, sweep_listed.hip)."""
    _, grp = _mode_c_instances()
    low = []
    for inst, k in sorted(grp.items()):
        B = int(inst.split(",")[1])
        if k["waves_per_simd"] < {1: 4, 4: 3, 8: 2}[B]:
            low.append((inst, k["vgpr"], k["waves_per_simd"]))
    assert not low, low


@pytest.mark.timeout(180)
def test_plan_covers_every_query_and_list_position_once(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "listed_groups_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "listed_groups_plan_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=150, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 2000
    # the generated tables reached what the plan is for: groups on both routes, many work items, launches held by the list cap
    assert min(line["listed_groups"], line["dense_groups"]) > 10000 and line["items"] > 100000 and line["capped"] > 50, line
