"""Filtered graph search (vdb_hip_index_search_graph_filtered), the part that needs no GPU: the entry point and the
two kernel bits agree between the header, the ctypes table and the Rust raw bindings; the safe Rust wrapper reaches the symbol;
without a device the call fails with a status; and the route rule (filter_graph_route in velesdb_amd/csrc/vdb_filter_route.hpp,
compiled stand-alone) holds at its boundaries."""
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
NAME = "vdb_hip_index_search_graph_filtered"
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
    assert [a.split()[-1].lstrip("*") for a in args] == ["idx", "f", "queries_rowmajor", "nq", "k", "ef", "mode", "route", "max_list", "out_ids",
                                                         "out_scores", "out_n", "out_route"]
    res, argtypes = _ffi.SIGNATURES[NAME]
    assert res is C.c_int32 and len(argtypes) == len(args)
    m = re.search(r"pub fn " + NAME + r"\(([^)]*)\) -> i32;", open(RUST_SYS).read())
    assert m, "sys.rs does not declare the entry point"
    rust = [a.split(":")[1].strip() for a in m.group(1).split(",")]
    assert len(rust) == len(args)
    for decl, at, rt in zip(args, argtypes, rust):
        if "*" in decl:
            assert at is C.c_void_p or issubclass(at, C._Pointer), (decl, at)
            assert rt.startswith("*const ") == ("const" in decl) and rt.startswith(("*const ", "*mut ")), (decl, rt)
        else:
            t = decl.rsplit(" ", 1)[0]
            assert at is C_TYPES[t] and rt == RUST_TYPES[t], (decl, at, rt)


def test_library_exports_the_entry_point():
    from velesdb_amd import _ffi
    assert hasattr(C.CDLL(_ffi.LIB_PATH), NAME)


def test_kernel_bits_agree_everywhere():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", _header()))
    rs = dict((k, int(v)) for k, v in re.findall(r"pub const (VDB_[A-Z0-9_]+): (?:i32|usize) = (-?\d+);", open(RUST_SYS).read()))
    for k, v in {"VDB_KERNEL_HNSW_FILTERED": 131072, "VDB_KERNEL_FILTER_RANK": 262144}.items():
        assert enums[k] == v and rs[k] == v and getattr(_ffi, k) == v, k
    assert va.KERNEL_HNSW_FILTERED == 131072 and va.KERNEL_FILTER_RANK == 262144
    assert (va.ROUTE_AUTO, va.ROUTE_WALK, va.ROUTE_EXACT) == (0, 1, 2)
    bits = [v for k, v in enums.items() if k.startswith("VDB_KERNEL_")]
    assert len(set(bits)) == len(bits) and all(b > 0 and b & (b - 1) == 0 for b in bits)
    assert enums["VDB_OPT_COUNT_"] == 9  # route and max_list travel with the call: no new option


def test_rust_wrapper_reaches_the_entry_point():
    lib = open(RUST_LIB).read()
    assert NAME in set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    for item in ("pub fn search_batch_graph_filtered", "pub fn search_graph_filtered", "filter: &HipFilter"):
        assert item in lib, item


def test_call_without_a_device_is_a_status():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(va.VelesHipError) as e:
        va.HnswIndex(8, va.DistanceMetric.Cosine)
    assert e.value.code == _ffi.VDB_ERR_NO_DEVICE  # no index can exist: this is how the call fails on a machine without a GPU
    L = _ffi.lib()
    q, out_n = np.zeros(8, np.float32), np.zeros(1, np.uint32)
    rc = L.vdb_hip_index_search_graph_filtered(None, None, q.ctypes.data_as(C.c_void_p), 1, 1, 0, 2, 0, 0, None, None,
                                               out_n.ctypes.data_as(C.c_void_p), None)
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != ""


@pytest.mark.timeout(120)
def test_graph_route_rule_at_its_boundaries(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filter_graph_route_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "filter_graph_route_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 10000
