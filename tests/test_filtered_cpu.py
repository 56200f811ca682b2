"""Filtered exact search (vdb_hip_index_search_batch_filtered), the part that needs no GPU: the three new entry
points and the new constants agree between the header, the ctypes table and the Rust raw bindings; without a device the filter
constructor fails with a status and a message; the listed kernels in the built library hold no scratch, spill nothing and use
no dynamic stack; and the route rule (velesdb_amd/csrc/vdb_filter_route.hpp, compiled stand-alone) holds at its boundaries."""
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
NEW = ("vdb_hip_index_filter_create", "vdb_hip_filter_destroy", "vdb_hip_index_search_batch_filtered")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"(\w[\w ]*?[\s\*]+)" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in velesdb_hip.h"
    return m.group(1).strip(), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype_of(c_decl):
    """ctypes type of one C parameter declaration, by the convention of velesdb_amd/_ffi.py (typed pointers for the small out
    parameters, void pointers for buffers: both are pointers, which is what is compared)"""
    t = c_decl.rsplit(" ", 1)[0] if re.search(r"[A-Za-z_0-9]$", c_decl) else c_decl
    if "*" in c_decl:
        return "pointer"
    return {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[t.replace("const ", "").strip()]


def test_ffi_signatures_match_the_header():
    from velesdb_amd import _ffi
    for name in NEW:
        ret, args = _header_args(name)
        res, argtypes = _ffi.SIGNATURES[name]
        assert (res is None) == (ret == "void"), name
        if res is not None:
            assert res is C.c_int32 and ret == "int32_t", name
        assert len(argtypes) == len(args), (name, args)
        for decl, at in zip(args, argtypes):
            want = _ctype_of(decl)
            if want == "pointer":
                assert at is C.c_void_p or issubclass(at, C._Pointer), (name, decl, at)
            else:
                assert at is want, (name, decl, at)
    # the filter's out parameter is a pointer to a pointer, `matched` a pointer to u64
    assert _ffi.SIGNATURES["vdb_hip_index_filter_create"][1][4] is C.POINTER(C.c_uint64)
    assert _ffi.SIGNATURES["vdb_hip_index_filter_create"][1][5] is C.POINTER(C.c_void_p)


def test_library_exports_the_new_entry_points():
    from velesdb_amd import _ffi
    L = C.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name


def test_new_constants_agree_everywhere():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", _header()))
    rs = dict((k, int(v)) for k, v in re.findall(r"pub const (VDB_[A-Z0-9_]+): (?:i32|usize) = (-?\d+);", open(RUST_SYS).read()))
    want = {"VDB_OPT_FILTER_ROUTE": 8, "VDB_OPT_COUNT_": 9, "VDB_KERNEL_SWEEP_LISTED": 65536}
    for k, v in want.items():
        assert enums[k] == v, (k, enums.get(k))
        assert rs[k] == v, (k, rs.get(k))
        assert getattr(_ffi, k) == v, k
    assert va.OPT_FILTER_ROUTE == 8 and va.KERNEL_SWEEP_LISTED == 65536
    # the kernel bit is a bit of its own
    bits = [v for k, v in enums.items() if k.startswith("VDB_KERNEL_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)


def test_rust_wrapper_reaches_the_new_entry_points():
    lib = open(RUST_LIB).read()
    used = set(re.findall(r"sys::(vdb_hip_[a-z0-9_]+)", lib))
    assert set(NEW) <= used
    for item in ("pub struct HipFilter", "impl Drop for HipFilter", "pub fn create_filter", "pub fn search_brute_force_filtered",
                 "pub fn search_batch_brute_force_filtered"):
        assert item in lib, item


def test_filter_create_without_a_device_is_a_loud_failure():
    """No device: no index can exist, so the constructor is reached with what a caller without a GPU has in hand — it answers a
    status and a message (and leaves its outputs cleared), it does not crash."""
    import velesdb_amd as va
    from velesdb_amd import _ffi
    if va.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(va.VelesHipError) as e:
        va.HnswIndex(8, va.DistanceMetric.Cosine)
    assert e.value.code == _ffi.VDB_ERR_NO_DEVICE
    L = _ffi.lib()
    ids = np.arange(4, dtype=np.uint64)
    h, m = C.c_void_p(0x1234), C.c_uint64(99)
    rc = L.vdb_hip_index_filter_create(None, ids.ctypes.data_as(C.c_void_p), 4, 0, C.byref(m), C.byref(h))
    assert rc < 0 and _ffi.last_error() != ""
    assert h.value is None and m.value == 0
    out_n = np.zeros(1, np.uint32)
    q = np.zeros(8, np.float32)
    rc = L.vdb_hip_index_search_batch_filtered(None, None, q.ctypes.data_as(C.c_void_p), 1, 1, 1, None, None, out_n.ctypes.data_as(C.c_void_p))
    assert rc == _ffi.VDB_ERR_INVALID_ARG and _ffi.last_error() != ""
    L.vdb_hip_filter_destroy(None)  # a null filter is a no-op


def test_listed_kernels_hold_no_scratch_and_spill_nothing():
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = [k for k in kr.kernels() if kr.family(k["name"]) in ("sweep_topk_listed", "sweep_topk_listed_m", "filter_mask_kernel")]
    fams = {kr.family(k["name"]) for k in ks}
    assert fams == {"sweep_topk_listed", "sweep_topk_listed_m", "filter_mask_kernel"}, fams
    # 3 metrics x B in (1, 4, 8) x CPL in (0 .. 4) mode-C instances, Cosine and DotProduct mode-M instances
    assert sum(kr.family(k["name"]) == "sweep_topk_listed" for k in ks) == 45
    assert sum(kr.family(k["name"]) == "sweep_topk_listed_m" for k in ks) == 2
    for k in ks:  # (kr.kernels() itself asserts wave64 for every kernel of the library)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
        assert k["vgpr"] <= kr.REGS_PER_LANE, k
    if os.path.exists(kr.OBJDUMP):  # explicit global_ / ds_ accesses: no FLAT instruction in any of them
        objs = kr.code_objects()
        for oi in {k["obj"] for k in ks}:
            funcs = kr.disassemble(objs[oi])
            for k in ks:
                if k["obj"] == oi:
                    ins = [x for _, b in funcs[k["symbol"]] for x in b]
                    assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                    assert kr.count(ins, "global_load") > 0, k["name"]


@pytest.mark.timeout(120)
def test_route_rule_at_its_boundaries(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filter_route_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "filter_route_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] > 1000
