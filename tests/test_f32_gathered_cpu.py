"""The gathered f32 matrix-core tier of filtered Cosine / DotProduct search (FILTER_ROUTE_GATHERED over the f32 rows) on the
CPU: its diagnostic bit in the header and the bindings, no new option, the header's words for the filtered call, and what the compiler
made of sweep_topk_f32_gathered (tools/kernel_resources.py, as tests/test_kernel_resources_cpu.py reads it)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADER = open(os.path.join(ROOT, "include", "velesdb_hip.h")).read()


def test_the_bit_is_a_shift_in_the_header_and_in_every_binding():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    assert re.search(r"^#define VDB_KERNEL_GEMM_F32_GATHERED \(1u << 26\)$", HEADER, re.M)
    sys_rs = open(os.path.join(ROOT, "velesdb-hip", "src", "sys.rs")).read()
    assert re.search(r"^pub const VDB_KERNEL_GEMM_F32_GATHERED: i32 = 1 << 26;$", sys_rs, re.M)
    assert va.KERNEL_GEMM_F32_GATHERED == _ffi.VDB_KERNEL_GEMM_F32_GATHERED == 2 * _ffi.VDB_KERNEL_BITS_GATHERED
    assert _ffi.VDB_OPT_COUNT_ == 9 and re.search(r"VDB_OPT_COUNT_ = 9\b", HEADER)   # the tier is a value of an existing option


def test_the_header_names_the_kernel_at_the_filtered_call():
    comment = HEADER[:HEADER.index("int32_t vdb_hip_index_search_batch_filtered(")].rsplit("/*", 1)[1]
    assert "sweep_topk_f32_gathered" in comment and "VDB_KERNEL_GEMM_F32_GATHERED" in comment
    assert "for the three float metrics 3 is auto" not in HEADER


def test_four_instances_two_blocks_per_cu_no_scratch():
    pytest.importorskip("msgpack")
    import kernel_resources as kr
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    ks = [k for k in kr.kernels() if kr.family(k["name"]) == "sweep_topk_f32_gathered"]
    assert sorted(k["name"] for k in ks) == ["vdb::sweep_topk_f32_gathered<%d, %d>" % (m, tn) for m in (0, 2) for tn in (128, 16)], ks
    for k in ks:   # __launch_bounds__(256, 2): two four-wave blocks per CU, nothing in scratch
        assert k["block"] == 256 and k["waves_per_simd"] >= 2 and not (k["scratch"] or k["vgpr_spill"] or k["dynamic_stack"]), k
