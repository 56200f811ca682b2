"""The per-query form of the hybrid fusion kernel (hybrid_fuse_filters_kernel) in the built library, read through
tools/kernel_resources.py: it exists once, holds no scratch, spills no register, uses no dynamic stack and no FLAT or scratch
instruction — the filter descriptor's bitmap pointer comes out of memory and is typed as a global address by hand, so the per-hit
bitmap read must be a global load — and sits at the occupancy of hybrid_fuse_kernel, whose body it shares.  hybrid_fuse_kernel itself
keeps the metadata record it had before the body moved into a shared function (the figures below were read from a library built
from the parent commit with tools/kernel_resources.py --diff: no kernel changed its record, one kernel was added), and
fuse_lists_kernel, which the multi-query form launches unchanged, keeps its own."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytest.importorskip("msgpack")
import kernel_resources as kr  # noqa: E402

RECORD = ("vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds", "block", "kernarg", "dynamic_stack", "waves_per_simd")
# the parent commit's records
PARENT = {
    "vdb::hybrid_fuse_kernel": (128, 0, 56, 0, 0, 0, 0, 1024, 368, False, 4),
    "vdb::fuse_lists_kernel": (126, 0, 52, 0, 0, 0, 0, 1024, 352, False, 4),
}
NEW = "vdb::hybrid_fuse_filters_kernel"


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kr.LIB):
        pytest.skip("library not built")
    return kr.kernels()


def named(kernels, name):
    ks = [k for k in kernels if k["name"] == name]
    assert len(ks) == 1, (name, len(ks))
    return ks[0]


def test_existing_fusion_kernels_keep_the_parents_metadata(kernels):
    for name, want in PARENT.items():
        k = named(kernels, name)
        assert tuple(k[c] for c in RECORD) == want, (name, {c: k[c] for c in RECORD})


def test_per_query_kernel_holds_no_scratch_and_spills_nothing(kernels):
    k = named(kernels, NEW)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and not k["dynamic_stack"], k
    assert k["block"] == 1024 and k["lds"] == 0, k                   # (the LDS array is the launch's dynamic allocation)
    one = named(kernels, "vdb::hybrid_fuse_kernel")
    assert k["waves_per_simd"] >= one["waves_per_simd"] and k["vgpr"] <= one["vgpr"], (k, one)
    # HybridArgs by value, the descriptor table, the slot table and the table's length behind it
    assert one["kernarg"] < k["kernarg"] <= one["kernarg"] + 24, (k["kernarg"], one["kernarg"])


def test_per_query_kernel_reads_the_bitmap_with_global_loads(kernels):
    if not os.path.exists(kr.OBJDUMP):
        pytest.skip("no llvm-objdump")
    k, one = named(kernels, NEW), named(kernels, "vdb::hybrid_fuse_kernel")
    objs = kr.code_objects()
    assert k["obj"] == one["obj"]
    funcs = kr.disassemble(objs[k["obj"]])
    ins = [x for _, b in funcs[k["symbol"]] for x in b]
    ref = [x for _, b in funcs[one["symbol"]] for x in b]
    assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0
    # the same vector memory traffic as the one-filter kernel: the shared body, no extra per-thread load for the slot or the descriptor
    for op in ("global_load", "global_store", "ds_read", "ds_write"):
        assert kr.count(ins, op) == kr.count(ref, op) > 0, (op, kr.count(ins, op), kr.count(ref, op))
