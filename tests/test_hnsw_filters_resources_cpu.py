"""What the compiler made of the filtered graph walk and its exact pass (hnsw_search_filters_kernel / filters_rank_kernel,
hnsw_filtered.hip), read from the built library like tests/test_hnsw_half_resources_cpu.py: every instance the
dispatch can reach exists, at four walks per CU, without scratch memory, vector spills or a dynamic stack — and the descriptor
loads left the LDS state and the filter reads off the flat path.  These two families serve the one-filter call
(vdb_hip_index_search_graph_filtered) as well: the families it once had of its own are gone from the library."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytest.importorskip("msgpack")

COSINE, EUCLIDEAN, DOT, HAMMING, JACCARD = 0, 1, 2, 3, 4
INSTANCES = [(m, cpl) for m in (COSINE, EUCLIDEAN, DOT) for cpl in (0, 1, 2, 3, 4)] + [(HAMMING, 0), (JACCARD, 0)]
NEW = ["hnsw_search_filters_kernel", "filters_rank_kernel"]
RETIRED = ["hnsw_search_filtered_kernel", "filter_rank_kernel"]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


@pytest.mark.parametrize("family", NEW)
def test_every_instance_exists_at_four_waves_without_scratch(kernels, family):
    fam = [n for n in kernels if kr.family(n) == family]
    want = {f"vdb::{family}<{m}, {cpl}>" for m, cpl in INSTANCES}
    assert len(want) == 17 and set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256 and k["waves_per_simd"] >= 4, k
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k


def test_the_one_filter_families_are_gone(kernels):
    assert [n for n in kernels if kr.family(n) in RETIRED] == []


@pytest.mark.skipif(not os.path.exists(kr.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_lds_state_and_descriptors_stay_off_the_flat_path(kernels):
    ks = [k for n, k in kernels.items() if kr.family(n) in NEW]
    assert len(ks) == 34
    objs = kr.code_objects()
    for oi in {k["obj"] for k in ks}:
        funcs = kr.disassemble(objs[oi])
        for k in ks:
            if k["obj"] == oi:
                ins = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                assert kr.count(ins, "ds_") > 0 and kr.count(ins, "global_load") > 0, k["name"]
