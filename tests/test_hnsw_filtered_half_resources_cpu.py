"""What the compiler made of the filtered graph walk and its exact pass over the half-precision images (hnsw_filtered.hip, DESIGN
4.1k), read from the built library like tests/test_hnsw_filters_resources_cpu.py: every instance the dispatch can reach exists —
three metrics x CPL 0-4 x f16 / bf16 in the per-query form — and none of them uses scratch memory, spills a vector register or
needs a dynamic stack; all of them keep the four 256-thread walks per CU the launch assumes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytest.importorskip("msgpack")

COSINE, EUCLIDEAN, DOT = 0, 1, 2
FAMILIES = ["hnsw_search_filters_half_kernel", "filters_rank_half_kernel"]
INSTANCES = [(m, cpl, f16) for m in (COSINE, EUCLIDEAN, DOT) for cpl in (0, 1, 2, 3, 4) for f16 in ("true", "false")]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


@pytest.mark.parametrize("family", FAMILIES)
def test_every_instance_exists_at_four_waves_without_scratch(kernels, family):
    fam = [n for n in kernels if kr.family(n) == family]
    want = {f"vdb::{family}<{m}, {cpl}, {f16}>" for m, cpl, f16 in INSTANCES}
    assert len(want) == 30 and set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256 and k["waves_per_simd"] >= 4, k  # the throughput form: four 256-thread walks per CU
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k


@pytest.mark.skipif(not os.path.exists(kr.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_lds_state_stays_off_the_flat_path(kernels):
    ks = [k for n, k in kernels.items() if kr.family(n) in FAMILIES]
    assert len(ks) == 60
    objs = kr.code_objects()
    for oi in {k["obj"] for k in ks}:
        funcs = kr.disassemble(objs[oi])
        for k in ks:
            if k["obj"] == oi:
                ins = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                assert kr.count(ins, "ds_") > 0 and kr.count(ins, "global_load") > 0, k["name"]
