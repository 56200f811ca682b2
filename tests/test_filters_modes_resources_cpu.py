"""The grouped listed kernels of vdb_hip_index_search_batch_filters_mode in the built library, read through
tools/kernel_resources.py: sweep_topk_sq8_listed_groups<METRIC, B> and sweep_topk_half_l2_listed_groups<F16, B> exist instance for
instance next to their one-filter twins, hold no scratch, spill no vector register, use no dynamic stack and no FLAT or scratch
instruction (the work-item table and the list are read with global loads), and run at no fewer waves per SIMD than the twin — the
plan (mode_groups_plan) sizes its launches by the twin's occupancy.  The four existing families keep their instance counts."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("sweep_topk_sq8_listed_groups", "sweep_topk_sq8_listed", 9), ("sweep_topk_half_l2_listed_groups", "sweep_topk_half_l2_listed", 6)]


@pytest.fixture(scope="module")
def kernels():
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    return kr, kr.kernels()


def by_instance(kr, allk, fam):
    return {k["name"].split("<", 1)[1]: k for k in allk if kr.family(k["name"]) == fam}


def test_existing_families_keep_their_counts(kernels):
    kr, allk = kernels
    for fam, n in (("sweep_topk_sq8", 9), ("sweep_topk_sq8_listed", 9), ("sweep_topk_half_l2", 6), ("sweep_topk_half_l2_listed", 6)):
        assert sum(kr.family(k["name"]) == fam for k in allk) == n, fam


@pytest.mark.parametrize("grouped,twin,n", PAIRS)
def test_grouped_families_match_their_twins_instance_for_instance(kernels, grouped, twin, n):
    kr, allk = kernels
    grp, one = by_instance(kr, allk, grouped), by_instance(kr, allk, twin)
    assert len(grp) == n and sorted(grp) == sorted(one), (sorted(grp), sorted(one))
    for inst, k in sorted(grp.items()):
        assert k["block"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
        assert k["vgpr"] <= kr.REGS_PER_LANE, k
        assert k["waves_per_simd"] >= one[inst]["waves_per_simd"], (k, one[inst])
        assert k["lds"] == one[inst]["lds"], (k, one[inst])  # (the footprint is the launch's dynamic allocation: fm_*_lds_bytes)


@pytest.mark.parametrize("grouped,twin,n", PAIRS)
def test_grouped_kernels_use_global_loads_only(kernels, grouped, twin, n):
    kr, allk = kernels
    if not os.path.exists(kr.OBJDUMP):
        pytest.skip("no llvm-objdump")
    ks = [k for k in allk if kr.family(k["name"]) == grouped]
    assert len(ks) == n
    objs = kr.code_objects()
    for oi in {k["obj"] for k in ks}:
        funcs = kr.disassemble(objs[oi])
        for k in ks:
            if k["obj"] == oi:
                ins = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                assert kr.count(ins, "global_load") > 0 and kr.count(ins, "global_store") > 0, k["name"]
