"""The listed forms of the two streaming kernels in the built library, read through tools/kernel_resources.py: the
families exist with every instance, hold no scratch, spill no vector register, use no dynamic stack and no FLAT instruction, sit
at no fewer waves per SIMD than their unlisted twins, and the unlisted families keep their instance counts."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytest.importorskip("msgpack")
import kernel_resources as kr  # noqa: E402

PAIRS = {"sweep_topk_sq8_listed": ("sweep_topk_sq8", 9), "sweep_topk_half_l2_listed": ("sweep_topk_half_l2", 6)}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kr.LIB):
        pytest.skip("library not built")
    return kr.kernels()


def fam(kernels, name):
    return [k for k in kernels if kr.family(k["name"]) == name]


def instance(k):
    return re.search(r"<(.*)>", k["name"]).group(1)


def test_listed_families_exist_next_to_unchanged_twins(kernels):
    for listed, (twin, n) in PAIRS.items():
        assert len(fam(kernels, listed)) == n, (listed, len(fam(kernels, listed)))
        assert len(fam(kernels, twin)) == n, (twin, len(fam(kernels, twin)))
        assert sorted(map(instance, fam(kernels, listed))) == sorted(map(instance, fam(kernels, twin)))


def test_listed_kernels_hold_no_scratch_and_spill_no_vector_register(kernels):
    for listed in PAIRS:
        for k in fam(kernels, listed):
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
            assert k["vgpr"] <= kr.REGS_PER_LANE, k


def test_listed_kernels_keep_their_twins_occupancy(kernels):
    for listed, (twin, _) in PAIRS.items():
        twins = {instance(k): k for k in fam(kernels, twin)}
        for k in fam(kernels, listed):
            assert k["waves_per_simd"] >= twins[instance(k)]["waves_per_simd"], (k["name"], k["vgpr"], twins[instance(k)]["vgpr"])
            assert k["lds"] == twins[instance(k)]["lds"], k["name"]  # (static LDS: none; the dynamic layout is the twin's)


def test_listed_kernels_read_the_list_with_global_loads(kernels):
    if not os.path.exists(kr.OBJDUMP):
        pytest.skip("no llvm-objdump")
    ks = [k for listed in PAIRS for k in fam(kernels, listed)]
    objs = kr.code_objects()
    for oi in {k["obj"] for k in ks}:
        funcs = kr.disassemble(objs[oi])
        for k in ks:
            if k["obj"] == oi:
                ins = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(ins, "flat_") == 0 and kr.count(ins, "scratch_") == 0, k["name"]
                assert kr.count(ins, "global_load") > 0, k["name"]
