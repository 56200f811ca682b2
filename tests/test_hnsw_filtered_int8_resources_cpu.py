"""What the compiler made of the filtered graph walk over the u8 codes (hnsw_search_filters_int8_kernel, hnsw_filtered.hip; DESIGN
4.1l), read from the built library's metadata like tests/test_hnsw_filtered_half_resources_cpu.py: every instance the dispatch can
reach exists — three metrics x CPL 0-4 — at the 256-thread block and the four walks per CU the launch assumes, without a dynamic
stack; and none of them keeps more in scratch memory, or spills more vector registers, than its sibling of the plain int8 walk — the
hnsw_search_int8_kernel instance of the same <METRIC, CPL> in the same form (LDS list, four waves, HBM visited bitmap) in the same
library.  The cap is the sibling's own figure, whatever the compiler of the day makes of it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytest.importorskip("msgpack")

COSINE, EUCLIDEAN, DOT = 0, 1, 2
FAMILY = "hnsw_search_filters_int8_kernel"
INSTANCES = [(m, cpl) for m in (COSINE, EUCLIDEAN, DOT) for cpl in (0, 1, 2, 3, 4)]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


def test_every_instance_exists_at_four_waves(kernels):
    fam = [n for n in kernels if kr.family(n) == FAMILY]
    want = {f"vdb::{FAMILY}<{m}, {cpl}>" for m, cpl in INSTANCES}
    assert len(want) == 15 and set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256 and k["waves_per_simd"] >= 4 and not k["dynamic_stack"], k


@pytest.mark.parametrize("metric,cpl", INSTANCES)
def test_no_more_scratch_or_spilled_vector_registers_than_the_plain_int8_walk(kernels, metric, cpl):
    k = kernels[f"vdb::{FAMILY}<{metric}, {cpl}>"]
    sib = kernels[f"vdb::hnsw_search_int8_kernel<{metric}, {cpl}, 0, 4, false>"]  # <METRIC, CPL, NS = 0, WAVES = 4, VIS = false>
    assert sib["block"] == 256 and sib["waves_per_simd"] >= 4, sib
    assert k["scratch"] <= sib["scratch"] and k["vgpr_spill"] <= sib["vgpr_spill"], (k, sib)
