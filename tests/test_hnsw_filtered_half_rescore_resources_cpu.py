"""What the compiler made of the half-precision filtered walk with the f32 re-score (hnsw_search_filters_half_rescore_kernel,
hnsw_filtered.hip), read from the built library's metadata like tests/test_hnsw_filtered_int8_resources_cpu.py: every
instance the dispatch can reach exists — three metrics x CPL 0-4 x two precisions — at the 256-thread block and the four walks per CU
the launch assumes, without a dynamic stack; and none of them keeps more in scratch memory, or spills more vector registers, than the
larger of its two siblings' own figures in the same library: hnsw_search_filters_half_kernel<M, CPL, F16> (the walk it runs) and
hnsw_search_filters_kernel<M, CPL> (the f32 phase it re-scores with).  The cap is the siblings' own figure, whatever the compiler of
the day makes of them; an instance above it is a finding to fix (the rows-per-group constants of FiltDistHalfRescore), not a cap to
raise."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytest.importorskip("msgpack")

COSINE, EUCLIDEAN, DOT = 0, 1, 2
FAMILY = "hnsw_search_filters_half_rescore_kernel"
INSTANCES = [(m, cpl, f16) for m in (COSINE, EUCLIDEAN, DOT) for cpl in (0, 1, 2, 3, 4) for f16 in ("false", "true")]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


def test_every_instance_exists_at_four_waves(kernels):
    fam = [n for n in kernels if kr.family(n) == FAMILY]
    want = {f"vdb::{FAMILY}<{m}, {cpl}, {f16}>" for m, cpl, f16 in INSTANCES}
    assert len(want) == 30 and set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256 and k["waves_per_simd"] >= 4 and not k["dynamic_stack"], k


@pytest.mark.parametrize("metric,cpl,f16", INSTANCES)
def test_no_more_scratch_or_spilled_vector_registers_than_its_siblings(kernels, metric, cpl, f16):
    k = kernels[f"vdb::{FAMILY}<{metric}, {cpl}, {f16}>"]
    half = kernels[f"vdb::hnsw_search_filters_half_kernel<{metric}, {cpl}, {f16}>"]
    f32 = kernels[f"vdb::hnsw_search_filters_kernel<{metric}, {cpl}>"]
    for sib in (half, f32):
        assert sib["block"] == 256 and sib["waves_per_simd"] >= 4, sib
    print(f"scratch {k['scratch']} (siblings {half['scratch']}, {f32['scratch']}), spilled vector registers {k['vgpr_spill']} "
          f"(siblings {half['vgpr_spill']}, {f32['vgpr_spill']})")
    assert k["scratch"] <= max(half["scratch"], f32["scratch"]), (k, half, f32)
    assert k["vgpr_spill"] <= max(half["vgpr_spill"], f32["vgpr_spill"]), (k, half, f32)
