"""What the compiler made of the half-precision graph walk (hnsw_half.hip), read from the built library like
tests/test_kernel_resources_cpu.py: every instance the dispatch can reach exists, none of them uses scratch memory, and the instances
of the headline shape (Cosine, 768 dimensions) sit at the occupancy of their f32 twins or above — they hold half the row registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytest.importorskip("msgpack")

COSINE, EUCLIDEAN, DOT = 0, 1, 2


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


def half(metric, cpl, ns, f16):
    return f"vdb::hnsw_search_half_kernel<{metric}, {cpl}, {ns}, {'true' if f16 else 'false'}>"


def test_every_instance_of_the_half_walk_exists(kernels):
    fam = [n for n in kernels if kr.family(n) == "hnsw_search_half_kernel"]
    want = {half(m, cpl, ns, f16) for m in (COSINE, EUCLIDEAN, DOT) for cpl in (0, 1, 2, 3, 4) for ns in (0, 4) for f16 in (True, False)}
    assert set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256 and k["waves_per_simd"] >= 4, k            # the throughput form: four 256-thread walks per CU
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("ns", [4, 0])
def test_headline_instances_are_no_worse_than_their_f32_twins(kernels, ns, f16):
    h = kernels[half(COSINE, 3, ns, f16)]
    t = kernels[f"vdb::hnsw_search_kernel<0, 3, {ns}, false, false, false>"]
    assert h["scratch"] <= t["scratch"] and h["waves_per_simd"] >= t["waves_per_simd"], (h, t)
    assert h["vgpr"] <= t["vgpr"], (h["vgpr"], t["vgpr"])                   # half the row registers: never more than the twin
