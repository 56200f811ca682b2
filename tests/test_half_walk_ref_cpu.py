"""CPU tier: the reference the GPU tests of the half-precision graph walk stand on (tests/half_walk_ref.py), and the new surface.

  * the file-patch helper: `file_load` of a patched dump returns the ROUNDED vectors and the neighbour lists of the original graph;
  * on the exact grid data the oracle's mode-C scores equal half_ref.scores (the reference's sequential chains) bit for bit — the
    claim that lets the mode-C oracle stand in as a half-precision reference there;
  * header, Python mirror and Rust constants name the two modes and the kernel bit (fails without the feature).
"""
import os
import re

import numpy as np
import pytest

import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("precision", [hr.F16, hr.BF16])
def test_patched_dump_loads_rounded_vectors_and_the_same_links(tmp_path, precision):
    rng = np.random.default_rng(3)
    n, dim, M, efc = 300, 37, 6, 40
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    g = hw.build_graph(rows, hr.DOT, M, efc)
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    os.makedirs(src)
    g.file_dump(src, "native_hnsw")
    rounded = hw.patch_vectors(src, dst, "native_hnsw", precision)
    assert np.array_equal(hw.bits(rounded), hw.bits(hr.round_half(rows, precision)))
    assert not np.array_equal(hw.bits(rounded), hw.bits(rows))            # N(0,1) is not half-representable
    gh = hw.load_graph(dst, "native_hnsw", hr.DOT, dim)
    assert len(gh) == n and gh.num_layers == g.num_layers and gh.entry_point == g.entry_point and gh.max_layer == g.max_layer
    for node in range(n):
        assert np.array_equal(hw.bits(gh.vector(node)), hw.bits(rounded[node]))
        for layer in range(g.num_layers):
            assert gh.neighbors(layer, node) == g.neighbors(layer, node)
    # and the source directory is untouched
    g2 = hw.load_graph(src, "native_hnsw", hr.DOT, dim)
    assert np.array_equal(hw.bits(g2.vector(5)), hw.bits(rows[5]))


@pytest.mark.parametrize("precision", [hr.F16, hr.BF16])
@pytest.mark.parametrize("dim", [96, 768, 37])
def test_oracle_mode_c_equals_the_half_reference_on_the_grid(precision, dim):
    rng = np.random.default_rng(dim + precision)
    rows, qs = hw.grid(rng, (200, dim), precision), hw.grid(rng, (6, dim), precision)
    assert np.array_equal(hw.bits(hr.round_half(rows, precision)), hw.bits(rows))      # the grid is representable
    if precision == hr.F16:
        assert not np.array_equal(hw.bits(hr.round_half(rows, hr.BF16)), hw.bits(rows))  # ... and holds values bf16 does not
    assert np.abs(rows).sum(1).min() > 0
    for metric in (hr.COSINE, hr.EUCLIDEAN, hr.DOT):
        want = hr.scores(metric, precision, rows, qs)
        for qi in range(qs.shape[0]):
            got = po.batch_compute_distance(hw.PO_METRIC[metric], qs[qi], rows, po.MODE_C)
            assert np.array_equal(hw.bits(got), hw.bits(want[qi])), (metric, qi)


def test_surface_header_python_rust():
    import velesdb_amd as va
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "velesdb_hip.h")).read(), flags=re.S)
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", src))
    assert (enums["VDB_SEARCH_HNSW_F16"], enums["VDB_SEARCH_HNSW_BF16"], enums["VDB_KERNEL_HNSW_HALF"]) == (8, 9, 32768)
    assert (va.MODE_HNSW_F16, va.MODE_HNSW_BF16, va.KERNEL_HNSW_HALF) == (8, 9, 32768)
    assert sorted(v for k, v in enums.items() if k.startswith("VDB_SEARCH_")) == list(range(10))
    bits = [v for k, v in enums.items() if k.startswith("VDB_KERNEL_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    assert callable(va.HnswIndex.search_batch_half_graph)
    rs = open(os.path.join(ROOT, "velesdb-hip", "src", "lib.rs")).read()
    assert "pub fn search_batch_half_graph" in rs and "sys::VDB_SEARCH_HNSW_F16" in rs and "sys::VDB_SEARCH_HNSW_BF16" in rs
