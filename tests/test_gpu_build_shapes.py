"""Graph construction on the GPU == the oracle's batch-synchronous restatement (NativeHnsw::insert, select_neighbors,
add_bidirectional_connection: native/graph.rs:158-237,526-639), link for link, at the shapes where hnsw_build.hip and the
link-request sort of radix_sort.hip take another path than on a few thousand Gaussian rows at dim 96:

  1. every dim class of hnsw_insert_kernel (CPL 1 / 2 / 4 and the generic LDS-query layout below, between and above them,
     dims that are no multiple of 4) x every metric, built in batches and continued with insert_batch_parallel;
  2. the batch schedule at its real size: 70 000 nodes, batches of 2 048 and 4 096 — radix digit plans with a 12- and a
     13-bit batch field and a 17-bit node field (three 8-bit digits);
  3. the layer cap: 16 layers, requests on layer 15 (whose key field equals the unused slots');
  4. hubs: (layer, target) groups several times the list's stride in one wave of hnsw_link_kernel; duplicate rows: lists
     full of zero and exactly tied distances;
  5. list strides of 4 .. 256 (1 .. 5 rounds of the prune's lane ownership, strides that are no multiple of 64), the
     reference's presets, ef_construction below the stride, 1, and around multiples of 64;
  6. an insert that visits more nodes than the visited log holds (CMD_CLEAN clears the whole bitmap);
  7. inserts into a loaded graph: graph_fill_ndist's distance cache, every metric and dim class, feeds the next prunes.

The shapes, and the oracle-side conditions that say a shape reaches its edge, live in tests/build_shapes.py; the
conditions alone run without a GPU in tests/test_build_shapes_cpu.py.  Every test also runs 16 queries at ef 64 over the
finished graph and compares ids with the oracle's search of its own graph."""
import numpy as np
import pytest

import build_shapes as bs
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
GPU_METRIC = {"cosine": DM.Cosine, "euclidean": DM.Euclidean, "dot": DM.DotProduct, "hamming": DM.Hamming, "jaccard": DM.Jaccard}


def gpu_build(rows, metric, M, efc, max_batch):
    n, dim = rows.shape
    ix = va.HnswIndex(dim, GPU_METRIC[metric], va.HnswParams(M, efc, n))
    assert ix.upload(np.arange(n, dtype=np.uint64), rows) == n
    ix.build_graph(max_batch)
    assert ix.node_count() == n
    return ix


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dim", bs.DIM_CASES)
def test_dim_classes_batched_build_and_insert(gpu_required, metric, dim):
    rows, more, qs = bs.dim_case_data(metric, dim)
    n = rows.shape[0]
    g = bs.new_oracle(dim, metric, bs.DIM_M, bs.DIM_EFC)
    g.build_batched(rows, bs.DIM_MB)
    ix = gpu_build(rows, metric, bs.DIM_M, bs.DIM_EFC, bs.DIM_MB)
    try:
        bs.assert_same_graph(g, ix, n)
        g.build_batched(more, bs.DIM_MB)
        assert ix.insert_batch_parallel([(n + i, v) for i, v in enumerate(more)], bs.DIM_MB) == len(more)
        bs.assert_same_graph(g, ix, n + len(more))
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


# ---- 2, 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bs.BIG_CASES))
def test_full_schedule_and_layer_cap(gpu_required, tmp_path, name):
    metric, n, _dim, M, efc, mb, _omb, _seed = bs.BIG_CASES[name]
    sizes, before_last, cap = bs.schedule_facts(name)
    assert po.lib().vo_build_batch_size(before_last, cap) == cap, "the last batch is not sized by the cap"
    if name in bs.FULL_BATCH_CASES:
        assert max(sizes) == cap
    rows, qs = bs.big_case_data(name)
    g = bs.oracle_build(name)
    if name == "layer_cap":
        assert g.num_layers == 16 and g.max_layer == 15
    ix = gpu_build(rows, metric, M, efc, mb)
    try:
        bs.assert_same_graph(g, ix, n, via_files=tmp_path)
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bs.HUB_CASES))
def test_hubs_and_duplicates(gpu_required, name):
    metric = bs.HUB_CASES[name]
    rows, qs, src = bs.hub_case_data(name)
    g, largest = bs.hub_case_oracle(name)
    if name.startswith("star"):
        assert largest >= bs.HUB_GROUP_MIN, f"largest (layer 0, target) group of a batch: {largest}"
    else:
        assert bs.zero_distance_pairs(g, src) >= bs.DUP_PAIRS_MIN
    ix = gpu_build(rows, metric, bs.HUB_M, bs.HUB_EFC, bs.HUB_MB)
    try:
        bs.assert_same_graph(g, ix, bs.HUB_N)
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bs.WIDTH_CASES))
def test_list_widths_and_small_ef(gpu_required, name):
    metric, n, _dim, M, efc = bs.WIDTH_CASES[name]
    rows, qs = bs.width_case_data(name)
    g = bs.oracle_build(name)
    if bs.width_case_must_fill(name):
        share = bs.full_share(g, n, M)
        assert share > 0.5, f"{share:.3f} of the layer-0 lists are full: the prune at stride {2 * M} is hardly exercised"
    ix = gpu_build(rows, metric, M, efc, 0)
    try:
        bs.assert_same_graph(g, ix, n)
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------
def test_visited_log_overflow(gpu_required, tmp_path):
    metric, n, _dim, M, efc = bs.VLOG_CASE
    rows, probes, qs = bs.vlog_case_data()
    g = bs.oracle_build("vlog")
    visited = bs.vlog_visited(g, probes)
    assert min(visited) > bs.VLOG_CAP, (min(visited), max(visited))
    ix = gpu_build(rows, metric, M, efc, 0)
    try:
        bs.assert_same_graph(g, ix, n, via_files=tmp_path)
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------
def insert_after_load(tmp_path, metric, dim, one_by_one):
    _rows, more, qs = bs.load_case_data(metric, dim)
    g, pruned = bs.load_case_oracle(metric, dim, tmp_path, one_by_one)
    assert pruned >= bs.LOAD_PRUNED_MIN, f"{pruned} loaded full lists changed: the cached distances hardly ranked anything"
    ix = va.HnswIndex(dim, GPU_METRIC[metric], va.HnswParams(bs.LOAD_M, bs.LOAD_EFC, bs.LOAD_N + bs.LOAD_MORE))
    try:
        ix.load_reference_files(str(tmp_path), "native_hnsw")
        assert ix.node_count() == bs.LOAD_N
        if one_by_one:
            for i, v in enumerate(more):
                ix.insert(bs.LOAD_N + i, v)
        else:
            assert ix.insert_batch_parallel([(bs.LOAD_N + i, v) for i, v in enumerate(more)], bs.LOAD_MB) == len(more)
        bs.assert_same_graph(g, ix, bs.LOAD_N + bs.LOAD_MORE)
        bs.assert_same_search(g, ix, qs, va)
    finally:
        ix.close()


@pytest.mark.parametrize("metric,dim", bs.LOAD_CASES)
def test_batched_inserts_after_load(gpu_required, tmp_path, metric, dim):
    insert_after_load(tmp_path, metric, dim, one_by_one=False)


@pytest.mark.parametrize("metric,dim", bs.LOAD_ONE_BY_ONE)
def test_single_inserts_after_load(gpu_required, tmp_path, metric, dim):
    insert_after_load(tmp_path, metric, dim, one_by_one=True)
