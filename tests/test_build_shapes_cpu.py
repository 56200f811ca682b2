"""The conditions of tests/build_shapes.py on the oracle alone: every case of tests/test_gpu_build_shapes.py still reaches
the edge of hnsw_build.hip it was chosen for.  A case that stops reaching it fails here, where no GPU is needed to see it.
The floors are caps, not measurements: if one does not hold any more, change the data of the case, not the floor."""
import numpy as np
import pytest

import build_shapes as bs
from oracle import pyoracle as po


def test_schedule_is_the_oracles():
    # schedule() restates vo_hnsw_build_batched's loop: same sizes as stepping the oracle's own build_batch_size
    for n, mb in ((1, 0), (17, 64), (3000, 256), (70_000, 0), (70_000, 4096), (72_000, 4096)):
        linked, want = 0, []
        while linked < n:
            b = 1 if linked == 0 else min(po.lib().vo_build_batch_size(linked, mb or 2048), n - linked)
            want.append(b)
            linked += b
        assert bs.schedule(n, mb) == want
    assert bs.schedule(400, 64, linked=1500) == [64] * 6 + [16]


@pytest.mark.parametrize("name", bs.SCHEDULE_CASES + ("layer_cap",))
def test_big_cases_reach_the_cap(name):
    sizes, before_last, cap = bs.schedule_facts(name)
    assert po.lib().vo_build_batch_size(before_last, cap) == cap, "the last batch is not sized by the cap"
    if name in bs.FULL_BATCH_CASES:
        assert max(sizes) == cap
    if cap == 4096:
        assert before_last + sizes[-1] > 65536 and before_last >= 65536      # a 17-bit node field: three 8-bit digits
        assert max(sizes) > 2048                                             # a batch field wider than the default cap's
    if name == "schedule_4096_full":
        assert sizes.count(4096) >= 1 and (4096).bit_length() == 13


def test_layer_cap_is_reached():
    g = bs.oracle_build("layer_cap")
    assert g.num_layers == 16 and g.max_layer == 15


def test_graph_file_reader_matches_neighbors(tmp_path):
    name = "layer_cap"
    g, n = bs.oracle_build(name), bs.BIG_CASES[name][1]
    g.file_dump(str(tmp_path), "ora")
    nl, ml, ep, count, lists = bs.read_graph_file(str(tmp_path / "ora.graph"))
    assert (nl, ml, ep, count) == (g.num_layers, g.max_layer, g.entry_point, n)
    for layer in range(nl):
        assert len(lists[layer]) == n
        for node in list(range(0, n, 101)) + [g.entry_point, n - 1]:
            assert list(lists[layer][node]) == g.neighbors(layer, node)


@pytest.mark.parametrize("name", sorted(bs.HUB_CASES))
def test_hub_cases_make_hubs(name):
    g, largest = bs.hub_case_oracle(name)
    assert len(g) == bs.HUB_N
    if name.startswith("star"):
        assert largest >= bs.HUB_GROUP_MIN, f"largest (layer 0, target) group of a batch: {largest}"
    else:
        pairs = bs.zero_distance_pairs(g, bs.hub_case_data(name)[2])
        assert pairs >= bs.DUP_PAIRS_MIN, f"{pairs} links between copies of one row"


def test_gaussian_rows_make_no_hubs():
    # what the star sets are compared with: the same build over plain Gaussian rows stays far below the floor
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((bs.HUB_N, bs.HUB_DIM)).astype(np.float32)
    g = bs.new_oracle(bs.HUB_DIM, "euclidean", bs.HUB_M, bs.HUB_EFC)
    pos, largest = 0, 0
    for b in bs.schedule(bs.HUB_N, bs.HUB_MB):
        g.insert_batch_sync(rows[pos:pos + b])
        t = [x for node in range(pos, pos + b) for x in g.neighbors(0, node)]
        largest = max(largest, int(np.bincount(np.asarray(t, dtype=np.int64)).max()) if t else 0)
        pos += b
    assert 0 < largest < bs.HUB_GROUP_MIN


@pytest.mark.parametrize("name", list(bs.WIDTH_CASES))
def test_width_cases_fill_their_lists(name):
    _, n, _, M, efc = bs.WIDTH_CASES[name]
    g = bs.oracle_build(name)
    assert len(g) == n
    share = bs.full_share(g, n, M)
    if bs.width_case_must_fill(name):
        assert share > 0.5, f"{share:.3f} of the layer-0 lists are full: the prune at stride {2 * M} is hardly exercised"
    else:
        assert efc < 2 * M     # the point of these: nbmax comes from the stride, not from ef_construction


def test_vlog_case_overflows_the_visited_log():
    g = bs.oracle_build("vlog")
    visited = bs.vlog_visited(g, bs.vlog_case_data()[1])
    assert len(visited) == bs.VLOG_PROBES and min(visited) > bs.VLOG_CAP, (min(visited), max(visited))


@pytest.mark.parametrize("metric,dim", bs.LOAD_CASES)
def test_inserts_after_a_load_prune_loaded_lists(tmp_path, metric, dim):
    _, pruned = bs.load_case_oracle(metric, dim, tmp_path)
    assert pruned >= bs.LOAD_PRUNED_MIN, pruned


@pytest.mark.parametrize("metric,dim", bs.LOAD_ONE_BY_ONE)
def test_single_inserts_after_a_load_prune_loaded_lists(tmp_path, metric, dim):
    assert (metric, dim) in bs.LOAD_CASES
    _, pruned = bs.load_case_oracle(metric, dim, tmp_path, one_by_one=True)
    assert pruned >= bs.LOAD_PRUNED_MIN, pruned


def test_tables_hold_what_the_kernels_dispatch_on():
    # CPL 1 / 2 / 4 and the generic layout below, between and above them; dims that are no multiple of 4; one bit word, a
    # ragged one, many
    assert {256, 512, 1024} <= set(bs.DIMS_FLOAT) and any(d % 4 for d in bs.DIMS_FLOAT) and max(bs.DIMS_FLOAT) > 4096
    assert {31, 32, 33} <= set(bs.DIMS_BITS)
    assert len(bs.DIM_CASES) == 3 * len(bs.DIMS_FLOAT) + 2 * len(bs.DIMS_BITS)
    assert {m for m, _ in bs.LOAD_CASES} == set(bs.METRIC) == {m for m, _ in bs.LOAD_ONE_BY_ONE}
    strides = sorted({2 * c[3] for c in bs.WIDTH_CASES.values()})
    assert {(s + 1 + 63) // 64 for s in strides} == {1, 2, 3, 4, 5}      # rounds of the prune's lane ownership over stride + 1 entries
