"""The yardstick of the filtered walk over the u8 codes validates itself on the CPU (tests/filtered_int8_ref.py), before any GPU run:
with every row allowed it IS the oracle's DualPrecisionHnsw search (po.dual_search_int8) — ids, exact-distance bits and both
counters; its two forms agree under filters; the worlds of tests/test_gpu_filters_graph_int8.py overflow nowhere the GPU tests assume
they do not, and split where the overflow test needs a split; and the big-distance world really tells integer order from
value-converted order."""
import numpy as np
import pytest

import filtered_int8_ref as fi
import filtered_walk_ref as fw
from oracle import pyoracle as po

KEF = [(10, 64), (1, 16), (25, 50)]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module", params=[(m, s) for m in fi.METRICS for s in ((1500, 96, 8, 60), (1200, 300, 8, 60))],
                ids=lambda p: f"m{p[0]}-{p[1][0]}x{p[1][1]}")
def world(request):
    return fi.World(None, *request.param)


@pytest.mark.parametrize("ratio", [4, 1])
@pytest.mark.parametrize("k,ef", KEF)
def test_every_row_allowed_is_the_oracle_dual_precision_search(world, k, ef, ratio):
    w, allowed = world, np.ones(world.n, dtype=bool)
    for q in w.qs:
        oid, od, nd, ne = po.dual_search_int8(w.g, w.sq, w.codes, q, k, ef, ratio, po.TIE_CANONICAL)
        a = fi.walk_two_heap(w.G, q, k, ef, ratio, allowed)
        b = fi.walk(w.G, q, k, ef, ratio, allowed, w.n + 64)
        for r in (a, b):
            assert r[0] == oid.tolist() and bits(r[1]) == bits(od) and (r[2], r[3]) == (nd, ne), (k, ef, ratio)
        assert not b[4]


def test_the_two_forms_agree_under_filters(world):
    w, k, ef, ratio = world, 10, 64, 4
    _, ef_w = fi.widths(k, ef, ratio)
    peak = 0
    for name in ("half", "tenth", "clustered"):
        allowed = w.filters[name]
        sized = fw.sized_list(ef_w, int(allowed.sum()), w.n)
        for q in w.qs:
            a = fi.walk_two_heap(w.G, q, k, ef, ratio, allowed)
            b = fi.walk(w.G, q, k, ef, ratio, allowed, sized)
            assert not b[4], (name, "the sized list overflows")
            assert b[0] == a[0] and bits(b[1]) == bits(a[1]) and b[2:4] == a[2:4], name
            assert all(allowed[i] for i in b[0]) and len(b[0]) == k
            peak = max(peak, b[5]["peak"])
    print(f"peak list length {peak}")


def test_bit_cast_distances_order_as_the_integers():
    d = np.array([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 24) + 1, (1 << 24) + 2, 66_585_600], dtype=np.uint32)  # (the last: 1024 * 255^2)
    f = d.view(np.float32)
    assert all(f[i] < f[i + 1] for i in range(len(f) - 1)) and [fw.tkey(x) for x in f] == sorted(fw.tkey(x) for x in f)
    assert np.array_equal(fi.d8_of(f), d)
    assert np.float32(int(d[5])) == np.float32(int(d[5]) - 1), "by value, 2^24 + 1 is not representable: that is the trap"


# ---- the worlds of the GPU tests --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_worlds():
    cache = {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = fi.World(None, metric, shape, const_dim=shape == fi.CONST_DIM_SHAPE)
        return cache[(metric, shape)]
    return get


@pytest.mark.parametrize("shape", fi.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("metric", fi.METRICS)
def test_no_query_of_the_gpu_worlds_overflows_its_sized_list(gpu_worlds, metric, shape):
    """what tests/test_gpu_filters_graph_int8.py assumes of the walk route: the first list holds every query (the GPU's own largest
    list is checked there, against the plan's)"""
    w, k = gpu_worlds(metric, shape), 10
    for name in ("half", "tenth", "clustered"):
        want = fi.expect_call(w.G, w.qs, w.filters[name], k, 64, 4, fi.ROUTE_WALK)
        assert want[2] == [1] * fi.NQ, name
    few = w.filters["few"]
    assert int(few.sum()) == 40 and fi.expect_call(w.G, w.qs[:1], few, k, 64, 4, fi.ROUTE_AUTO)[2] == [2]
    if shape == fi.CONST_DIM_SHAPE:  # the ratio cases (k 25, Balanced ef) and k beyond the allowed rows (the list takes the graph)
        for name in ("half", "tenth"):
            for ratio in (1, 4, 7):
                assert fi.expect_call(w.G, w.qs, w.filters[name], 25, 0, ratio, fi.ROUTE_WALK)[2] == [1] * fi.NQ, (name, ratio)
        want = fi.expect_call(w.G, w.qs, few, 50, 0, 1, fi.ROUTE_WALK)
        assert want[2] == [1] * fi.NQ and all(30 <= len(i) <= 40 for i in want[0])  # (what the directed links reach of the 40)


@pytest.mark.parametrize("metric", fi.METRICS)
def test_the_overflow_case_splits_the_queries(gpu_worlds, metric):
    w = gpu_worlds(metric, fi.SHAPES[0])
    allowed, qs, max_list, over = fi.overflow_case(w, 10, 16, 1)
    assert max_list is not None and 0 < sum(over) < fi.NQ, "no list size splits the queries: the GPU case would be meaningless"
    want = fi.expect_call(w.G, qs, allowed, 10, 16, 1, fi.ROUTE_AUTO, max_list=max_list)
    assert want[2] == [2 if o else 1 for o in over]


# ---- integers beyond 2^24, and ties ----------------------------------------------------------------------------------------------------
def test_the_big_distance_world_separates_integer_order_from_value_converted_order():
    w = fi.BigWorld(None)
    k, ef, ratio = fi.BIG_K, fi.BIG_EF, fi.BIG_RATIO
    cand_k, ef_w = fi.widths(k, ef, ratio)
    sized = fw.sized_list(ef_w, int(w.allowed.sum()), w.n)
    big = tied = changed = 0
    for q in w.qs:
        qc = w.sq.quantize(q)[0]
        coarse = fw.walk_single_list(w.G, qc, cand_k, ef_w, w.allowed, sized)
        assert not coarse[4]
        d8 = fi.d8_of(coarse[1])
        big += int((d8 >= 1 << 24).sum())
        tied += int(len(d8) - len(set(d8.tolist())))
        exact = fi.walk(w.G, q, k, ef, ratio, w.allowed, sized)
        wrong = fi.walk(w.G_by_value, q, k, ef, ratio, w.allowed, sized)
        changed += exact[0] != wrong[0] or exact[2:4] != wrong[2:4]
        two = fi.walk_two_heap(w.G, q, k, ef, ratio, w.allowed)
        assert exact[0] == two[0] and bits(exact[1]) == bits(two[1]) and exact[2:4] == two[2:4]
    print(f"coarse distances >= 2^24: {big}, tied: {tied}, queries that change when distances are converted by value: {changed} of {fi.NQ}")
    assert big > 0 and tied > 0, "the world does not reach past 2^24 or has no ties"
    assert changed >= 1, "converting by value changes nothing here: the world cannot tell the two orders apart"
