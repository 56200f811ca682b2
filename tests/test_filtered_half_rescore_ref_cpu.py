"""The yardstick of the half-precision filtered walk with the exact f32 re-score validates itself on the CPU
(tests/filtered_half_rescore_ref.py), before any GPU run: its two forms agree on every case tests/test_gpu_filters_graph_half_rescore.py
runs; the worlds of that file overflow nowhere it assumes they do not, and split where the overflow test needs a split; TieWorld
really tells a kernel that cuts in coarse order from one that sorts first; and the largest list of the documented LDS layout is what
the library computes."""
import ctypes as C
import os

import numpy as np
import pytest

import filtered_half_rescore_ref as fr
import filtered_walk_ref as fw
import half_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "velesdb_amd", "lib", "libvelesdb_hip.so")


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("half_rescore_ref")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = fr.World(root, metric, shape)
        return cache[(metric, shape)]
    return get


@pytest.fixture(scope="module")
def tie_worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("half_rescore_tie")), {}

    def get(metric):
        if metric not in cache:
            cache[metric] = fr.TieWorld(root, metric)
        return cache[metric]
    return get


def test_widths():
    assert fr.widths(10, 64, 4) == (40, 64) and fr.widths(10, 0, 0) == (40, 128) and fr.widths(25, 50, 4) == (100, 100)
    assert fr.widths(10, 300, 1) == (10, 300) and fr.widths(40, 0, 0) == (160, 160) and fr.widths(1, 16, 1) == (1, 16)


# ---- the two forms on every case of the GPU test -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.FILTERS)
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("metric", fr.METRICS)
def test_single_list_form_equals_two_heaps_and_rescore(worlds, metric, shape, prec, name):
    """every (world, precision, filter, k, ef, ratio) of the GPU grid, on the first two queries (the GPU test itself asserts that
    no query of its grid overflows the sized list)"""
    w = worlds(metric, shape)
    v, allowed = w.view(prec), w.filters[name]
    for k, ef in fr.KEF:
        for ratio in fr.RATIOS:
            _, ef_w = fr.widths(k, ef, ratio)
            sized = fw.sized_list(ef_w, int(allowed.sum()), w.n)
            for q in w.qs[:2]:
                a = fr.walk_two_heap(v, q, k, ef, ratio, allowed)
                b = fr.walk(v, q, k, ef, ratio, allowed, sized)
                assert not b[4], (k, ef, ratio, "the sized list overflows")
                assert b[0] == a[0] and bits(b[1]) == bits(a[1]) and b[2:4] == a[2:4], (k, ef, ratio)
                assert all(allowed[i] for i in b[0])


@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_the_overflow_case_splits_the_queries(worlds, metric, prec):
    w = worlds(metric, fr.SHAPES[0])
    v = w.view(prec)
    allowed, qs, max_list, over = fr.overflow_case(w, v, 10, 16, 1)
    assert max_list is not None and 0 < sum(over) < fr.NQ, "no list size splits the queries: the GPU case would be meaningless"
    want = fr.expect_call(v, allowed, 10, 16, 1, fr.ROUTE_AUTO, max_list=max_list, qs=qs)
    assert want[2] == [2 if o else 1 for o in over]


# ---- TieWorld --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", fr.METRICS)
def test_tie_world_tells_the_cut_in_coarse_order_from_a_sort_before_the_cut(tie_worlds, metric):
    w = tie_worlds(metric)
    sizes = np.bincount(w.labels, minlength=40)
    assert all(22 <= sizes[c] <= 37 for c in w.qlabels), sizes[w.qlabels]
    everything = w.filters["all"]
    for prec in fr.PRECISIONS:
        v = w.view(prec)
        # the image of every row is its centre, exactly: coarse distances tie across a cluster
        assert np.array_equal(hr.round_half(w.rows, prec), w.centres[w.labels])
        assert np.array_equal(v.G.rows, w.centres[w.labels])
        for qi, q in enumerate(w.qs):
            cluster = w.labels == w.qlabels[qi]
            sized = fw.sized_list(fr.widths(fr.TIE_K, fr.TIE_EF, 1)[1], w.n, w.n)
            c = fr.coarse(v, q, fr.TIE_K, fr.TIE_EF, 1, everything, sized)
            # no result depends on an overflow: the sized list holds the walk at both ratios, under both filters
            for name in ("all", "half"):
                for ratio in (1, 4):
                    cap = fw.sized_list(fr.widths(fr.TIE_K, fr.TIE_EF, ratio)[1], int(w.filters[name].sum()), w.n)
                    assert not fr.walk(v, q, fr.TIE_K, fr.TIE_EF, ratio, w.filters[name], cap)[4], (name, ratio, qi)
            # the coarse order within the cluster is the row order, all distances equal
            assert len(set(bits(c[1]))) == 1 and list(c[0]) == sorted(c[0]) and all(cluster[i] for i in c[0]), qi
            r1 = fr.walk(v, q, fr.TIE_K, fr.TIE_EF, 1, everything, sized)
            assert r1[0] != list(c[0]), (qi, "the re-score does not reorder the coarse candidates")
            truth = fw.exact_pass(v.F, q, fr.TIE_K, everything)[0]
            assert set(r1[0]) != set(truth), (qi, "the cut in coarse order returns the true top-10: a sort before the cut would pass")
            assert set(r1[0]) == set(c[0])
            r4 = fr.walk(v, q, fr.TIE_K, fr.TIE_EF, 4, everything, sized)
            in_cluster = fw.exact_pass(v.F, q, fr.TIE_K, cluster)
            assert r4[0] == list(in_cluster[0]) and bits(r4[1]) == bits(in_cluster[1]), qi
            assert r4[0] == list(truth)
            two = fr.walk_two_heap(v, q, fr.TIE_K, fr.TIE_EF, 1, everything)
            assert two[0] == r1[0] and bits(two[1]) == bits(r1[1]) and two[2:4] == r1[2:4]


# ---- the largest list follows the layout with the re-score output behind the lists ---------------------------------------------------
def test_the_largest_list_of_the_documented_layout_is_the_library_s():
    """fr.lds_bytes is the layout include/velesdb_hip.h documents; vdb::hnsw_half_rescore_lds_bytes is what the host path sizes every
    walk launch of the call with and searches its largest list over (hnsw_filtered.hip)"""
    assert os.path.exists(LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    fn = C.CDLL(LIB)._ZN3vdb27hnsw_half_rescore_lds_bytesEjjj
    fn.restype, fn.argtypes = C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]
    f32 = C.CDLL(LIB)._ZN3vdb14hnsw_lds_bytesEjjjji
    f32.restype, f32.argtypes = C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    for dim in (37, 256, 512, 768, 1000, 1024):
        for longest, cand_k in ((12, 1), (16, 40), (32, 100), (16, 640), (32, 1600)):
            nbmax = fr.nbmax_of(longest, cand_k)
            for cap in (64, 192, 1024, 4096, 15360, 17984):
                assert fn(cap, nbmax, dim) == fr.lds_bytes(cap, nbmax, dim), (dim, nbmax, cap)
                assert fn(cap, nbmax, dim) == f32(cap, nbmax, dim, 0, 0) + nbmax * 8  # the f32 call's layout and the output behind it
            cap = fr.largest_list(nbmax, dim)
            assert cap % 64 == 0 and fn(cap, nbmax, dim) <= fr.LDS_BUDGET < fn(cap + 64, nbmax, dim), (dim, nbmax, cap)
            # the output behind the lists costs room: never more than the f32 call's largest list at the same nbmax
            cap32 = fr.LDS_BUDGET // 9 // 64 * 64
            while f32(cap32, nbmax, dim, 0, 0) > fr.LDS_BUDGET:
                cap32 -= 64
            assert cap <= cap32 and (cap32 - cap) * 9 <= nbmax * 8 + 64 * 9, (dim, nbmax, cap, cap32)
