"""GPU tests of the half-precision filtered graph walk with the exact f32 re-score (vdb_hip_index_search_graph_filters_half_rescore,
csrc/hnsw_filtered.hip).

Reference: tests/filtered_half_rescore_ref.py — tests/filtered_walk_ref.py over the handle's links and the ROUNDED rows, asked with
the rounded query at (cand_k, ef_w), then the exact f32 re-score over the f32 rows with the unrounded query
(tests/test_filtered_half_rescore_ref_cpu.py holds it to the two-heap form).  Everything is compared bit for bit: ids, ranks, score
bits, out_n, the ~0 / NaN padding, the per-query route and the call's summed n_dist / n_expand.  Shapes: the smallest that reach
every instance of the kernel family — the generic layout with a tail, the register-chunk instances CPL 1 / 2 / 3 / 4, the generic
layout just under the 1024-dimension limit — and TieWorld, whose coarse distances tie across a cluster.
"""
import ctypes as C

import numpy as np
import pytest

import filtered_half_rescore_ref as fr
import filtered_walk_ref as fw
import half_ref as hr
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP = va.DistanceMetric, va.VectorPrecision
METRIC = {hr.COSINE: DM.Cosine, hr.EUCLIDEAN: DM.Euclidean, hr.DOT: DM.DotProduct}
VPREC = {hr.F16: VP.F16, hr.BF16: VP.BF16}
MODE = {hr.F16: va.MODE_HNSW_F16, hr.BF16: va.MODE_HNSW_BF16}
HALF_BITS = {hr.F16: va.KERNEL_HNSW_HALF | va.KERNEL_F16, hr.BF16: va.KERNEL_HNSW_HALF}
NQ = fr.NQ
INVALID, UNSUPPORTED, STATE = -1, -7, -8
SHAPE_IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def walk_bits(prec):
    return va.KERNEL_HALF_RESCORE | va.KERNEL_HNSW_FILTERED | HALF_BITS[prec]


class Handle:
    """the GPU side of a world: the handle that loaded its dump, both images enabled, the named filters as handles"""

    def __init__(self, world):
        n, dim, M, efc = world.shape
        self.w, self.M = world, M
        self.ix = va.HnswIndex(dim, METRIC[world.metric], va.HnswParams(M, efc, n))
        self.ix.load_reference_files(world.dir, fr.BASE)
        for p in fr.PRECISIONS:
            self.ix.enable_half_precision(VPREC[p])
        self._flt = {}

    def flt(self, name):  # (created after the load: a load renumbers the rows)
        if name is None:
            return None
        if name not in self._flt:
            self._flt[name] = self.ix.create_filter(np.flatnonzero(self.w.filters[name]).astype(np.uint64))
            assert self._flt[name].matched == int(self.w.filters[name].sum())
        return self._flt[name]

    def largest(self, k, ratio):
        """the call's largest list by the documented layout: the longest neighbour list of the graph is layer 0's 2 * M"""
        return fr.largest_list(fr.nbmax_of(2 * self.M, k * (ratio or 4)), self.w.dim)

    def close(self):
        for f in self._flt.values():
            f.close()
        self.ix.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("filters_graph_half_rescore")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            w = fr.TieWorld(root, metric) if shape == "tie" else fr.World(root, metric, shape)
            cache[(metric, shape)] = (w, Handle(w))
        return cache[(metric, shape)]
    yield get
    for _, h in cache.values():
        h.close()


def batch(ix, qs, k, filters, prec, ef, ratio=0, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_with_filters_half_rescore(qs, k, filters, MODE[prec], ef=ef, oversampling=ratio, route=route,
                                                            max_list=max_list)
    return out, routes, ix.last_search_stats(), ix.last_kernels()


def one(ix, qs, k, flt, prec, ef, ratio=0, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_filtered_graph_half_rescore(qs, k, flt, MODE[prec], ef=ef, oversampling=ratio, route=route,
                                                              max_list=max_list)
    return out, routes, ix.last_search_stats()


def same_bits(a, b):
    (ai, asc, ac), (bi, bsc, bc) = a, b
    return np.array_equal(ai, bi) and np.array_equal(asc.view(np.uint32), bsc.view(np.uint32)) and np.array_equal(ac, bc)


def raw_call(ix, mode, handles, fq, qs, k, ef=64, ratio=0, route=0, max_list=0):
    """the entry point with a hand-made table -> (status, ids, scores, counts, routes); the outputs start as a known pattern"""
    from velesdb_amd import _ffi
    nq = qs.shape[0]
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    ids, sc = np.full((nq, max(k, 1)), 7, dtype=np.uint64), np.full((nq, max(k, 1)), 7.0, dtype=np.float32)
    cnt, routes = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint32)
    fq = np.asarray(fq, dtype=np.uint32)
    table = (C.c_void_p * max(len(handles), 1))(*handles)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().vdb_hip_index_search_graph_filters_half_rescore(ix._h, mode, table if handles else None, len(handles), p(fq), p(qs),
                                                                    nq, k, ef, ratio, route, max_list, p(ids), p(sc), p(cnt), p(routes))
    return rc, ids, sc, cnt, routes


def untouched(r):
    return np.all(r[1] == 7) and np.all(r[2] == 7.0) and np.all(r[3] == 7) and np.all(r[4] == 7)


# ---- 1. against the CPU reference: (k, ef) x ratio x routes, per world, precision and filter ----------------------------------------
def against_reference(w, h, prec, name, kefs, ratios):
    v, allowed, walked = w.view(prec), w.filters[name], 0
    for k, ef in kefs:
        for ratio in ratios:
            cap_max = h.largest(k, ratio)
            wants = {va.ROUTE_WALK: fr.expect_call(v, allowed, k, ef, ratio, va.ROUTE_WALK, max_list=cap_max),
                     va.ROUTE_EXACT: fr.expect_call(v, allowed, k, ef, ratio, va.ROUTE_EXACT, max_list=cap_max)}
            wants[va.ROUTE_AUTO] = fr.expect_call(v, allowed, k, ef, ratio, va.ROUTE_AUTO, max_list=cap_max)
            assert wants[va.ROUTE_WALK][2] == [1] * NQ, "the reference itself overflows the largest list at this shape"
            for route, want in wants.items():
                got = one(h.ix, w.qs, k, h.flt(name), prec, ef, ratio, route=route)
                kern = h.ix.last_kernels()
                assert kern == (va.KERNEL_FILTER_RANK if want[2] == [2] * NQ else walk_bits(prec)), (name, k, ef, ratio, route, hex(kern))
                fr.assert_call(got, want, (name, prec, k, ef, ratio, route))
                assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])
                walked += want[2] == [1] * NQ
    return walked


@pytest.mark.parametrize("name", fr.FILTERS)
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_equals_the_reference(worlds, metric, shape, prec, name):
    w, h = worlds(metric, shape)
    assert against_reference(w, h, prec, name, fr.KEF, fr.RATIOS) >= len(fr.KEF) * len(fr.RATIOS)


@pytest.mark.parametrize("name", ["all", "half"])
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_tie_world_equals_the_reference(worlds, metric, prec, name):
    """coarse distances tie across a cluster: at ratio 1 the cut to cand_k is made in coarse (row) order, and equal exact distances
    keep it (tests/test_filtered_half_rescore_ref_cpu.py shows that a sort before the cut answers differently here)"""
    w, h = worlds(metric, "tie")
    against_reference(w, h, prec, name, [(fr.TIE_K, fr.TIE_EF)], [1, 4])


@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_queries_that_overflow_the_largest_list_take_the_exact_pass_alone(worlds, metric, prec):
    """fr.overflow_case: max_list is chosen from the peaks of the reference's own lists so that some but not all queries overflow it"""
    (w, h), k, ef, ratio = worlds(metric, fr.SHAPES[0]), 10, 16, 1
    v = w.view(prec)
    allowed, qs, chosen, over = fr.overflow_case(w, v, k, ef, ratio)
    assert chosen is not None, "no list size splits the queries: the case is meaningless"
    want = fr.expect_call(v, allowed, k, ef, ratio, va.ROUTE_AUTO, max_list=chosen, qs=qs)
    assert want[2] == [2 if o else 1 for o in over]
    print(f"metric {metric} precision {prec}: max_list {chosen}, routes {want[2]}")
    with h.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as flt:
        got = one(h.ix, qs, k, flt, prec, ef, ratio, max_list=chosen)
        assert h.ix.last_kernels() == walk_bits(prec) | va.KERNEL_FILTER_RANK
        fr.assert_call(got, want, ("fallback", chosen))
        # route 1: the queries that overflow the largest list fail the whole call, and nothing is written
        with pytest.raises(va.VelesHipError) as e:
            h.ix.search_batch_filtered_graph_half_rescore(qs, k, flt, MODE[prec], ef=ef, oversampling=ratio, route=va.ROUTE_WALK,
                                                          max_list=chosen)
        assert e.value.code == UNSUPPORTED and f"{sum(over)} queries overflow" in str(e.value), str(e.value)
        r = raw_call(h.ix, MODE[prec], [flt._h], [0] * NQ, qs, k, ef=ef, ratio=ratio, route=va.ROUTE_WALK, max_list=chosen)
        assert r[0] == UNSUPPORTED and untouched(r)


# ---- 2. GPU against GPU, no Python walk: the half call's list at (cand_k, ef_w), re-sorted by the oracle's exact distances ------------
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", list(fr.SHAPES) + ["tie"], ids=lambda s: s if s == "tie" else SHAPE_IDS(s))
@pytest.mark.parametrize("metric", fr.METRICS)
def test_is_the_stable_exact_sort_of_the_half_call_s_list(worlds, metric, shape, prec):
    w, h = worlds(metric, shape)
    pm = w.view(prec).metric
    for name in ("all", "half", "tenth"):
        if name not in w.filters:
            continue
        for k, ef, ratio in ((10, 64, 4), (10, 64, 1), (25, 50, 4), (1, 16, 1), (10, 0, 0)):
            cand_k, ef_w = fr.widths(k, ef, ratio)
            (cid, _, ccnt), croutes = h.ix.search_batch_filtered_graph_half(w.qs, cand_k, h.flt(name), MODE[prec], ef=ef_w, route=va.ROUTE_WALK)
            cstats = h.ix.last_search_stats()
            (ids, sc, cnt), routes, stats = one(h.ix, w.qs, k, h.flt(name), prec, ef, ratio, route=va.ROUTE_WALK)
            assert np.all(routes == 1) and np.all(croutes == 1) and tuple(stats) == tuple(cstats), (name, k, ef, ratio, stats, cstats)
            for qi in range(NQ):
                coarse = cid[qi, :int(ccnt[qi])].astype(np.int64)
                ds = po.batch_distance(pm, w.qs[qi], w.rows[coarse], po.MODE_C)
                order = sorted(range(len(coarse)), key=lambda i: fw.tkey(ds[i]))[:k]
                assert int(cnt[qi]) == len(order) and ids[qi, :len(order)].tolist() == coarse[order].tolist(), (name, k, ef, ratio, qi)
                assert np.array_equal(sc[qi, :len(order)].view(np.uint32), fw.score_bits(pm, [ds[i] for i in order])), (name, k, ef, ratio, qi)


# ---- 3. the rounded world: rows that equal their image, rounded queries -> the f32 per-query call at ef_w, bit for bit ------------------
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("dim", [37, 256, 768, 1024])
@pytest.mark.parametrize("metric", fr.METRICS)
def test_rounded_world_is_the_f32_call_at_ef_w(metric, dim, prec):
    n = 1000
    rng = np.random.default_rng(37 * dim + 7 * metric + prec)
    rows = hr.round_half(rng.standard_normal((n, dim)).astype(np.float32), prec)
    qs = hr.round_half(rng.standard_normal((NQ, dim)).astype(np.float32), prec)
    if metric == hr.COSINE:  # the one place the two calls may differ: a norm below f32::EPSILON
        assert np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1)).min() > 1.0
        assert np.sqrt((qs.astype(np.float64) ** 2).sum(axis=1)).min() > 1.0
    ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(8, 60, n))
    ix.insert_batch_parallel([(i, rows[i]) for i in range(n)], 64)
    ix.enable_half_precision(VPREC[prec])
    frng = np.random.default_rng(dim)
    half = ix.create_filter(np.flatnonzero(fw.random_filter(frng, n, 0.5)).astype(np.uint64))
    tenth = ix.create_filter(np.flatnonzero(fw.random_filter(frng, n, 0.1)).astype(np.uint64))
    filters = [(half, tenth, None)[i % 3] for i in range(NQ)]
    for k, ef, ratio in ((10, 64, 4), (25, 50, 4), (10, 64, 1)):
        _, ef_w = fr.widths(k, ef, ratio)
        for route in (va.ROUTE_AUTO, va.ROUTE_EXACT):
            got, routes, stats, kern = batch(ix, qs, k, filters, prec, ef, ratio, route=route)
            want, wroutes = ix.search_batch_with_filters(qs, k, filters, ef=ef_w, route=route)
            wstats, wkern = ix.last_search_stats(), ix.last_kernels()
            assert same_bits(got, want), (metric, dim, prec, route, k, ef, ratio)
            assert np.array_equal(routes, wroutes) and tuple(stats) == tuple(wstats), (routes, wroutes, stats, wstats)
            assert kern == (wkern | HALF_BITS[prec] | va.KERNEL_HALF_RESCORE if route == va.ROUTE_AUTO else va.KERNEL_FILTER_RANK), hex(kern)
            assert np.all(got[2] > 0)
    half.close()
    tenth.close()
    ix.close()


# ---- 4. one distance on both routes; no filters; mixed batches -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_same_score_bits_on_both_routes_and_the_kernel_mask(worlds, metric, shape, prec):
    (w, h), k, ef = worlds(metric, shape), 10, 64
    got_e = one(h.ix, w.qs, k, h.flt("half"), prec, ef, route=va.ROUTE_EXACT)
    assert h.ix.last_kernels() == va.KERNEL_FILTER_RANK, hex(h.ix.last_kernels())
    # (the exact pass IS the f32 call's)
    f32 = h.ix.search_batch_filtered_graph(w.qs, k, h.flt("half"), ef=ef, route=va.ROUTE_EXACT)
    assert same_bits(got_e[0], f32[0]) and np.array_equal(got_e[1], f32[1]) and tuple(got_e[2]) == tuple(h.ix.last_search_stats())
    got_w = one(h.ix, w.qs, k, h.flt("half"), prec, ef, route=va.ROUTE_WALK)
    assert h.ix.last_kernels() == walk_bits(prec), hex(h.ix.last_kernels())
    common = 0
    for qi in range(NQ):
        ce, cw = int(got_e[0][2][qi]), int(got_w[0][2][qi])
        exact = dict(zip(got_e[0][0][qi, :ce].tolist(), got_e[0][1][qi, :ce].view(np.uint32).tolist()))
        for i, s in zip(got_w[0][0][qi, :cw].tolist(), got_w[0][1][qi, :cw].view(np.uint32).tolist()):
            if i in exact:
                common += 1
                assert exact[i] == s, (qi, i)
    assert common > NQ * k // 2


@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_no_filters(worlds, metric, shape, prec):
    """n_filters = 0, "no filter" everywhere in a table of one, the all-rows filter and search_batch_half_rescore: one answer, the
    reference's; oversampling 0 is 4"""
    (w, h), k, ef = worlds(metric, shape), 10, 64
    v = w.view(prec)
    want = fr.expect_call(v, w.filters["all"], k, ef, 4, va.ROUTE_AUTO)
    a = batch(h.ix, w.qs, k, [None] * NQ, prec, ef, 4)
    assert a[3] == walk_bits(prec), hex(a[3])
    fr.assert_call(a[:3], want, "n_filters = 0")
    b = batch(h.ix, w.qs, k, [None] * NQ, prec, ef, 0)
    c = batch(h.ix, w.qs, k, [h.flt("all")] * NQ, prec, ef, 4)
    for other in (b, c):
        assert same_bits(a[0], other[0]) and np.array_equal(a[1], other[1]) and tuple(a[2]) == tuple(other[2])
    r = raw_call(h.ix, MODE[prec], [h.flt("half")._h], [1] * NQ, w.qs, k, ef=ef, ratio=4)  # a table of one, nobody on it
    assert r[0] == 0 and same_bits(a[0], (r[1], r[2], r[3])) and np.all(r[4] == 1)
    plain = h.ix.search_batch_half_rescore(w.qs, k, MODE[prec], ef=ef)
    assert same_bits(a[0], plain)


@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", [fr.SHAPES[0], fr.SHAPES[3]], ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fr.METRICS)
def test_mixed_batch_equals_the_one_query_calls(worlds, metric, shape, prec):
    (w, h), k, ef = worlds(metric, shape), 10, 64
    with h.ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        for order in (list(range(NQ)), list(reversed(range(NQ)))):
            kinds = [("half", "tenth", "few", None, "empty")[i % 5] for i in order]
            filters = [empty if n == "empty" else h.flt(n) for n in kinds]
            qs = w.qs[order]
            (ids, sc, cnt), routes, stats, kern = batch(h.ix, qs, k, filters, prec, ef)
            assert kern == walk_bits(prec) | va.KERNEL_FILTER_RANK, hex(kern)
            nd = ne = 0
            for qi in range(NQ):
                (i1, s1, c1), r1, st1, k1 = batch(h.ix, qs[qi:qi + 1], k, [filters[qi]], prec, ef)
                nd, ne = nd + st1[0], ne + st1[1]
                assert int(routes[qi]) == int(r1[0]) == {"few": 2, "empty": 0}.get(kinds[qi], 1), (qi, kinds[qi])
                assert np.array_equal(ids[qi], i1[0]) and np.array_equal(sc[qi].view(np.uint32), s1[0].view(np.uint32)), (qi, kinds[qi])
                assert cnt[qi] == c1[0], (qi, kinds[qi])
                if kinds[qi] == "empty":  # out_n = 0 and route 0 while the others are answered
                    assert cnt[qi] == 0 and k1 == 0 and np.all(ids[qi] == fr.PAD_ID) and np.all(sc[qi].view(np.uint32) == 0x7FC00000)
                else:
                    assert cnt[qi] == k
            assert tuple(stats) == (nd, ne)


# ---- 5. dead rows, life cycle and refusals -----------------------------------------------------------------------------------------------
def test_dead_rows_and_refusals(tmp_path):
    w = fr.World(str(tmp_path), hr.EUCLIDEAN, fr.SHAPES[0])
    n, dim, M, efc = w.shape
    k, ef, qs = 10, 32, w.qs
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, n))
    ix.load_reference_files(w.dir, fr.BASE)
    base = w.filters["half"]
    flt = ix.create_filter(np.flatnonzero(base).astype(np.uint64))
    # a handle without the image; then with only the other precision's
    r = raw_call(ix, va.MODE_HNSW_BF16, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    ix.enable_half_precision(VP.F16)
    r = raw_call(ix, va.MODE_HNSW_BF16, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    ix.enable_half_precision(VP.BF16)

    def check(allowed, ctx, route):
        for p in fr.PRECISIONS:
            got = one(ix, qs, k, flt, p, ef, route=route)
            assert ix.last_kernels() == (va.KERNEL_FILTER_RANK if route == va.ROUTE_EXACT else walk_bits(p)), (ctx, hex(ix.last_kernels()))
            want = fr.expect_call(w.view(p), allowed, k, ef, 4, route, matched=flt.matched)
            assert 2 not in want[2] or route == va.ROUTE_EXACT
            fr.assert_call(got, want, (ctx, p))
            yield got[0]

    list(check(base, "fresh", va.ROUTE_WALK))
    # rows removed after the filter was made are absent on both routes, and out_n is not shortened by a post-drop: the dead rows
    # are each query's nearest allowed ones
    live = np.ones(n, dtype=bool)
    first = one(ix, qs, k, flt, hr.F16, ef, route=va.ROUTE_WALK)[0]
    for row in sorted({int(i) for i in first[0][:, :3].reshape(-1)}):
        assert ix.remove(row)
        live[row] = False
    for route in (va.ROUTE_WALK, va.ROUTE_EXACT):
        for ids, _, cnt in check(base & live, "after removes", route):
            assert np.all(cnt == k) and all(live[i] for i in ids.reshape(-1))
    # refusals: the outputs keep their pattern
    before = one(ix, qs, k, flt, hr.F16, ef)
    for mode in (va.MODE_HNSW, va.MODE_BRUTE_F16, va.MODE_AUTO, va.MODE_HNSW_INT8):
        r = raw_call(ix, mode, [flt._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == UNSUPPORTED and untouched(r), mode
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h], [0] * NQ, qs, k, ef=ef, ratio=65)
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h], [0] * NQ, qs, k, ef=ef, route=3)
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h, None], [0] * NQ, qs, k, ef=ef)  # a NULL table entry, used or not
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h], [0] * (NQ - 1) + [2], qs, k, ef=ef)  # a query names a filter behind "no filter"
    assert r[0] == INVALID and untouched(r)
    other = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    other.insert_batch_parallel([(i, w.rows[i]) for i in range(64)], 16)
    other.enable_half_precision(VP.F16)
    with other.create_filter(np.arange(10, dtype=np.uint64)) as foreign:
        r = raw_call(ix, va.MODE_HNSW_F16, [flt._h, foreign._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == INVALID and untouched(r)
    other.close()
    ham = va.HnswIndex(dim, DM.Hamming, va.HnswParams(8, 60, 64))
    ham.insert_batch_parallel([(i, (w.rows[i] > 0).astype(np.float32)) for i in range(64)], 16)
    with ham.create_filter(np.arange(10, dtype=np.uint64)) as fham:
        for mode in (va.MODE_HNSW_F16, va.MODE_HNSW_BF16):
            r = raw_call(ham, mode, [fham._h], [0] * NQ, qs, k, ef=ef)
            assert r[0] == UNSUPPORTED and untouched(r)
    ham.close()
    group = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    group.insert_batch_parallel([(i, w.rows[i]) for i in range(64)], 16)
    group.enable_half_precision(VP.F16)
    r = raw_call(group, va.MODE_HNSW_F16, [], [0] * NQ, qs, k, ef=ef)
    assert r[0] == UNSUPPORTED and untouched(r)
    group.close()
    nograph = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    nograph.upload(np.arange(64), w.rows[:64])
    nograph.enable_half_precision(VP.F16)
    with nograph.create_filter(np.arange(10, dtype=np.uint64)) as f2:
        r = raw_call(nograph, va.MODE_HNSW_F16, [f2._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == STATE and untouched(r)
    nograph.close()
    # the existing calls keep refusing what they refused: rerank over the half walks, the half modes on the f32 filtered call
    with pytest.raises(va.VelesHipError) as e:
        ix.search_batch_filtered_graph(qs, k, flt, ef=ef, mode=va.MODE_HNSW_F16)
    assert e.value.code == UNSUPPORTED
    # the handle is as usable as before; oversampling 0 is 4
    after = one(ix, qs, k, flt, hr.F16, ef, 4)
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1]) and tuple(before[2]) == tuple(after[2])
    # vacuum renumbers the rows: the filter is stale
    ix.vacuum()
    for p in fr.PRECISIONS:
        r = raw_call(ix, MODE[p], [flt._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == STATE and untouched(r)
    flt.close()
    ix.close()
