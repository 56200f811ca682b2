"""GPU tests of the filtered graph search over the half-precision images (vdb_hip_index_search_graph_filters_half,
csrc/hnsw_filtered.hip).

Reference: tests/filtered_walk_ref.py over an oracle graph with the handle's links and the ROUNDED vectors, asked with rounded
queries (tests/filtered_half_world.py) — the product of the two references the f32 filtered walk and the plain half walk are
tested against.  Everything is compared bit for bit: ids, ranks, score bits, out_n, padding, the per-query route and the call's
n_dist / n_expand.  Shapes are tests/half_walk_ref.py's (CPL 0, CPL 3, dim % 4 != 0); the register-chunk instances CPL 1 / 2 / 4, the
LDS-resident query and the tail chunk are covered by the dequantised twin, which needs no oracle: on rows that equal their image the
call must equal the f32 per-query call.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import filtered_half_world as fh
import filtered_walk_ref as fw
import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP = va.DistanceMetric, va.VectorPrecision
METRIC = {hr.COSINE: DM.Cosine, hr.EUCLIDEAN: DM.Euclidean, hr.DOT: DM.DotProduct}
VPREC = {hr.F16: VP.F16, hr.BF16: VP.BF16}
MODE = {hr.F16: va.MODE_HNSW_F16, hr.BF16: va.MODE_HNSW_BF16}
HALF_BITS = {hr.F16: va.KERNEL_HNSW_HALF | va.KERNEL_F16, hr.BF16: va.KERNEL_HNSW_HALF}
NQ = fh.NQ
INVALID, UNSUPPORTED, STATE = -1, -7, -8
OTHER_KERNELS = ~(va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK | va.KERNEL_HNSW_HALF | va.KERNEL_F16)


class GpuWorld(fh.World):
    """a world with the GPU handle that loaded its dump, both images enabled, and the named filters as handles"""

    def __init__(self, root, metric, shape):
        super().__init__(root, metric, shape)
        n, dim, M, efc = shape
        self.ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
        self.ix.load_reference_files(self.dir, fh.BASE)
        for p in fh.PRECISIONS:
            self.ix.enable_half_precision(VPREC[p])
        self._flt = {}

    def flt(self, name):  # (created after the load: a load renumbers the rows)
        if name is None:
            return None
        if name not in self._flt:
            self._flt[name] = self.ix.create_filter(np.flatnonzero(self.filters[name]).astype(np.uint64))
            assert self._flt[name].matched == int(self.filters[name].sum())
        return self._flt[name]

    def close(self):
        for f in self._flt.values():
            f.close()
        self.ix.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("filters_graph_half")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = GpuWorld(root, metric, shape)
        return cache[(metric, shape)]
    yield get
    for w in cache.values():
        w.close()


def batch(ix, qs, k, filters, prec, ef, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_with_filters_half(qs, k, filters, MODE[prec], ef=ef, route=route, max_list=max_list)
    return out, routes, ix.last_search_stats(), ix.last_kernels()


def one(ix, qs, k, flt, prec, ef, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_filtered_graph_half(qs, k, flt, MODE[prec], ef=ef, route=route, max_list=max_list)
    return out, routes, ix.last_search_stats()


def same_bits(a, b):
    (ai, asc, ac), (bi, bsc, bc) = a, b
    return np.array_equal(ai, bi) and np.array_equal(asc.view(np.uint32), bsc.view(np.uint32)) and np.array_equal(ac, bc)


# ---- 1. no query filtered: the call IS search_batch(mode) --------------------------------------------------------------------------
@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", fh.METRICS)
def test_no_filter_is_the_plain_half_walk(worlds, metric, shape, prec):
    w = worlds(metric, shape)
    for k, ef in hw.KEF:
        pid, psc, pcnt = w.ix._search_raw(w.qs, k, ef, MODE[prec])
        pstats = w.ix.last_search_stats()
        assert w.ix.last_kernels() & va.KERNEL_HNSW_HALF
        for filters in ([None] * NQ, [w.flt("all")] * NQ, [None if i % 2 else w.flt("all") for i in range(NQ)]):
            (ids, sc, cnt), routes, stats, kern = batch(w.ix, w.qs, k, filters, prec, ef)
            assert kern == va.KERNEL_HNSW_FILTERED | HALF_BITS[prec], hex(kern)
            assert np.all(routes == 1)
            assert np.array_equal(cnt, pcnt) and tuple(stats) == tuple(pstats), (k, ef, stats, pstats)
            # (whole blocks: the padding of both calls is id 2^64 - 1 / the canonical NaN)
            assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)), (k, ef)


# ---- 2. random and clustered filters against the single-list reference over the rounded rows ---------------------------------------
@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("name", ["half", "tenth", "clustered"])
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", fh.METRICS)
def test_filtered_half_walk_equals_the_single_list_reference(worlds, metric, shape, name, prec):
    w, k, ef = worlds(metric, shape), 10, 64
    v, allowed = w.view(prec), w.filters[name]
    want = fh.expect_call(v, allowed, k, ef, va.ROUTE_WALK)
    assert want[2] == [1] * NQ, "the reference itself overflows at this shape"
    got = one(w.ix, w.qs, k, w.flt(name), prec, ef, route=va.ROUTE_WALK)
    assert w.ix.last_kernels() == va.KERNEL_HNSW_FILTERED | HALF_BITS[prec], hex(w.ix.last_kernels())
    fh.assert_call(got, want, (metric, shape, name, prec))
    assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])


# ---- 3. routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", fh.METRICS)
def test_routes(worlds, metric, shape, prec):
    w, k, ef = worlds(metric, shape), 10, 64
    v, few = w.view(prec), w.filters["few"]
    assert int(few.sum()) < ef
    # auto: the walk could never fill its result set -> the exact pass for every query, over the rounded rows
    got = one(w.ix, w.qs, k, w.flt("few"), prec, ef)
    assert w.ix.last_kernels() == va.KERNEL_FILTER_RANK | HALF_BITS[prec], hex(w.ix.last_kernels())
    want = fh.expect_call(v, few, k, ef, va.ROUTE_AUTO)
    assert want[2] == [2] * NQ and want[3] == (NQ * int(few.sum()), 0)
    fh.assert_call(got, want, "auto, few")
    assert np.all(got[0][2] == min(k, int(few.sum())))
    for qi in range(NQ):
        e = fw.exact_pass(v.G, v.qs[qi], k, few)
        assert got[0][0][qi, :len(e[0])].tolist() == list(e[0])
    # the exact pass on demand, and the walk: one distance function — an id both routes return has the same score bits
    got_e = one(w.ix, w.qs, k, w.flt("half"), prec, ef, route=va.ROUTE_EXACT)
    assert w.ix.last_kernels() == va.KERNEL_FILTER_RANK | HALF_BITS[prec]
    fh.assert_call(got_e, fh.expect_call(v, w.filters["half"], k, ef, va.ROUTE_EXACT), "exact, half")
    got_w = one(w.ix, w.qs, k, w.flt("half"), prec, ef, route=va.ROUTE_WALK)
    common = 0
    for qi in range(NQ):
        ce, cw = int(got_e[0][2][qi]), int(got_w[0][2][qi])
        exact = dict(zip(got_e[0][0][qi, :ce].tolist(), got_e[0][1][qi, :ce].view(np.uint32).tolist()))
        for i, s in zip(got_w[0][0][qi, :cw].tolist(), got_w[0][1][qi, :cw].view(np.uint32).tolist()):
            if i in exact:
                common += 1
                assert exact[i] == s, (qi, i)
    assert common > NQ * k // 2


def raw_call(ix, mode, handles, fq, qs, k, ef=64, route=0, max_list=0):
    """the entry point with a hand-made table -> (status, ids, scores, counts, routes); the outputs start as a known pattern"""
    from velesdb_amd import _ffi
    nq = qs.shape[0]
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    ids, sc = np.full((nq, max(k, 1)), 7, dtype=np.uint64), np.full((nq, max(k, 1)), 7.0, dtype=np.float32)
    cnt, routes = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint32)
    fq = np.asarray(fq, dtype=np.uint32)
    table = (C.c_void_p * max(len(handles), 1))(*handles)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().vdb_hip_index_search_graph_filters_half(ix._h, mode, table if handles else None, len(handles), p(fq), p(qs), nq, k,
                                                            ef, route, max_list, p(ids), p(sc), p(cnt), p(routes))
    return rc, ids, sc, cnt, routes


def untouched(r):
    return np.all(r[1] == 7) and np.all(r[2] == 7.0) and np.all(r[3] == 7) and np.all(r[4] == 7)


@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("metric", fh.METRICS)
def test_queries_that_overflow_the_largest_list_take_the_exact_pass_alone(worlds, metric, prec):
    """The end-clustered filter and shifted queries of tests/test_gpu_filtered_graph.py: max_list is chosen with the reference over
    the rounded rows so that some but not all of the 20 queries overflow it."""
    w, k, ef = worlds(metric, hw.SHAPES[0]), 10, 16
    v = w.view(prec)
    allowed = np.zeros(w.n, dtype=bool)
    allowed[np.argsort(w.rows[:, 0])[-w.n // 10:]] = True
    qs = w.qs.copy()
    qs[:, 0] += np.resize(np.array([30, -30, 0, -4, -8, -2], dtype=np.float32), NQ)
    rqs = hr.round_half(qs, prec)
    ef_eff, matched = fw.ef_rule(k, ef), int(allowed.sum())
    sized = fw.sized_list(ef_eff, matched, w.n)
    chosen = None
    for max_list in (4 * sized, 2 * sized, sized):  # (below `sized` the auto rule sends the whole call to the exact pass)
        over = [fh.protocol(v.G, q, k, ef_eff, allowed, sized, max_list)[1] for q in rqs]
        if 0 < sum(over) < NQ:
            chosen = max_list
            break
    assert chosen is not None, "no list size splits the queries: the case is meaningless"
    want = fh.expect_call(v, allowed, k, ef, va.ROUTE_AUTO, max_list=chosen, qs=rqs)
    assert want[2] == [2 if o else 1 for o in over]
    print(f"metric {metric} precision {prec}: max_list {chosen} (first list {sized}), routes {want[2]}")
    with w.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as flt:
        got = one(w.ix, qs, k, flt, prec, ef, max_list=chosen)
        assert w.ix.last_kernels() == va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK | HALF_BITS[prec]
        fh.assert_call(got, want, ("fallback", chosen))
        # route 1: the queries that overflow the largest list fail the whole call, and nothing is written
        with pytest.raises(va.VelesHipError) as e:
            w.ix.search_batch_filtered_graph_half(qs, k, flt, MODE[prec], ef=ef, route=va.ROUTE_WALK, max_list=chosen)
        assert e.value.code == UNSUPPORTED and f"{sum(over)} queries overflow" in str(e.value), str(e.value)
        r = raw_call(w.ix, MODE[prec], [flt._h], [0] * NQ, qs, k, ef=ef, route=va.ROUTE_WALK, max_list=chosen)
        assert r[0] == UNSUPPORTED and untouched(r)


# ---- 4. the per-query contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", fh.METRICS)
def test_mixed_batch_equals_the_one_query_calls(worlds, metric, shape, prec):
    w, k, ef = worlds(metric, shape), 10, 64
    with w.ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        kinds = [("half", "tenth", "few", None, "empty")[i % 5] for i in range(NQ)]
        filters = [empty if n == "empty" else w.flt(n) for n in kinds]
        (ids, sc, cnt), routes, stats, kern = batch(w.ix, w.qs, k, filters, prec, ef)
        assert kern == va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK | HALF_BITS[prec], hex(kern)
        nd = ne = 0
        for qi in range(NQ):
            (i1, s1, c1), r1, st1, k1 = batch(w.ix, w.qs[qi:qi + 1], k, [filters[qi]], prec, ef)
            nd, ne = nd + st1[0], ne + st1[1]
            assert int(routes[qi]) == int(r1[0]) == {"few": 2, "empty": 0}.get(kinds[qi], 1), (qi, kinds[qi])
            assert np.array_equal(ids[qi], i1[0]) and np.array_equal(sc[qi].view(np.uint32), s1[0].view(np.uint32)), (qi, kinds[qi])
            assert cnt[qi] == c1[0], (qi, kinds[qi])
            if kinds[qi] == "empty":
                assert cnt[qi] == 0 and k1 == 0 and np.all(ids[qi] == fh.PAD_ID) and np.all(sc[qi].view(np.uint32) == 0x7FC00000)
        assert tuple(stats) == (nd, ne)


# ---- 5. the dequantised twin: rows that equal their image, rounded queries -> the f32 per-query call, bit for bit --------------------
@pytest.mark.parametrize("prec", fh.PRECISIONS)
@pytest.mark.parametrize("dim", [256, 512, 1024, 1536, 4099])
@pytest.mark.parametrize("metric", fh.METRICS)
def test_dequantised_twin(metric, dim, prec):
    n, k, ef = 1000, 10, 64
    rng = np.random.default_rng(31 * dim + 7 * metric + prec)
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
    for route in (va.ROUTE_AUTO, va.ROUTE_EXACT):
        got, routes, stats, kern = batch(ix, qs, k, filters, prec, ef, route=route)
        want, wroutes = ix.search_batch_with_filters(qs, k, filters, ef=ef, route=route)
        wstats, wkern = ix.last_search_stats(), ix.last_kernels()
        assert same_bits(got, want), (metric, dim, prec, route)
        assert np.array_equal(routes, wroutes) and tuple(stats) == tuple(wstats), (routes, wroutes, stats, wstats)
        assert kern == wkern | HALF_BITS[prec] and not wkern & OTHER_KERNELS, (hex(kern), hex(wkern))
        assert np.all(got[2] > 0)
    half.close()
    tenth.close()
    ix.close()


# ---- 6. life cycle and refusals ----------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(va.VelesHipError) as e:
        fn()
    return e.value.code


class Live:
    """a graph built row by row on both sides (the GPU's sequential insert == the oracle's, link for link); the reference views are
    re-made from a fresh dump of the oracle graph whenever it grew"""

    def __init__(self, root, n, dim, seed):
        rng = np.random.default_rng(seed)
        self.root, self.metric, self.dim, self.n, self.gen = root, hr.EUCLIDEAN, dim, 0, 0
        self.all_rows = rng.standard_normal((n + 64, dim)).astype(np.float32)
        self.raw_qs = rng.standard_normal((NQ, dim)).astype(np.float32)
        self.g = po.NativeHnsw(dim, po.EUCLIDEAN, 8, 60, po.MODE_C)
        self.g.set_build_tie(po.TIE_CANONICAL)
        self.ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, n + 64))

    def grow(self, to):
        for i in range(self.n, to):
            self.g.insert(self.all_rows[i])
            self.ix.insert(i, self.all_rows[i])
        self.n, self.gen = to, self.gen + 1
        d = os.path.join(self.root, f"live{self.gen}")
        os.makedirs(d)
        self.g.file_dump(d, fh.BASE)
        self.views = {}
        for p in fh.PRECISIONS:
            self.views[p] = types.SimpleNamespace(G=fh.half_graph(d, p, hr.EUCLIDEAN, self.dim), n=to, metric=po.EUCLIDEAN,
                                                  qs=hr.round_half(self.raw_qs, p))


def test_life_cycle_and_refusals(tmp_path):
    L = Live(str(tmp_path), 500, 32, 21)
    L.grow(500)
    ix, k, ef, qs = L.ix, 10, 32, L.raw_qs
    rng = np.random.default_rng(22)
    base = fw.random_filter(rng, L.n, 0.3)
    flt = ix.create_filter(np.flatnonzero(base).astype(np.uint64))
    # a handle without the image; then with only the other precision's
    assert code_of(lambda: ix.search_batch_filtered_graph_half(qs, k, flt, va.MODE_HNSW_F16, ef=ef)) == STATE
    r = raw_call(ix, va.MODE_HNSW_BF16, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    ix.enable_half_precision(VP.F16)
    r = raw_call(ix, va.MODE_HNSW_BF16, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    ix.enable_half_precision(VP.BF16)

    def check(f, allowed, ctx, route=va.ROUTE_WALK):
        outs = []
        for p in fh.PRECISIONS:
            got = one(ix, qs, k, f, p, ef, route=route)
            kern = ix.last_kernels()
            assert kern == (va.KERNEL_FILTER_RANK if route == va.ROUTE_EXACT else va.KERNEL_HNSW_FILTERED) | HALF_BITS[p], (ctx, hex(kern))
            want = fh.expect_call(L.views[p], allowed, k, ef, route, matched=f.matched)
            assert 2 not in want[2] or route == va.ROUTE_EXACT
            fh.assert_call(got, want, (ctx, p))
            outs.append(got[0])
        return outs

    check(flt, base, "fresh")
    # rows removed after the filter was made drop out, on both routes: allowed = filter AND live
    live = np.ones(L.n, dtype=bool)
    for row in np.flatnonzero(base)[:25]:
        assert ix.remove(int(row))
        live[row] = False
    check(flt, base & live, "after removes")
    check(flt, base & live, "after removes, exact", route=va.ROUTE_EXACT)
    # rows inserted after enable_half_precision (and after the filter) are walked through but never returned
    L.grow(540)
    grown = np.concatenate([base & live, np.zeros(40, dtype=bool)])
    for out in check(flt, grown, "after inserts"):
        assert np.all(out[0][out[0] != fh.PAD_ID] < 500)
    # a negated filter: every row present at creation except the given ones, dead rows dropped at search time
    live = np.concatenate([live, np.ones(40, dtype=bool)])
    with ix.create_filter(np.flatnonzero(base).astype(np.uint64), negate=True) as neg:
        check(neg, ~np.concatenate([base, np.zeros(40, dtype=bool)]) & live, "negated")
    # the empty filter: out_n = 0, nothing runs; k = 0
    with ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        for p in fh.PRECISIONS:
            (ids, sc, cnt), routes = ix.search_batch_filtered_graph_half(qs, k, empty, MODE[p], ef=ef)
            assert np.all(cnt == 0) and np.all(routes == 0) and ix.last_kernels() == 0
            assert np.all(ids == fh.PAD_ID) and np.all(sc.view(np.uint32) == 0x7FC00000)
    for p in fh.PRECISIONS:
        (_, _, cnt), routes = ix.search_batch_with_filters_half(qs, 0, [flt, None] * (NQ // 2), MODE[p], ef=ef)
        assert np.all(cnt == 0) and np.all(routes == 0) and ix.last_kernels() == 0
    # refusals: the outputs keep their pattern
    f32_before = ix.search_batch_filtered_graph(qs, k, flt, ef=ef)
    for mode in (va.MODE_HNSW, va.MODE_BRUTE_F16, va.MODE_AUTO, va.MODE_HNSW_INT8):
        r = raw_call(ix, mode, [flt._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == UNSUPPORTED and untouched(r), mode
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h], [0] * NQ, qs, k, ef=ef, route=3)
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h, None], [0] * NQ, qs, k, ef=ef)  # a NULL table entry, used or not
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, va.MODE_HNSW_F16, [flt._h], [0] * (NQ - 1) + [2], qs, k, ef=ef)  # a query names a filter behind "no filter"
    assert r[0] == INVALID and untouched(r)
    other = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    other.insert_batch_parallel([(i, L.all_rows[i]) for i in range(64)], 16)
    other.enable_half_precision(VP.F16)
    with other.create_filter(np.arange(10, dtype=np.uint64)) as foreign:
        r = raw_call(ix, va.MODE_HNSW_F16, [flt._h, foreign._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == INVALID and untouched(r)
    other.close()
    ham = va.HnswIndex(L.dim, DM.Hamming, va.HnswParams(8, 60, 64))
    ham.insert_batch_parallel([(i, (L.all_rows[i] > 0).astype(np.float32)) for i in range(64)], 16)
    with ham.create_filter(np.arange(10, dtype=np.uint64)) as fham:
        for mode in (va.MODE_HNSW_F16, va.MODE_HNSW_BF16):
            r = raw_call(ham, mode, [fham._h], [0] * NQ, qs, k, ef=ef)
            assert r[0] == UNSUPPORTED and untouched(r)
    ham.close()
    group = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    group.insert_batch_parallel([(i, L.all_rows[i]) for i in range(64)], 16)
    group.enable_half_precision(VP.F16)
    r = raw_call(group, va.MODE_HNSW_F16, [], [0] * NQ, qs, k, ef=ef)
    assert r[0] == UNSUPPORTED and untouched(r)
    group.close()
    nograph = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    nograph.upload(np.arange(64), L.all_rows[:64])
    nograph.enable_half_precision(VP.F16)
    with nograph.create_filter(np.arange(10, dtype=np.uint64)) as f2:
        r = raw_call(nograph, va.MODE_HNSW_F16, [f2._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == STATE and untouched(r)
    nograph.close()
    # the handle is as usable as before, on both calls
    f32_after = ix.search_batch_filtered_graph(qs, k, flt, ef=ef)
    assert same_bits(f32_before[0], f32_after[0]) and np.array_equal(f32_before[1], f32_after[1])
    assert ix.last_kernels() == va.KERNEL_HNSW_FILTERED
    check(flt, grown, "after the refusals")
    # vacuum renumbers the rows: the filter is stale
    ix.vacuum()
    for p in fh.PRECISIONS:
        r = raw_call(ix, MODE[p], [flt._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == STATE and untouched(r)
    flt.close()
    ix.close()
