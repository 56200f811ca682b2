"""GPU tests of the filtered graph search over the u8 codes (vdb_hip_index_search_graph_filters_int8, csrc/hnsw_filtered.hip;
DESIGN 4.1l).

Reference: tests/filtered_int8_ref.py — tests/filtered_walk_ref.py over an oracle graph with the handle's links and the integer
distances between the oracle quantiser's codes, then the exact f32 re-score (tests/test_filtered_int8_ref_cpu.py holds it to
po.dual_search_int8).  Everything is compared bit for bit: ids, ranks, score bits, out_n, the ~0 / NaN padding, the per-query route
and the call's summed n_dist / n_expand.  Shapes: the smallest that reach every instance of the kernel family — the generic layout
with a tail code word, the register-chunk instances CPL 1 / 2 / 3 / 4, the generic layout just under the 1024-dimension limit — and a
constant dimension in one world.
"""
import ctypes as C

import numpy as np
import pytest

import filtered_int8_ref as fi
import filtered_walk_ref as fw
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
METRIC = {fi.COSINE: DM.Cosine, fi.EUCLIDEAN: DM.Euclidean, fi.DOT: DM.DotProduct}
NQ = fi.NQ
INVALID, UNSUPPORTED, STATE = -1, -7, -8
WALK_BITS = va.KERNEL_HNSW_FILTERED | va.KERNEL_HNSW_INT8
SHAPE_IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


class GpuWorld(fi.World):
    """a world with the GPU handle that loaded its dump and trained its quantiser, and the named filters as handles"""

    def __init__(self, root, metric, shape):
        super().__init__(root, metric, shape, const_dim=shape == fi.CONST_DIM_SHAPE)
        n, dim, M, efc = shape
        self.ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
        self.ix.load_reference_files(self.dir, fi.BASE)
        self.ix.train_quantizer()  # the first min(1000, n) rows, as DualPrecisionHnsw
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
    root, cache = str(tmp_path_factory.mktemp("filters_graph_int8")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = GpuWorld(root, metric, shape)
        return cache[(metric, shape)]
    yield get
    for w in cache.values():
        w.close()


def batch(ix, qs, k, filters, ef, ratio=0, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_with_filters_int8(qs, k, filters, ef=ef, oversampling=ratio, route=route, max_list=max_list)
    return out, routes, ix.last_search_stats(), ix.last_kernels()


def one(ix, qs, k, flt, ef, ratio=0, route=va.ROUTE_AUTO, max_list=0):
    out, routes = ix.search_batch_filtered_graph_int8(qs, k, flt, ef=ef, oversampling=ratio, route=route, max_list=max_list)
    return out, routes, ix.last_search_stats()


def same_bits(a, b):
    (ai, asc, ac), (bi, bsc, bc) = a, b
    return np.array_equal(ai, bi) and np.array_equal(asc.view(np.uint32), bsc.view(np.uint32)) and np.array_equal(ac, bc)


# ---- 1. no query filtered: the call IS search_batch(MODE_HNSW_INT8), and so the oracle's dual-precision search --------------------------
@pytest.mark.parametrize("shape", fi.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fi.METRICS)
def test_no_filter_is_the_plain_int8_walk(worlds, metric, shape):
    w = worlds(metric, shape)
    for k, ef in fi.KEF:
        pid, psc, pcnt = w.ix._search_raw(w.qs, k, ef, va.MODE_HNSW_INT8)
        pstats = w.ix.last_search_stats()
        assert w.ix.last_kernels() & va.KERNEL_HNSW_INT8
        nd = ne = 0
        for qi, q in enumerate(w.qs):
            oid, od, a, b = po.dual_search_int8(w.g, w.sq, w.codes, q, k, ef, 4, po.TIE_CANONICAL)
            nd, ne = nd + a, ne + b
            assert int(pcnt[qi]) == len(oid) and pid[qi, :len(oid)].tolist() == oid.tolist(), (k, ef, qi)
            assert np.array_equal(psc[qi, :len(oid)].view(np.uint32), fw.score_bits(w.G.metric, od)), (k, ef, qi)
        assert tuple(pstats) == (nd, ne)
        for filters, ratio in (([None] * NQ, 0), ([w.flt("all")] * NQ, 4), ([None if i % 2 else w.flt("all") for i in range(NQ)], 0)):
            (ids, sc, cnt), routes, stats, kern = batch(w.ix, w.qs, k, filters, ef, ratio)
            assert kern == WALK_BITS, hex(kern)
            assert np.all(routes == 1)
            assert np.array_equal(cnt, pcnt) and tuple(stats) == tuple(pstats), (k, ef, stats, pstats)
            # (whole blocks: the padding of both calls is id 2^64 - 1 / the canonical NaN)
            assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)), (k, ef)


# ---- 2. random and clustered filters against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half", "tenth", "clustered"])
@pytest.mark.parametrize("shape", fi.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fi.METRICS)
def test_filtered_int8_walk_equals_the_reference(worlds, metric, shape, name):
    w, k, ef, ratio = worlds(metric, shape), 10, 64, 4
    allowed = w.filters[name]
    want = fi.expect_call(w.G, w.qs, allowed, k, ef, ratio, va.ROUTE_WALK)
    assert want[2] == [1] * NQ, "the reference itself overflows at this shape"
    got = one(w.ix, w.qs, k, w.flt(name), ef, ratio, route=va.ROUTE_WALK)
    assert w.ix.last_kernels() == WALK_BITS, hex(w.ix.last_kernels())
    fi.assert_call(got, want, (metric, shape, name))
    assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])
    assert np.all(got[0][2] == k)


@pytest.mark.parametrize("ratio", [1, 4, 7])
@pytest.mark.parametrize("name", ["half", "tenth"])
@pytest.mark.parametrize("metric", fi.METRICS)
def test_ratios_and_the_balanced_ef(worlds, metric, name, ratio):
    """ef = 0 (Balanced: max(128, 4k)) under three ratios — ef_w = 128 at ratios 1 and 4, 25 * 7 = 175 at ratio 7 — in the world with
    the constant dimension; the handle's own option serves ratio 0"""
    w, k = worlds(metric, fi.CONST_DIM_SHAPE), 25
    want = fi.expect_call(w.G, w.qs, w.filters[name], k, 0, ratio, va.ROUTE_WALK)
    assert want[2] == [1] * NQ
    got = one(w.ix, w.qs, k, w.flt(name), 0, ratio, route=va.ROUTE_WALK)
    fi.assert_call(got, want, (metric, name, ratio))
    if ratio == 7:
        w.ix.set_option(va.OPT_INT8_OVERSAMPLING, 7)
        try:
            fi.assert_call(one(w.ix, w.qs, k, w.flt(name), 0, 0, route=va.ROUTE_WALK), want, (metric, name, "option 7"))
        finally:
            w.ix.set_option(va.OPT_INT8_OVERSAMPLING, 4)


@pytest.mark.parametrize("metric", fi.METRICS)
def test_k_larger_than_the_allowed_rows(worlds, metric):
    """40 allowed rows, k = 50: the walk never has a pivot, its list takes every node the links reach, and the allowed ones among
    them come back re-scored; on the auto route the exact pass answers with all 40"""
    w, k, ratio = worlds(metric, fi.CONST_DIM_SHAPE), 50, 1
    few = w.filters["few"]
    want = fi.expect_call(w.G, w.qs, few, k, 0, ratio, va.ROUTE_WALK)
    assert want[2] == [1] * NQ and all(30 <= len(i) <= 40 for i in want[0])
    got = one(w.ix, w.qs, k, w.flt("few"), 0, ratio, route=va.ROUTE_WALK)
    fi.assert_call(got, want, (metric, "walk"))
    got_a = one(w.ix, w.qs, k, w.flt("few"), 0, ratio)
    assert w.ix.last_kernels() == va.KERNEL_FILTER_RANK
    fi.assert_call(got_a, fi.expect_call(w.G, w.qs, few, k, 0, ratio, va.ROUTE_AUTO), (metric, "auto"))
    assert np.all(got_a[0][2] == 40)
    for qi in range(NQ):  # every row the walk returned is among the exact pass's 40, with the same score bits, in the same order
        c = int(got[0][2][qi])
        b = dict(zip(got_a[0][0][qi, :40].tolist(), got_a[0][1][qi, :40].view(np.uint32).tolist()))
        assert [b[i] for i in got[0][0][qi, :c].tolist()] == got[0][1][qi, :c].view(np.uint32).tolist(), qi


# ---- 3. routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fi.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fi.METRICS)
def test_routes_and_the_f32_exact_pass(worlds, metric, shape):
    w, k, ef = worlds(metric, shape), 10, 64
    few = w.filters["few"]
    assert int(few.sum()) == 40 < ef
    # auto: the walk could never fill its result set -> the exact pass for every query; it is the f32 call's, bit for bit
    got = one(w.ix, w.qs, k, w.flt("few"), ef)
    assert w.ix.last_kernels() == va.KERNEL_FILTER_RANK, hex(w.ix.last_kernels())
    f32 = w.ix.search_batch_filtered_graph(w.qs, k, w.flt("few"), ef=ef, route=va.ROUTE_EXACT)
    f32_stats = w.ix.last_search_stats()
    assert same_bits(got[0], f32[0]) and np.array_equal(got[1], f32[1]) and tuple(got[2]) == tuple(f32_stats) == (NQ * 40, 0)
    fi.assert_call(got, fi.expect_call(w.G, w.qs, few, k, ef, 4, va.ROUTE_AUTO), "auto, few")
    # the exact pass on demand, and the walk: a row has the same score bits on either route
    got_e = one(w.ix, w.qs, k, w.flt("half"), ef, route=va.ROUTE_EXACT)
    assert w.ix.last_kernels() == va.KERNEL_FILTER_RANK
    f32 = w.ix.search_batch_filtered_graph(w.qs, k, w.flt("half"), ef=ef, route=va.ROUTE_EXACT)
    assert same_bits(got_e[0], f32[0]) and np.array_equal(got_e[1], f32[1]) and tuple(got_e[2]) == tuple(w.ix.last_search_stats())
    fi.assert_call(got_e, fi.expect_call(w.G, w.qs, w.filters["half"], k, ef, 4, va.ROUTE_EXACT), "exact, half")
    got_w = one(w.ix, w.qs, k, w.flt("half"), ef, route=va.ROUTE_WALK)
    common = 0
    for qi in range(NQ):
        ce, cw = int(got_e[0][2][qi]), int(got_w[0][2][qi])
        exact = dict(zip(got_e[0][0][qi, :ce].tolist(), got_e[0][1][qi, :ce].view(np.uint32).tolist()))
        for i, s in zip(got_w[0][0][qi, :cw].tolist(), got_w[0][1][qi, :cw].view(np.uint32).tolist()):
            if i in exact:
                common += 1
                assert exact[i] == s, (qi, i)
    assert common > NQ * k // 2


def raw_call(ix, handles, fq, qs, k, ef=64, ratio=0, route=0, max_list=0):
    """the entry point with a hand-made table -> (status, ids, scores, counts, routes); the outputs start as a known pattern"""
    from velesdb_amd import _ffi
    nq = qs.shape[0]
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    ids, sc = np.full((nq, max(k, 1)), 7, dtype=np.uint64), np.full((nq, max(k, 1)), 7.0, dtype=np.float32)
    cnt, routes = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint32)
    fq = np.asarray(fq, dtype=np.uint32)
    table = (C.c_void_p * max(len(handles), 1))(*handles)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().vdb_hip_index_search_graph_filters_int8(ix._h, table if handles else None, len(handles), p(fq), p(qs), nq, k, ef, ratio,
                                                            route, max_list, p(ids), p(sc), p(cnt), p(routes))
    return rc, ids, sc, cnt, routes


def untouched(r):
    return np.all(r[1] == 7) and np.all(r[2] == 7.0) and np.all(r[3] == 7) and np.all(r[4] == 7)


@pytest.mark.parametrize("metric", fi.METRICS)
def test_queries_that_overflow_the_largest_list_take_the_exact_pass_alone(worlds, metric):
    """fi.overflow_case: max_list is chosen from the peaks of the reference's own lists so that some but not all queries overflow it"""
    w, k, ef, ratio = worlds(metric, fi.SHAPES[0]), 10, 16, 1
    allowed, qs, chosen, over = fi.overflow_case(w, k, ef, ratio)
    assert chosen is not None, "no list size splits the queries: the case is meaningless"
    want = fi.expect_call(w.G, qs, allowed, k, ef, ratio, va.ROUTE_AUTO, max_list=chosen)
    assert want[2] == [2 if o else 1 for o in over]
    print(f"metric {metric}: max_list {chosen}, routes {want[2]}")
    with w.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as flt:
        got = one(w.ix, qs, k, flt, ef, ratio, max_list=chosen)
        assert w.ix.last_kernels() == WALK_BITS | va.KERNEL_FILTER_RANK
        fi.assert_call(got, want, ("fallback", chosen))
        # route 1: the queries that overflow the largest list fail the whole call, and nothing is written
        with pytest.raises(va.VelesHipError) as e:
            w.ix.search_batch_filtered_graph_int8(qs, k, flt, ef=ef, oversampling=ratio, route=va.ROUTE_WALK, max_list=chosen)
        assert e.value.code == UNSUPPORTED and f"{sum(over)} queries overflow" in str(e.value), str(e.value)
        r = raw_call(w.ix, [flt._h], [0] * NQ, qs, k, ef=ef, ratio=ratio, route=va.ROUTE_WALK, max_list=chosen)
        assert r[0] == UNSUPPORTED and untouched(r)


# ---- 4. the per-query contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [fi.SHAPES[0], fi.SHAPES[3]], ids=SHAPE_IDS)
@pytest.mark.parametrize("metric", fi.METRICS)
def test_mixed_batch_equals_the_one_query_calls(worlds, metric, shape):
    w, k, ef = worlds(metric, shape), 10, 64
    with w.ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        for order in (list(range(NQ)), list(reversed(range(NQ)))):
            kinds = [("half", "tenth", "few", None, "empty")[i % 5] for i in order]
            filters = [empty if n == "empty" else w.flt(n) for n in kinds]
            qs = w.qs[order]
            (ids, sc, cnt), routes, stats, kern = batch(w.ix, qs, k, filters, ef)
            assert kern == WALK_BITS | va.KERNEL_FILTER_RANK, hex(kern)
            nd = ne = 0
            for qi in range(NQ):
                (i1, s1, c1), r1, st1, k1 = batch(w.ix, qs[qi:qi + 1], k, [filters[qi]], ef)
                nd, ne = nd + st1[0], ne + st1[1]
                assert int(routes[qi]) == int(r1[0]) == {"few": 2, "empty": 0}.get(kinds[qi], 1), (qi, kinds[qi])
                assert np.array_equal(ids[qi], i1[0]) and np.array_equal(sc[qi].view(np.uint32), s1[0].view(np.uint32)), (qi, kinds[qi])
                assert cnt[qi] == c1[0], (qi, kinds[qi])
                if kinds[qi] == "empty":
                    assert cnt[qi] == 0 and k1 == 0 and np.all(ids[qi] == fi.PAD_ID) and np.all(sc[qi].view(np.uint32) == 0x7FC00000)
            assert tuple(stats) == (nd, ne)


# ---- 5. integers beyond 2^24, and ties ------------------------------------------------------------------------------------------------
def test_integer_distances_beyond_2_pow_24_and_ties(tmp_path):
    """fi.BigWorld (tests/test_filtered_int8_ref_cpu.py shows that a walk which converts its integers by value answers differently
    there): the kernel is held to the exact-integer reference, at the ratio where the coarse order decides the ids and at 4"""
    w = fi.BigWorld(str(tmp_path))
    n, dim, M, efc = w.shape
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, n))
    ix.load_reference_files(w.dir, fi.BASE)
    ix.train_quantizer()
    with ix.create_filter(np.flatnonzero(w.allowed).astype(np.uint64)) as flt:
        for ratio in (fi.BIG_RATIO, 4):
            want = fi.expect_call(w.G, w.qs, w.allowed, fi.BIG_K, fi.BIG_EF, ratio, va.ROUTE_WALK)
            assert want[2] == [1] * NQ
            got = one(ix, w.qs, fi.BIG_K, flt, fi.BIG_EF, ratio, route=va.ROUTE_WALK)
            fi.assert_call(got, want, ("big", ratio))
    ix.close()


# ---- 6. life cycle and refusals ----------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(va.VelesHipError) as e:
        fn()
    return e.value.code


def test_life_cycle_and_refusals(tmp_path):
    """a graph built row by row on both sides (the GPU's sequential insert == the oracle's, link for link)"""
    rng = np.random.default_rng(21)
    dim, k, ef, ratio = 32, 10, 32, 4
    all_rows = rng.standard_normal((604, dim)).astype(np.float32)
    qs = rng.standard_normal((NQ, dim)).astype(np.float32)
    g = po.NativeHnsw(dim, po.EUCLIDEAN, 8, 60, po.MODE_C)
    g.set_build_tie(po.TIE_CANONICAL)
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 604))

    def grow(frm, to):
        for i in range(frm, to):
            g.insert(all_rows[i])
            ix.insert(i, all_rows[i])

    grow(0, 500)
    base = fw.random_filter(np.random.default_rng(22), 500, 0.3)
    flt = ix.create_filter(np.flatnonzero(base).astype(np.uint64))
    # an untrained handle: VDB_ERR_STATE, as mode 4
    assert code_of(lambda: ix.search_batch_filtered_graph_int8(qs, k, flt, ef=ef)) == STATE
    r = raw_call(ix, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    ix.train_quantizer()
    sq = po.ScalarQuantizer(all_rows[:500])

    def ref(n):
        return fi.CodeGraph(g, all_rows[:n], po.EUCLIDEAN, sq, sq.quantize(all_rows[:n]))

    def check(G, f, allowed, ctx, route=va.ROUTE_WALK, queries=qs):
        got = one(ix, queries, k, f, ef, ratio, route=route)
        assert ix.last_kernels() == (va.KERNEL_FILTER_RANK if route == va.ROUTE_EXACT else WALK_BITS), (ctx, hex(ix.last_kernels()))
        want = fi.expect_call(G, queries, allowed, k, ef, ratio, route, matched=f.matched)
        assert 2 not in want[2] or route == va.ROUTE_EXACT
        fi.assert_call(got, want, ctx)
        return got[0]

    G = ref(500)
    check(G, flt, base, "fresh")
    # rows removed after the filter was made drop out, on both routes: allowed = filter AND live
    live = np.ones(500, dtype=bool)
    for row in np.flatnonzero(base)[:25]:
        assert ix.remove(int(row))
        live[row] = False
    check(G, flt, base & live, "after removes")
    check(G, flt, base & live, "after removes, exact", route=va.ROUTE_EXACT)
    # rows inserted after training are encoded with the trained quantiser and walked through, but are not in the older filter ...
    grow(500, 540)
    G = ref(540)
    grown = np.concatenate([base & live, np.zeros(40, dtype=bool)])
    out = check(G, flt, grown, "after inserts")
    assert np.all(out[0][out[0] != fi.PAD_ID] < 500)
    # ... and are reachable: a filter made now holds them, and queries at those rows find them
    live = np.concatenate([live, np.ones(40, dtype=bool)])
    newer = np.concatenate([base, np.ones(40, dtype=bool)])
    with ix.create_filter(np.flatnonzero(newer).astype(np.uint64)) as f2:
        out = check(G, f2, newer & live, "a filter made after the inserts", queries=all_rows[500:500 + NQ])
        assert int((out[0][:, 0] == np.arange(500, 500 + NQ)).sum()) >= NQ // 2  # (a greedy walk may miss one: the reference decides)
    # the empty filter: out_n = 0, nothing runs; k = 0
    with ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        (ids, sc, cnt), routes = ix.search_batch_filtered_graph_int8(qs, k, empty, ef=ef)
        assert np.all(cnt == 0) and np.all(routes == 0) and ix.last_kernels() == 0
        assert np.all(ids == fi.PAD_ID) and np.all(sc.view(np.uint32) == 0x7FC00000)
    (_, _, cnt), routes = ix.search_batch_with_filters_int8(qs, 0, [flt, None] * (NQ // 2), ef=ef)
    assert np.all(cnt == 0) and np.all(routes == 0) and ix.last_kernels() == 0
    # refusals: the outputs keep their pattern
    before = one(ix, qs, k, flt, ef, ratio)
    r = raw_call(ix, [flt._h], [0] * NQ, qs, k, ef=ef, ratio=65)
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, [flt._h], [0] * NQ, qs, k, ef=ef, route=3)
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, [flt._h, None], [0] * NQ, qs, k, ef=ef)  # a NULL table entry, used or not
    assert r[0] == INVALID and untouched(r)
    r = raw_call(ix, [flt._h], [0] * (NQ - 1) + [2], qs, k, ef=ef)  # a query names a filter behind "no filter"
    assert r[0] == INVALID and untouched(r)
    other = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    other.insert_batch_parallel([(i, all_rows[i]) for i in range(64)], 16)
    other.train_quantizer()
    with other.create_filter(np.arange(10, dtype=np.uint64)) as foreign:
        r = raw_call(ix, [flt._h, foreign._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == INVALID and untouched(r)
    other.close()
    ham = va.HnswIndex(dim, DM.Hamming, va.HnswParams(8, 60, 64))
    ham.insert_batch_parallel([(i, (all_rows[i] > 0).astype(np.float32)) for i in range(64)], 16)
    with ham.create_filter(np.arange(10, dtype=np.uint64)) as fham:
        r = raw_call(ham, [fham._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == UNSUPPORTED and untouched(r)
    ham.close()
    group = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    group.insert_batch_parallel([(i, all_rows[i]) for i in range(64)], 16)
    r = raw_call(group, [], [0] * NQ, qs, k, ef=ef)
    assert r[0] == UNSUPPORTED and untouched(r)
    group.close()
    nograph = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    nograph.upload(np.arange(64), all_rows[:64])
    nograph.train_quantizer()
    with nograph.create_filter(np.arange(10, dtype=np.uint64)) as f3:
        r = raw_call(nograph, [f3._h], [0] * NQ, qs, k, ef=ef)
        assert r[0] == STATE and untouched(r)
    nograph.close()
    # the three existing filtered calls keep refusing mode 4
    assert code_of(lambda: ix.search_batch_brute_force_filtered(qs, k, flt, mode=va.MODE_HNSW_INT8)) == UNSUPPORTED
    assert code_of(lambda: ix.search_batch_filtered_graph(qs, k, flt, ef=ef, mode=va.MODE_HNSW_INT8)) == UNSUPPORTED
    from velesdb_amd import _ffi
    o_ids, o_sc = np.full((NQ, k), 7, dtype=np.uint64), np.full((NQ, k), 7.0, dtype=np.float32)
    o_cnt, o_rt, fq = np.full(NQ, 7, dtype=np.uint32), np.full(NQ, 7, dtype=np.uint32), np.zeros(NQ, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().vdb_hip_index_search_graph_filters(ix._h, (C.c_void_p * 1)(flt._h), 1, p(fq), p(np.ascontiguousarray(qs)), NQ, k, ef,
                                                       va.MODE_HNSW_INT8, 0, 0, p(o_ids), p(o_sc), p(o_cnt), p(o_rt))
    assert rc == UNSUPPORTED and untouched((rc, o_ids, o_sc, o_cnt, o_rt))
    # the handle is as usable as before
    after = one(ix, qs, k, flt, ef, ratio)
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1]) and tuple(before[2]) == tuple(after[2])
    # vacuum renumbers the rows: the filter is stale
    ix.vacuum()
    r = raw_call(ix, [flt._h], [0] * NQ, qs, k, ef=ef)
    assert r[0] == STATE and untouched(r)
    flt.close()
    ix.close()
