"""GPU tests of the filtered graph search (vdb_hip_index_search_graph_filtered, csrc/hnsw_filtered.hip).

The reference is tests/filtered_walk_ref.py (validated on the CPU by tests/test_filtered_walk_ref_cpu.py): the reference's
search_layer with `results` receiving allowed nodes only, in the kernel's single-list form at the capacity the host chose, and
the exact pass as a plain sort.  Everything is compared bit for bit — ids, ranks, score bits, out_n, the per-query route and the
call's n_dist / n_expand; there are no tolerances.  Shapes are those of tests/half_walk_ref.py (CPL 0, CPL 3, dim % 4 != 0), one
oracle graph and one GPU handle per (metric, shape); the handle loads the oracle's dump, so both sides walk the same links.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import filtered_walk_ref as fw
import half_walk_ref as hw
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
METRIC = {po.COSINE: DM.Cosine, po.EUCLIDEAN: DM.Euclidean, po.DOT: DM.DotProduct, po.HAMMING: DM.Hamming, po.JACCARD: DM.Jaccard}
F32_METRICS = [po.COSINE, po.EUCLIDEAN, po.DOT]
BASE = "native_hnsw"
NQ = hw.NQ
INVALID, UNSUPPORTED, STATE = -1, -7, -8


class World:
    """rows, queries, the oracle graph (canonical build ties), its dump and — on first use — the GPU handle that loaded the dump"""

    def __init__(self, root, metric, shape):
        n, dim, M, efc = shape
        self.metric, self.shape, self.n, self.dim = metric, shape, n, dim
        rng = np.random.default_rng(7000 + 100 * metric + n + dim)
        self.rows = rng.standard_normal((n, dim)).astype(np.float32)
        self.qs = rng.standard_normal((NQ, dim)).astype(np.float32)
        if metric in (po.HAMMING, po.JACCARD):  # sign-bit data: the packed-bit metrics read bit = (x > 0.5)
            self.rows, self.qs = (self.rows > 0).astype(np.float32), (self.qs > 0).astype(np.float32)
        g = po.NativeHnsw(dim, metric, M, efc, po.MODE_C)
        g.set_build_tie(po.TIE_CANONICAL)
        for v in self.rows:
            g.insert(v)
        self.g, self.G = g, fw.Graph(g, self.rows, metric)
        self.dir = os.path.join(root, f"m{metric}_{n}_{dim}")
        os.makedirs(self.dir)
        g.file_dump(self.dir, BASE)
        frng = np.random.default_rng(n + dim)
        self.filters = {"all": np.ones(n, dtype=bool), "half": fw.random_filter(frng, n, 0.5), "tenth": fw.random_filter(frng, n, 0.1),
                        "clustered": self.rows[:, 0] > (0.5 if metric in (po.HAMMING, po.JACCARD) else 0.0),
                        "few": fw.random_filter(frng, n, 40 / n)}
        self._ix, self._flt = None, {}

    @property
    def ix(self):
        if self._ix is None:
            n, dim, M, efc = self.shape
            self._ix = va.HnswIndex(dim, METRIC[self.metric], va.HnswParams(M, efc, n))
            self._ix.load_reference_files(self.dir, BASE)
        return self._ix

    def flt(self, name):  # (created after the load: a load renumbers the rows)
        if name not in self._flt:
            self._flt[name] = self.ix.create_filter(np.flatnonzero(self.filters[name]).astype(np.uint64))
            assert self._flt[name].matched == int(self.filters[name].sum())
        return self._flt[name]

    def close(self):
        for f in self._flt.values():
            f.close()
        if self._ix is not None:
            self._ix.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("filtered_graph")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = World(root, metric, shape)
        return cache[(metric, shape)]
    yield get
    for w in cache.values():
        w.close()


def protocol(G, q, k, ef_eff, allowed, first, cap_max):
    """what the host does with one query on the walk / auto route: the walk at `first`, four times the room while it overflows, up
    to cap_max.  -> (form (b) result of the last attempt, overflowed at cap_max)"""
    cap = first
    while True:
        r = fw.walk_single_list(G, q, k, ef_eff, allowed, cap)
        if not r[4] or cap >= cap_max:
            return r, r[4]
        cap = min(4 * cap, cap_max)


def expect_call(w, allowed, k, ef, route, max_list=0, matched=None, qs=None):
    """the whole call by the reference -> (ids, score bits, routes, (n_dist, n_expand)); asserts nothing.  allowed = filter AND
    live; matched = the rows in the filter (what sizes the list), when that differs.  Without max_list the largest list is taken as
    unbounded: the callers assert that no query overflows."""
    G, ef_eff = w.G, fw.ef_rule(k, ef)
    matched = int(allowed.sum()) if matched is None else matched
    ids, sbits, routes, nd, ne = [], [], [], 0, 0
    cap_max = max_list if max_list else 1 << 30
    sized = fw.sized_list(ef_eff, matched, w.n) if matched else None
    whole_exact = route == va.ROUTE_EXACT or (route == va.ROUTE_AUTO and (matched < ef_eff or sized > cap_max))
    for q in (w.qs if qs is None else qs):
        over = True
        if not whole_exact:
            r, over = protocol(G, q, k, ef_eff, allowed, min(sized, cap_max), cap_max)
            nd, ne = nd + r[2], ne + r[3]
        if over:
            e = fw.exact_pass(G, q, k, allowed)
            r, nd = (e[0], e[1]), nd + e[2]
        ids.append(list(r[0]))
        sbits.append(fw.score_bits(w.metric, r[1]))
        routes.append(2 if over else 1)
    return ids, sbits, routes, (nd, ne)


def assert_call(got, want, ctx):
    (ids, sc, cnt), routes, stats = got
    wi, wb, wr, ws = want
    assert routes.tolist() == wr, ctx
    for qi in range(len(wi)):
        c = int(cnt[qi])
        assert c == len(wi[qi]) and ids[qi, :c].tolist() == wi[qi], (ctx, qi)
        assert np.array_equal(sc[qi, :c].view(np.uint32), wb[qi]), (ctx, qi)
        assert np.all(ids[qi, c:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isnan(sc[qi, c:])), (ctx, qi)
    assert stats == ws, ctx


def run(w, name, k, ef, route, max_list=0):
    out, routes = w.ix.search_batch_filtered_graph(w.qs, k, w.flt(name), ef=ef, route=route, max_list=max_list)
    return out, routes, w.ix.last_search_stats()


# ---- 1. a filter that allows every row: the call IS VDB_SEARCH_HNSW --------------------------------------------------------------
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", F32_METRICS)
def test_all_allowed_filter_is_the_unfiltered_walk(worlds, metric, shape):
    w = worlds(metric, shape)
    for k, ef in hw.KEF:
        (ids, sc, cnt), routes, stats = run(w, "all", k, ef, va.ROUTE_WALK)
        kern = w.ix.last_kernels()
        assert kern & va.KERNEL_HNSW_FILTERED and not kern & (va.KERNEL_HNSW | va.KERNEL_FILTER_RANK), hex(kern)
        assert np.all(routes == 1)
        pid, psc, pcnt = w.ix._search_raw(w.qs, k, ef, va.MODE_HNSW)
        pstats = w.ix.last_search_stats()
        assert w.ix.last_kernels() & va.KERNEL_HNSW
        assert np.array_equal(cnt, pcnt) and stats == pstats, (k, ef, stats, pstats)
        oid, obits, ostats = hw.oracle_walk(w.g, metric, w.qs, k, ef)
        assert stats == ostats, (k, ef)
        for qi in range(NQ):
            c = int(cnt[qi])
            assert ids[qi, :c].tolist() == pid[qi, :c].tolist() == oid[qi], (k, ef, qi)
            assert np.array_equal(sc[qi, :c].view(np.uint32), psc[qi, :c].view(np.uint32)), (k, ef, qi)
            assert np.array_equal(sc[qi, :c].view(np.uint32), obits[qi]), (k, ef, qi)


@pytest.mark.parametrize("metric", [po.HAMMING, po.JACCARD])
def test_all_allowed_filter_bit_metrics(worlds, metric):
    w = worlds(metric, hw.SHAPES[0])
    for k, ef in [(10, 64), (10, 300)]:
        got = run(w, "all", k, ef, va.ROUTE_WALK)
        assert w.ix.last_kernels() & va.KERNEL_HNSW_FILTERED and not w.ix.last_kernels() & va.KERNEL_HNSW
        pid, psc, pcnt = w.ix._search_raw(w.qs, k, ef, va.MODE_HNSW)
        assert got[2] == w.ix.last_search_stats()
        (ids, sc, cnt), _, _ = got
        assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)) and np.array_equal(cnt, pcnt)
        assert_call(got, expect_call(w, w.filters["all"], k, ef, va.ROUTE_WALK), (metric, k, ef))  # exact distance ties: canonical order


# ---- 2. random and clustered filters, the walk route ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half", "tenth", "clustered"])
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", F32_METRICS)
def test_filtered_walk_equals_the_single_list_reference(worlds, metric, shape, name):
    w, k, ef = worlds(metric, shape), 10, 64
    allowed = w.filters[name]
    want = expect_call(w, allowed, k, ef, va.ROUTE_WALK)
    assert want[2] == [1] * NQ, "the reference itself overflows at this shape"
    got = run(w, name, k, ef, va.ROUTE_WALK)
    kern = w.ix.last_kernels()
    assert kern & va.KERNEL_HNSW_FILTERED and not kern & (va.KERNEL_HNSW | va.KERNEL_FILTER_RANK), hex(kern)
    assert_call(got, want, (metric, shape, name))
    assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])


@pytest.mark.parametrize("metric", F32_METRICS)
def test_selective_filter_returns_k_where_over_fetching_comes_back_short(worlds, metric):
    w, k = worlds(metric, hw.SHAPES[0]), 10
    allowed = w.filters["tenth"]
    short_ref = sum(len(fw.over_fetch(w.g, q, k, allowed)[0]) < k for q in w.qs)
    assert short_ref > NQ // 2, "the case is meaningless: the reference's over-fetch rule already returns k"
    (ids, sc, cnt), routes, _ = run(w, "tenth", k, 0, va.ROUTE_WALK)
    assert np.all(cnt == k) and np.all(routes == 1)
    kk = max(4 * k, k + 10)
    pid, _, pcnt = w.ix._search_raw(w.qs, kk, 0, va.MODE_HNSW)
    short = sum(sum(bool(allowed[int(i)]) for i in pid[qi, :int(pcnt[qi])]) < k for qi in range(NQ))
    assert short == short_ref and short > NQ // 2


# ---- 3. routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", F32_METRICS)
def test_routes(worlds, metric, shape):
    w, k, ef = worlds(metric, shape), 10, 64
    few = w.filters["few"]
    assert int(few.sum()) < ef
    # auto: the walk could never fill its result set -> the exact pass for every query
    got = run(w, "few", k, ef, va.ROUTE_AUTO)
    kern = w.ix.last_kernels()
    assert kern & va.KERNEL_FILTER_RANK and not kern & (va.KERNEL_HNSW_FILTERED | va.KERNEL_HNSW), hex(kern)
    want = expect_call(w, few, k, ef, va.ROUTE_AUTO)
    assert want[2] == [2] * NQ and want[3] == (NQ * int(few.sum()), 0)
    assert_call(got, want, "auto, few")
    # walk: on these small graphs the list holds the component, the walk completes
    got_w = run(w, "few", k, ef, va.ROUTE_WALK)
    want_w = expect_call(w, few, k, ef, va.ROUTE_WALK)
    assert want_w[2] == [1] * NQ
    assert_call(got_w, want_w, "walk, few")
    # where the walk reached every allowed row its answer is the exact one — same ids, same score bits: one distance function
    reached = 0
    for qi in range(NQ):
        c, cw = int(got[0][2][qi]), int(got_w[0][2][qi])
        if set(got_w[0][0][qi, :cw].tolist()) == set(got[0][0][qi, :c].tolist()):
            reached += 1
            assert got_w[0][0][qi, :cw].tolist() == got[0][0][qi, :c].tolist()
            assert np.array_equal(got_w[0][1][qi, :cw].view(np.uint32), got[0][1][qi, :c].view(np.uint32))
    assert reached > 0
    # exact pass on demand
    got_e = run(w, "half", k, ef, va.ROUTE_EXACT)
    assert w.ix.last_kernels() & va.KERNEL_FILTER_RANK and not w.ix.last_kernels() & va.KERNEL_HNSW_FILTERED
    assert_call(got_e, expect_call(w, w.filters["half"], k, ef, va.ROUTE_EXACT), "exact, half")


# ---- 4. per-query fallback -----------------------------------------------------------------------------------------------------------
def overflow_case(w):
    """Density 1/10, all of it at one end of the data: the 10 % of the rows with the largest first coordinate, and queries pushed
    along that coordinate by +30 ... -30 — towards the allowed rows a query fills its results at once, away from them it admits
    most of the graph first.  max_list is chosen with the reference so that some but not all of the 20 queries overflow it.
    -> (allowed, qs, k, ef, max_list, the reference's call); computed once per world"""
    if getattr(w, "_overflow_case", None) is None:
        k, ef = 10, 16
        allowed = np.zeros(w.n, dtype=bool)
        allowed[np.argsort(w.rows[:, 0])[-w.n // 10:]] = True
        qs = w.qs.copy()
        qs[:, 0] += np.resize(np.array([30, -30, 0, -4, -8, -2], dtype=np.float32), NQ)
        ef_eff, matched = fw.ef_rule(k, ef), int(allowed.sum())
        sized = fw.sized_list(ef_eff, matched, w.n)
        chosen = None
        for max_list in (4 * sized, 2 * sized, sized):  # (below `sized` the auto rule sends the whole call to the exact pass)
            over = [protocol(w.G, q, k, ef_eff, allowed, sized, max_list)[1] for q in qs]
            if 0 < sum(over) < NQ:
                chosen = max_list
                break
        assert chosen is not None, "no list size splits the queries: the case is meaningless"
        want = expect_call(w, allowed, k, ef, va.ROUTE_AUTO, max_list=chosen, qs=qs)
        assert 1 in want[2] and 2 in want[2]
        print(f"metric {w.metric}: max_list {chosen} (first list {sized}), routes {want[2]}")
        w._overflow_case = (allowed, qs, k, ef, chosen, want)
    return w._overflow_case


@pytest.mark.parametrize("metric", F32_METRICS)
def test_queries_that_overflow_the_largest_list_take_the_exact_pass_alone(worlds, metric):
    """overflow_case: some queries of the call answer from the walk, the others overflow the largest list and take the exact pass"""
    w = worlds(metric, hw.SHAPES[0])
    allowed, qs, k, ef, chosen, want = overflow_case(w)
    with w.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as flt:
        out, routes = w.ix.search_batch_filtered_graph(qs, k, flt, ef=ef, route=va.ROUTE_AUTO, max_list=chosen)
        stats, kern = w.ix.last_search_stats(), w.ix.last_kernels()
        assert kern & va.KERNEL_HNSW_FILTERED and kern & va.KERNEL_FILTER_RANK, hex(kern)
        assert_call((out, routes, stats), want, ("fallback", chosen))
        # a query's answer does not depend on its companions: alone it takes the same route and gives the same bits
        for qi in (want[2].index(1), want[2].index(2)):
            o1, r1 = w.ix.search_batch_filtered_graph(qs[qi:qi + 1], k, flt, ef=ef, route=va.ROUTE_AUTO, max_list=chosen)
            assert r1[0] == want[2][qi] and np.array_equal(o1[0][0], out[0][qi]), qi
            assert np.array_equal(o1[1][0].view(np.uint32), out[1][qi].view(np.uint32)) and o1[2][0] == out[2][qi], qi
        with pytest.raises(va.VelesHipError) as e:
            w.ix.search_batch_filtered_graph(qs, k, flt, ef=ef, route=va.ROUTE_WALK, max_list=chosen)
        assert e.value.code == UNSUPPORTED and "route" in str(e.value) and "max_list" in str(e.value)


def test_call_without_out_route_gives_the_same_answer(worlds):
    """out_route is nullable at the C level; multi-query fusion is the only caller inside the library that leaves it out.  The same
    one-filter call with and without it — walks, re-runs and exact passes in one call (overflow_case) — gives the same ids, score
    bits and out_n."""
    from velesdb_amd import _ffi
    w = worlds(po.COSINE, hw.SHAPES[0])
    allowed, qs, k, ef, chosen, want = overflow_case(w)
    with w.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as flt:
        (ids, sc, cnt), routes = w.ix.search_batch_filtered_graph(qs, k, flt, ef=ef, route=va.ROUTE_AUTO, max_list=chosen)
        assert routes.tolist() == want[2]
        q32 = np.ascontiguousarray(qs, dtype=np.float32)
        ids0, sc0, cnt0 = np.zeros((NQ, k), dtype=np.uint64), np.zeros((NQ, k), dtype=np.float32), np.full(NQ, 77, dtype=np.uint32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = _ffi.lib().vdb_hip_index_search_graph_filtered(w.ix._h, flt._h, vp(q32), NQ, k, ef, va.MODE_HNSW, va.ROUTE_AUTO, chosen,
                                                            vp(ids0), vp(sc0), vp(cnt0), None)
        assert rc == 0, _ffi.last_error()
        assert np.array_equal(ids0, ids) and np.array_equal(sc0.view(np.uint32), sc.view(np.uint32)) and np.array_equal(cnt0, cnt)


# ---- 5. life cycle --------------------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(va.VelesHipError) as e:
        fn()
    return e.value.code


class Live:
    """a graph built row by row on both sides (the GPU's sequential insert == the oracle's, link for link)"""

    def __init__(self, n, dim, seed):
        rng = np.random.default_rng(seed)
        self.metric, self.dim, self.n = po.EUCLIDEAN, dim, 0
        self.all_rows = rng.standard_normal((n + 64, dim)).astype(np.float32)
        self.qs = rng.standard_normal((NQ, dim)).astype(np.float32)
        self.g = po.NativeHnsw(dim, po.EUCLIDEAN, 8, 60, po.MODE_C)
        self.g.set_build_tie(po.TIE_CANONICAL)
        self.ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, n + 64))
        self.grow(n)

    def grow(self, to):
        for i in range(self.n, to):
            self.g.insert(self.all_rows[i])
            self.ix.insert(i, self.all_rows[i])
        self.n = to
        self.G = fw.Graph(self.g, self.all_rows[:to], po.EUCLIDEAN)


def test_life_cycle():
    L = Live(500, 48, 11)
    ix, k, ef = L.ix, 10, 32
    rng = np.random.default_rng(12)
    base = fw.random_filter(rng, L.n, 0.3)
    flt = ix.create_filter(np.flatnonzero(base).astype(np.uint64))

    def check(f, allowed, ctx, route=va.ROUTE_WALK):
        out, routes = ix.search_batch_filtered_graph(L.qs, k, f, ef=ef, route=route)
        want = expect_call(L, allowed, k, ef, route, matched=f.matched)
        assert 2 not in want[2] or route == va.ROUTE_EXACT
        assert_call((out, routes, ix.last_search_stats()), want, ctx)
        return out

    check(flt, base, "fresh")
    # rows removed after the filter was made drop out: allowed = filter AND live
    live = np.ones(L.n, dtype=bool)
    for r in np.flatnonzero(base)[:25]:
        assert ix.remove(int(r))
        live[r] = False
    check(flt, base & live, "after removes")
    check(flt, base & live, "after removes, exact", route=va.ROUTE_EXACT)
    # rows inserted after creation are walked through but never returned
    L.grow(540)
    grown = np.concatenate([base & live, np.zeros(40, dtype=bool)])
    out = check(flt, grown, "after inserts")
    assert np.all(out[0][out[0] != np.uint64(0xFFFFFFFFFFFFFFFF)] < 500)
    # a negated filter: every row present at creation except the given ones, dead rows dropped at search time
    live = np.concatenate([live, np.ones(40, dtype=bool)])
    with ix.create_filter(np.flatnonzero(base).astype(np.uint64), negate=True) as neg:
        check(neg, ~np.concatenate([base, np.zeros(40, dtype=bool)]) & live, "negated")
    # the empty filter: out_n = 0, nothing runs
    with ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        (ids, sc, cnt), routes = ix.search_batch_filtered_graph(L.qs, k, empty, ef=ef)
        assert np.all(cnt == 0) and np.all(routes == 0) and ix.last_kernels() == 0
    # refusals
    for mode in (va.MODE_BRUTE, va.MODE_AUTO, va.MODE_HNSW_INT8, va.MODE_HNSW_F16):
        assert code_of(lambda: ix.search_batch_filtered_graph(L.qs, k, flt, ef=ef, mode=mode)) == UNSUPPORTED
    assert code_of(lambda: ix.search_batch_filtered_graph(L.qs, k, flt, ef=ef, route=3)) == INVALID
    assert code_of(lambda: ix.search_batch_filtered_graph(L.qs, k, None, ef=ef)) == INVALID
    other = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    other.insert_batch_parallel([(i, L.all_rows[i]) for i in range(64)], 16)
    with other.create_filter(np.arange(10, dtype=np.uint64)) as foreign:
        assert code_of(lambda: ix.search_batch_filtered_graph(L.qs, k, foreign, ef=ef)) == INVALID
    other.close()
    group = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    group.insert_batch_parallel([(i, L.all_rows[i]) for i in range(64)], 16)
    assert code_of(lambda: group.search_batch_filtered_graph(L.qs, k, flt, ef=ef)) == UNSUPPORTED
    group.close()
    nograph = va.HnswIndex(L.dim, DM.Euclidean, va.HnswParams(8, 60, 64))
    nograph.upload(np.arange(64), L.all_rows[:64])
    with nograph.create_filter(np.arange(10, dtype=np.uint64)) as f2:
        assert code_of(lambda: nograph.search_batch_filtered_graph(L.qs, k, f2, ef=ef)) == STATE
    nograph.close()
    check(flt, grown, "after the refusals")  # the handle is as usable as before
    # vacuum renumbers the rows: the filter is stale
    ix.vacuum()
    assert code_of(lambda: ix.search_batch_filtered_graph(L.qs, k, flt, ef=ef)) == STATE
    flt.close()
    ix.close()


def test_four_threads_with_four_filters_get_what_they_get_alone(worlds):
    w, k, ef = worlds(po.COSINE, hw.SHAPES[0]), 10, 64
    names = ["half", "tenth", "clustered", "few"]
    for n in names:
        w.flt(n)
    alone = {n: run(w, n, k, ef, va.ROUTE_AUTO) for n in names}
    got, errors = {}, []

    def worker(n):
        try:
            for _ in range(3):
                out, routes = w.ix.search_batch_filtered_graph(w.qs, k, w.flt(n), ef=ef, route=va.ROUTE_AUTO)
                got[n] = (out, routes, w.ix.last_search_stats(), w.ix.last_kernels())
        except Exception as e:  # noqa: BLE001
            errors.append((n, e))
    threads = [threading.Thread(target=worker, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n in names:
        (ids, sc, cnt), routes, stats = alone[n]
        (gi, gs, gc), gr, gstats, gk = got[n]
        assert np.array_equal(gi, ids) and np.array_equal(gs.view(np.uint32), sc.view(np.uint32)) and np.array_equal(gc, cnt), n
        assert np.array_equal(gr, routes) and gstats == stats, n
        assert bool(gk & va.KERNEL_FILTER_RANK) == (n == "few") and bool(gk & va.KERNEL_HNSW_FILTERED) == (n != "few"), (n, hex(gk))
