"""GPU tests of one filter PER QUERY in one graph call (vdb_hip_index_search_graph_filters, csrc/hnsw_filtered.hip).

The contract under test: query i of a mixed batch gets, bit for bit, what search_batch_filtered_graph returns for that query ALONE
with its filter and the same k, ef, route, max_list — ids, ranks, score bits, out_n, padding, its route, and its share of the call's
n_dist / n_expand.  "No filter" is compared against create_filter([], negate=True).  The one-query call goes through the same host
path and the same kernels as the batch (the one-filter entry point is the per-query one with a table of one filter), so this is a
batch held against its queries one at a time: what a query computes must not depend on its companions or on the launches it shares.
So that the tests do not rest on the product alone, (k, ef) = (10, 64) is also checked against tests/filtered_walk_ref.py (a Python
model, never the product) at the query's own ladder, as tests/test_gpu_filtered_graph.py checks the one-filter entry point.  No
tolerances anywhere.
Worlds (oracle graph, dump, GPU handle, the five named filters), the reference protocol and the shapes are those of
tests/test_gpu_filtered_graph.py.
"""
import threading

import numpy as np
import pytest

import filtered_walk_ref as fw
import half_walk_ref as hw
import test_gpu_filtered_graph as fg
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
NQ = hw.NQ
INVALID, UNSUPPORTED, STATE = -1, -7, -8
NAMES = ["all", "half", "tenth", "clustered", "few", None]  # None = no filter
PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("filters_graph")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            w = cache[(metric, shape)] = fg.World(root, metric, shape)
            w.none = w.ix.create_filter(np.empty(0, dtype=np.uint64), negate=True)  # what "no filter" is defined as
            assert w.none.matched == w.n
        return cache[(metric, shape)]
    yield get
    for w in cache.values():
        w.none.close()
        w.close()


def flt_of(w, name):
    return None if name is None else w.flt(name)


def single_of(w, name):
    return w.none if name is None else w.flt(name)


def batch(ix, qs, k, filters, ef, route=0, max_list=0):
    out, routes = ix.search_batch_with_filters(qs, k, filters, ef=ef, route=route, max_list=max_list)
    return out, routes, ix.last_search_stats(), ix.last_kernels()


def singles(ix, qs, k, filters, ef, route=0, max_list=0):
    """the same queries as one-query calls of the single-filter entry: (per-query outputs, routes, summed stats, or-ed kernels)"""
    outs, routes, nd, ne, kern = [], [], 0, 0, 0
    for q, f in zip(qs, filters):
        o, r = ix.search_batch_filtered_graph(q[None, :], k, f, ef=ef, route=route, max_list=max_list)
        s = ix.last_search_stats()
        nd, ne, kern = nd + s[0], ne + s[1], kern | ix.last_kernels()
        outs.append((o[0][0], o[1][0], int(o[2][0])))
        routes.append(int(r[0]))
    return outs, routes, (nd, ne), kern


def assert_same(got, want, ctx):
    (ids, sc, cnt), routes, stats, kern = got
    outs, wroutes, wstats, wkern = want
    assert routes.tolist() == wroutes, ctx
    for qi, (wi, ws, wc) in enumerate(outs):
        c = int(cnt[qi])
        assert c == wc, (ctx, qi)
        assert np.all(ids[qi, c:] == PAD_ID) and np.all(sc[qi, c:].view(np.uint32) == 0x7FC00000), (ctx, qi)
        if wroutes[qi] == 0:  # nothing ran: the single call defines out_n = 0 only
            assert c == 0, (ctx, qi)
            continue
        assert np.array_equal(ids[qi], wi) and np.array_equal(sc[qi].view(np.uint32), ws.view(np.uint32)), (ctx, qi)
    assert tuple(stats) == tuple(wstats), (ctx, stats, wstats)
    assert kern == wkern, (ctx, hex(kern), hex(wkern))


def assert_reference(w, got, names, k, ef, live=None):
    """each query against tests/filtered_walk_ref.py at its own filter's plan (auto route, no max_list)"""
    (ids, sc, cnt), routes, stats, _ = got
    nd = ne = 0
    want_routes = []
    for qi, name in enumerate(names):
        flt = np.ones(w.n, dtype=bool) if name is None else w.filters[name]
        allowed = flt if live is None else flt & live
        wi, wb, wr, ws = fg.expect_call(w, allowed, k, ef, va.ROUTE_AUTO, matched=int(flt.sum()), qs=w.qs[qi:qi + 1])
        c = int(cnt[qi])
        assert int(routes[qi]) == wr[0] and ids[qi, :c].tolist() == wi[0], (qi, name)
        assert np.array_equal(sc[qi, :c].view(np.uint32), wb[0]), (qi, name)
        nd, ne = nd + ws[0], ne + ws[1]
        want_routes.append(wr[0])
    assert tuple(stats) == (nd, ne)
    return want_routes


def mixed_batch_case(w, k, ef, reference):
    names = [NAMES[i % len(NAMES)] for i in range(NQ)]
    got = batch(w.ix, w.qs, k, [flt_of(w, n) for n in names], ef)
    want = singles(w.ix, w.qs, k, [single_of(w, n) for n in names], ef)
    assert_same(got, want, (w.metric, w.shape, k, ef))
    if reference:
        want_routes = assert_reference(w, got, names, k, ef)
        assert 1 in want_routes and 2 in want_routes and all(r == 2 for r, n in zip(want_routes, names) if n == "few")
        assert got[3] & va.KERNEL_HNSW_FILTERED and got[3] & va.KERNEL_FILTER_RANK, hex(got[3])
    return got


# ---- 1. a mixed batch is the single calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_mixed_batch_equals_the_single_calls(worlds, metric, shape):
    w = worlds(metric, shape)
    assert int(w.filters["few"].sum()) < 64
    for k, ef in hw.KEF:
        mixed_batch_case(w, k, ef, reference=(k, ef) == (10, 64))


# ---- 2. the packed-bit metrics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [po.HAMMING, po.JACCARD])
def test_mixed_batch_bit_metrics(worlds, metric):
    w = worlds(metric, hw.SHAPES[0])
    for k, ef in [(10, 64), (10, 300)]:
        mixed_batch_case(w, k, ef, reference=(k, ef) == (10, 64))


# ---- 3. ladders and companions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_every_query_climbs_its_own_ladder_whatever_its_companions(worlds, metric):
    """The end-clustered filter and the shifted queries of the single-filter fallback test, in one call with "half" and unfiltered
    queries.  max_list is chosen with the reference so that some but not all clustered queries overflow it."""
    w, k, ef = worlds(metric, hw.SHAPES[0]), 10, 16
    allowed = np.zeros(w.n, dtype=bool)
    allowed[np.argsort(w.rows[:, 0])[-w.n // 10:]] = True
    qs = w.qs.copy()
    qs[:, 0] += np.resize(np.array([30, -30, 0, -4, -8, -2], dtype=np.float32), NQ)
    kinds = [("end", "half", None, "end")[i % 4] for i in range(NQ)]
    end_q = [i for i, n in enumerate(kinds) if n == "end"]
    ef_eff = fw.ef_rule(k, ef)
    sized = fw.sized_list(ef_eff, int(allowed.sum()), w.n)
    chosen = None
    for max_list in (4 * sized, 2 * sized, sized):
        over = [fg.protocol(w.G, qs[i], k, ef_eff, allowed, sized, max_list)[1] for i in end_q]
        if 0 < sum(over) < len(end_q):
            chosen = max_list
            break
    assert chosen is not None, "no list size splits the clustered queries: the case is meaningless"
    with w.ix.create_filter(np.flatnonzero(allowed).astype(np.uint64)) as end:
        def f(n, single=False):
            return end if n == "end" else (single_of(w, n) if single else flt_of(w, n))
        got = batch(w.ix, qs, k, [f(n) for n in kinds], ef, max_list=chosen)
        want = singles(w.ix, qs, k, [f(n, True) for n in kinds], ef, max_list=chosen)
        assert_same(got, want, ("ladders", chosen))
        for j, i in enumerate(end_q):  # the routes the reference chose max_list by
            assert int(got[1][i]) == (2 if over[j] else 1), i
        assert got[3] & va.KERNEL_HNSW_FILTERED and got[3] & va.KERNEL_FILTER_RANK
        # the same queries in another batch: other companions, another position — the same bits
        order = [i for i in reversed(range(NQ)) if i % 3 != 1]
        got2 = batch(w.ix, qs[order], k, [f(kinds[i]) for i in order], ef, max_list=chosen)
        for at, i in enumerate(order):
            assert got2[1][at] == got[1][i] and got2[0][2][at] == got[0][2][i], i
            assert np.array_equal(got2[0][0][at], got[0][0][i]), i
            assert np.array_equal(got2[0][1][at].view(np.uint32), got[0][1][i].view(np.uint32)), i
        # route 1: the queries that overflow the largest list fail the whole call, and nothing is written
        with pytest.raises(va.VelesHipError) as e:
            w.ix.search_batch_with_filters(qs, k, [f(n) for n in kinds], ef=ef, route=va.ROUTE_WALK, max_list=chosen)
        assert e.value.code == UNSUPPORTED and f"{sum(over)} queries overflow" in str(e.value), str(e.value)
        r = raw_call(w.ix, [end._h, w.flt("half")._h], [(0, 1, 2, 0)[i % 4] for i in range(NQ)], qs, k, ef=ef, route=va.ROUTE_WALK, max_list=chosen)
        assert r[0] == UNSUPPORTED and untouched(r)


# ---- 4. liveness -----------------------------------------------------------------------------------------------------------------------
def test_rows_removed_after_the_filters_exist_drop_out_inside_the_walk(tmp_path):
    w = fg.World(str(tmp_path), po.EUCLIDEAN, hw.SHAPES[2])
    w.none = w.ix.create_filter(np.empty(0, dtype=np.uint64), negate=True)
    names = [NAMES[i % len(NAMES)] for i in range(NQ)]
    filters, single = [flt_of(w, n) for n in names], [single_of(w, n) for n in names]
    rng = np.random.default_rng(5)
    dead = rng.choice(w.n, w.n // 20, replace=False)
    live = np.ones(w.n, dtype=bool)
    for r in dead:
        assert w.ix.remove(int(r))
        live[r] = False
    k, ef = 10, 64
    got = batch(w.ix, w.qs, k, filters, ef)
    assert_same(got, singles(w.ix, w.qs, k, single, ef), "after removes")
    assert_reference(w, got, names, k, ef, live=live)
    (ids, _, cnt), _, _, _ = got
    assert np.all(cnt > 0) and not set(dead.tolist()) & {int(i) for qi in range(NQ) for i in ids[qi, :int(cnt[qi])]}
    w.none.close()
    w.close()


# ---- 5. edges and errors ---------------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(va.VelesHipError) as e:
        fn()
    return e.value.code


def raw_call(ix, handles, fq, qs, k, ef=64, mode=None, route=0, max_list=0):
    """the entry point with a hand-made table -> (status, ids, scores, counts, routes); the outputs start as a known pattern"""
    import ctypes as C
    from velesdb_amd import _ffi
    nq = qs.shape[0]
    ids, sc = np.full((nq, max(k, 1)), 7, dtype=np.uint64), np.full((nq, max(k, 1)), 7.0, dtype=np.float32)
    cnt, routes = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint32)
    fq = np.asarray(fq, dtype=np.uint32)
    table = (C.c_void_p * max(len(handles), 1))(*handles)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().vdb_hip_index_search_graph_filters(ix._h, table if handles else None, len(handles), p(fq), p(qs), nq, k, ef,
                                                       va.MODE_HNSW if mode is None else mode, route, max_list, p(ids), p(sc), p(cnt), p(routes))
    return rc, ids, sc, cnt, routes


def untouched(r):
    return np.all(r[1] == 7) and np.all(r[2] == 7.0) and np.all(r[3] == 7) and np.all(r[4] == 7)


def test_edges_and_errors(worlds):
    w, k, ef = worlds(po.EUCLIDEAN, hw.SHAPES[2]), 10, 64
    ix, qs = w.ix, w.qs
    # no table at all: every query unfiltered
    got = batch(ix, qs, k, [None] * NQ, ef)
    assert_same(got, singles(ix, qs, k, [w.none] * NQ, ef), "n_filters = 0")
    rc, ids, sc, cnt, routes = raw_call(ix, [], [0] * NQ, qs, k)
    assert rc == 0 and np.array_equal(ids, got[0][0]) and np.array_equal(cnt, got[0][2]) and np.all(routes == 1)
    # an empty filter on some queries: out_n = 0 and route 0 for them only
    with ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        mix = [empty if i % 3 == 0 else (w.flt("half") if i % 3 == 1 else None) for i in range(NQ)]
        got = batch(ix, qs, k, mix, ef)
        assert_same(got, singles(ix, qs, k, [w.none if f is None else f for f in mix], ef), "empty among others")
        assert all((got[1][i] == 0 and got[0][2][i] == 0) == (i % 3 == 0) for i in range(NQ))
        got = batch(ix, qs, k, [empty] * NQ, ef)
        assert np.all(got[0][2] == 0) and np.all(got[1] == 0) and got[3] == 0
    # k = 0; one query
    (_, _, cnt), routes, _, kern = batch(ix, qs, 0, [w.flt("half"), None] * (NQ // 2), ef)
    assert np.all(cnt == 0) and np.all(routes == 0) and kern == 0
    for f, s in ((w.flt("tenth"), w.flt("tenth")), (None, w.none), (w.flt("few"), w.flt("few"))):
        assert_same(batch(ix, qs[3:4], k, [f], ef), singles(ix, qs[3:4], k, [s], ef), "nq = 1")
    with pytest.raises(ValueError, match="does not match filters count"):
        ix.search_batch_with_filters(qs, k, [None] * (NQ - 1))
    # refusals: a status, and the outputs as they were
    half, tenth = w.flt("half")._h, w.flt("tenth")._h
    fq = [i % 3 for i in range(NQ)]
    ok = raw_call(ix, [half, tenth], fq, qs, k)
    assert ok[0] == 0 and not untouched(ok)
    for r, code in ((raw_call(ix, [half, tenth], [3] + fq[1:], qs, k), INVALID),           # an index past "no filter"
                    (raw_call(ix, [half, None], fq, qs, k), INVALID),                      # a NULL table entry
                    (raw_call(ix, [half, tenth], fq, qs, k, route=3), INVALID),
                    (raw_call(ix, [half, tenth], fq, qs, k, mode=va.MODE_BRUTE), UNSUPPORTED),
                    (raw_call(ix, [half, tenth], fq, qs, k, mode=va.MODE_HNSW_F16), UNSUPPORTED)):
        assert r[0] == code and untouched(r), (r[0], code)
    n, dim, M, efc = w.shape
    other = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, 64))
    other.insert_batch_parallel([(i, w.rows[i]) for i in range(64)], 16)
    with other.create_filter(np.arange(10, dtype=np.uint64)) as foreign:
        r = raw_call(ix, [half, foreign._h], fq, qs, k)  # (even when no query names it: the whole table is checked)
        assert r[0] == INVALID and untouched(r)
        r = raw_call(ix, [half, foreign._h], [0] * NQ, qs, k)
        assert r[0] == INVALID and untouched(r)
    other.close()
    group = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, 64), devices=[0, 0], shard_mode=va.SHARD_REPLICA)
    group.insert_batch_parallel([(i, w.rows[i]) for i in range(64)], 16)
    assert code_of(lambda: group.search_batch_with_filters(qs, k, [None] * NQ, ef=ef)) == UNSUPPORTED
    group.close()
    nograph = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, 64))
    nograph.upload(np.arange(64), w.rows[:64])
    assert code_of(lambda: nograph.search_batch_with_filters(qs, k, [None] * NQ, ef=ef)) == STATE
    nograph.close()
    assert_same(batch(ix, qs, k, [w.flt("half")] * NQ, ef), singles(ix, qs, k, [w.flt("half")] * NQ, ef), "after the refusals")


def test_a_stale_filter_in_the_table_is_a_state_error(tmp_path):
    w = fg.World(str(tmp_path), po.EUCLIDEAN, hw.SHAPES[2])
    half, tenth = w.flt("half"), w.flt("tenth")
    assert w.ix.remove(5)
    w.ix.vacuum()
    with w.ix.create_filter(np.arange(100, dtype=np.uint64)) as fresh:
        r = raw_call(w.ix, [fresh._h, tenth._h], [0] * NQ, w.qs, 10)  # the stale one is not even named by a query
        assert r[0] == STATE and untouched(r)
        assert code_of(lambda: w.ix.search_batch_with_filters(w.qs, 10, [half] * NQ, ef=64)) == STATE
        assert raw_call(w.ix, [fresh._h], [i % 2 for i in range(NQ)], w.qs, 10)[0] == 0
    w.close()


# ---- 6. threads ------------------------------------------------------------------------------------------------------------------------
def test_four_threads_with_four_mixed_batches_get_what_they_get_alone(worlds):
    w, k, ef = worlds(po.COSINE, hw.SHAPES[0]), 10, 64
    mixes = {t: [flt_of(w, NAMES[(i * (t + 1) + t) % len(NAMES)]) for i in range(NQ)] for t in range(4)}
    alone = {t: batch(w.ix, w.qs, k, mixes[t], ef) for t in mixes}
    got, errors = {}, []

    def worker(t):
        try:
            for _ in range(3):
                got[t] = batch(w.ix, w.qs, k, mixes[t], ef)
        except Exception as e:  # noqa: BLE001
            errors.append((t, e))
    threads = [threading.Thread(target=worker, args=(t,)) for t in mixes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in mixes:
        (ids, sc, cnt), routes, stats, kern = alone[t]
        (gi, gs, gc), gr, gstats, gk = got[t]
        assert np.array_equal(gi, ids) and np.array_equal(gs.view(np.uint32), sc.view(np.uint32)) and np.array_equal(gc, cnt), t
        assert np.array_equal(gr, routes) and gstats == stats and gk == kern, t
