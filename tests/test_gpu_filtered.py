"""Filtered exact search on the GPU (vdb_hip_index_search_batch_filtered).

The contract: a filtered call returns, bit for bit, what VDB_SEARCH_BRUTE returns on an index that holds only the allowed, live
rows, inserted in the same order under the same ids — ids, ranks, counts and score bits, on both routes (the listed sweep and
mask substitution) and at every tier mask substitution reaches.  The expected answer is always the oracle over that subset
(`po.scan_topk(metric, rows[sel], Q, min(k, len(sel)), mode)`, mode from `sweep_arith_mode`), ids mapped back through `sel`.
Nothing is compared approximately.  References are computed once per (metric, shape, arithmetic mode) and shared by the tests."""
import threading

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
FLOATS = [DM.Cosine, DM.DotProduct, DM.Euclidean]
BITS = [DM.Hamming, DM.Jaccard]
FLOAT_SHAPES = [(5000, 100), (3000, 17), (2500, 768), (777, 3)]
BIT_SHAPES = [(5000, 48), (2500, 768)]  # few distinct integer distances: heavy ties at rank k
NQ_K = [(1, 10), (3, 1), (8, 10), (17, 5), (2, 64), (5, 200), (70, 10)]
K0 = 10  # the "k - 1 rows" / "exactly k rows" sets are taken for k = 10


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rand_rows(rng, n, d, metric):
    if metric in (DM.Hamming, DM.Jaccard):
        return (rng.random((n, d)) > 0.6915).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)


def ext_ids(n):
    return np.arange(n, dtype=np.uint64) * 3 + 11  # non-contiguous external ids


def oracle_subset(metric, rows, ids, queries, k, sel, mode):
    """tests/test_gpu_sweep.py::oracle_brute over the rows `sel` (ascending internal rows): [(ids, scores)] per query"""
    n = min(k, len(sel))
    if n == 0:
        return [(np.empty(0, np.uint64), np.empty(0, np.float32)) for _ in range(queries.shape[0])]
    r, s = po.scan_topk(int(metric), rows[sel], queries, n, mode, nthreads=po.host_threads())
    return [(ids[sel[r[qi, :n].astype(np.int64)]], s[qi, :n]) for qi in range(queries.shape[0])]


def arith_mode(ix, k):
    return po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C


def allowed_sets(rng, n):
    """name -> (internal rows passed to create_filter, negate, expected ascending internal rows).  Every set but the one-row set
    holds internal row 0 and the last row (the one-row set is row n - 1)."""
    def with_ends(m):
        mid = rng.choice(np.arange(1, n - 1), size=max(0, m - 2), replace=False)
        return np.sort(np.concatenate([[0, n - 1], mid])).astype(np.int64)
    out = {"one": np.array([n - 1], dtype=np.int64), "k-1": with_ends(K0 - 1), "k": with_ends(K0), "1pct": with_ends(max(3, n // 100)),
           "half": with_ends(n // 2), "all": np.arange(n, dtype=np.int64)}
    sets = {name: (rows, False, rows) for name, rows in out.items()}
    excl = np.sort(rng.choice(np.arange(1, n - 1), size=n // 10, replace=False)).astype(np.int64)
    sets["not10pct"] = (excl, True, np.setdiff1d(np.arange(n, dtype=np.int64), excl))
    return sets


_CASES = {}


def case(metric, n, dim, mode_name):
    """rows, queries, sets and the oracle's answers for one (metric, shape, arithmetic mode): built once, shared, never changed"""
    key = (int(metric), n, dim, mode_name)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n + dim + int(metric))
        rows, ids = rand_rows(rng, n, dim, metric), ext_ids(n)
        sets = allowed_sets(rng, n)
        qs = {(nq, k): rand_rows(rng, nq, dim, metric) for nq, k in NQ_K}
        mode = po.MODE_M if mode_name == "M" else po.MODE_C
        exp = {(name, nq, k): oracle_subset(metric, rows, ids, qs[(nq, k)], k, sets[name][2], mode) for name in sets for nq, k in NQ_K}
        _CASES[key] = dict(rows=rows, ids=ids, sets=sets, qs=qs, exp=exp)
    return _CASES[key]


def assert_equal(got, exp, what):
    gid, gsc, gcnt = got
    for qi, (eid, esc) in enumerate(exp):
        assert gcnt[qi] == len(eid), (what, qi, int(gcnt[qi]), len(eid))
        assert np.array_equal(gid[qi, :gcnt[qi]], eid), (what, qi)
        assert np.array_equal(bits(gsc[qi, :gcnt[qi]]), bits(esc)), (what, qi)


def run_case(metric, n, dim, route, want_listed):
    ix = va.HnswIndex(dim, metric)
    try:
        mode_name = ix.sweep_arith_mode(10)
        c = case(metric, n, dim, mode_name)
        assert all(ix.sweep_arith_mode(k) == mode_name for _, k in NQ_K)
        assert ix.upload(c["ids"], c["rows"]) == n
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        for name, (given, negate, sel) in c["sets"].items():
            with ix.create_filter(c["ids"][given], negate=negate) as flt:
                assert flt.matched == len(sel), name
                for nq, k in NQ_K:
                    got = ix.search_batch_brute_force_filtered(c["qs"][(nq, k)], k, flt)
                    listed = bool(ix.last_kernels() & va.KERNEL_SWEEP_LISTED)
                    assert listed == want_listed, (name, nq, k, hex(ix.last_kernels()))
                    assert_equal(got, c["exp"][(name, nq, k)], (str(metric), n, dim, name, nq, k, route))
    finally:
        ix.close()


# ---- 1. the listed sweep, forced ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", FLOATS)
@pytest.mark.parametrize("n,dim", FLOAT_SHAPES)
def test_listed_route_bit_exact(gpu_required, metric, n, dim):
    run_case(metric, n, dim, va.FILTER_ROUTE_LISTED, want_listed=True)


@pytest.mark.parametrize("n,dim", FLOAT_SHAPES)
def test_listed_route_cosine_mode_c_body(gpu_required, n, dim):
    """engine 0: a Cosine handle answers in mode C, so the listed sweep's mode-C body serves it"""
    va.set_sweep_engine(0)
    try:
        ix = va.HnswIndex(dim, DM.Cosine)
        assert ix.sweep_arith_mode(10) == "C"
        ix.close()
        run_case(DM.Cosine, n, dim, va.FILTER_ROUTE_LISTED, want_listed=True)
    finally:
        va.set_sweep_engine(1)


# ---- 2. mask substitution, forced -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,dim", [(m, n, d) for m in FLOATS for n, d in FLOAT_SHAPES] + [(m, n, d) for m in BITS for n, d in BIT_SHAPES])
def test_mask_route_bit_exact(gpu_required, metric, n, dim):
    run_case(metric, n, dim, va.FILTER_ROUTE_MASK, want_listed=False)


def test_bit_metrics_have_no_listed_kernel(gpu_required):
    """Hamming / Jaccard always take mask substitution, whatever the option says"""
    run_case(DM.Hamming, 5000, 48, va.FILTER_ROUTE_LISTED, want_listed=False)


# ---- 3. mask substitution through the selection stage ------------------------------------------------------------------------
@pytest.mark.parametrize("metric", FLOATS)
def test_mask_route_through_the_selection_stage(gpu_required, metric):
    n, dim, nq = 66000, 128, 64
    rng = np.random.default_rng(77 + int(metric))
    rows, ids = rand_rows(rng, n, dim, metric), ext_ids(n)
    Q = rand_rows(rng, nq, dim, metric)
    ix = va.HnswIndex(dim, metric)
    try:
        assert ix.upload(ids, rows) == n
        ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_MASK)
        sets = {"half": np.sort(rng.choice(n, size=n // 2, replace=False)), "1/64": np.arange(5, n, 64), "7rows": np.sort(rng.choice(n, size=7, replace=False))}
        for k in (10, 50):
            mode = arith_mode(ix, k)
            full = oracle_subset(metric, rows, ids, Q, k, np.arange(n), mode)
            before = ix.search_batch_brute_force(Q, k)
            level = ix.last_select_level()
            assert level == 4, level  # the WIDE selection serves this shape at both k
            assert_equal(before, full, ("unfiltered before", k))
            for name, sel in sets.items():
                with ix.create_filter(ids[sel]) as flt:
                    got = ix.search_batch_brute_force_filtered(Q, k, flt)
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                    if name == "half":
                        assert ix.last_select_level() == level  # the filtered call went through the selection stage itself
                    assert_equal(got, oracle_subset(metric, rows, ids, Q, k, sel, mode), (str(metric), name, k))
            after = ix.search_batch_brute_force(Q, k)
            assert ix.last_select_level() == level, "a filtered call moved the handle's selector"
            assert_equal(after, full, ("unfiltered after", k))
    finally:
        ix.close()


# ---- 4. the route never changes a result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,dim", [(DM.Cosine, 2500, 768), (DM.DotProduct, 5000, 100), (DM.Euclidean, 3000, 17), (DM.Hamming, 5000, 48),
                                          (DM.Jaccard, 2500, 768)])
def test_routes_agree(gpu_required, metric, n, dim):
    ix = va.HnswIndex(dim, metric)
    try:
        c = case(metric, n, dim, ix.sweep_arith_mode(10))
        ix.upload(c["ids"], c["rows"])
        for name in ("1pct", "half", "not10pct"):
            given, negate, _ = c["sets"][name]
            with ix.create_filter(c["ids"][given], negate=negate) as flt:
                for nq, k in ((1, 10), (17, 5), (70, 10)):
                    res = []
                    for route in (va.FILTER_ROUTE_AUTO, va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK):
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        res.append(ix.search_batch_brute_force_filtered(c["qs"][(nq, k)], k, flt))
                    for other in res[1:]:
                        assert np.array_equal(res[0][2], other[2])
                        assert np.array_equal(res[0][0], other[0]) and np.array_equal(bits(res[0][1]), bits(other[1])), (name, nq, k)
                    assert_equal(res[0], c["exp"][(name, nq, k)], (name, nq, k))
    finally:
        ix.close()


# ---- 5. exact ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", FLOATS)
@pytest.mark.parametrize("route", [1, 2])
def test_exact_copies_keep_insertion_order(gpu_required, metric, route):
    n, dim = 1200, 100
    rng = np.random.default_rng(5)
    rows, ids = rand_rows(rng, n, dim, metric), ext_ids(n)
    rows[900] = rows[300]   # allowed copies of row 300, which is NOT allowed
    rows[40] = rows[300]
    ix = va.HnswIndex(dim, metric)
    try:
        ix.upload(ids, rows)
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        sel = np.setdiff1d(np.arange(n), [300])
        with ix.create_filter(ids[[300]], negate=True) as flt:
            got = ix.search_batch_brute_force_filtered(rows[300:301], 5, flt)
        gid, gsc, gcnt = got
        assert gcnt[0] == 5 and ids[300] not in gid[0]
        if metric != DM.DotProduct:  # (a longer row may beat the copy under DotProduct)
            assert list(gid[0, :2]) == [ids[40], ids[900]] and bits(gsc[0, 0]) == bits(gsc[0, 1])
        pos = {int(v): i for i, v in enumerate(gid[0])}
        assert pos[int(ids[40])] + 1 == pos[int(ids[900])]
        assert_equal(got, oracle_subset(metric, rows, ids, rows[300:301], 5, sel, arith_mode(ix, 5)), (str(metric), route))
    finally:
        ix.close()


# ---- 6. snapshot semantics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_snapshot_semantics(gpu_required, route):
    n, dim, k = 1000, 64, 10
    rng = np.random.default_rng(9)
    rows, ids = rand_rows(rng, n + 1, dim, DM.Cosine), ext_ids(n + 1)
    Q = rand_rows(rng, 3, dim, DM.Cosine)
    ix = va.HnswIndex(dim, DM.Cosine)
    other = va.HnswIndex(dim, DM.Cosine)
    try:
        ix.upload(ids[:n], rows[:n])
        other.upload(ids[:n], rows[:n])
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        mode = arith_mode(ix, k)
        sel = np.sort(rng.choice(n, size=12, replace=False))
        # unknown ids (one of them arrives later), duplicates: ignored
        given = np.concatenate([ids[sel], ids[sel[:4]], [ids[n]], [7, 8]]).astype(np.uint64)
        flt = ix.create_filter(given)
        assert flt.matched == 12
        assert_equal(ix.search_batch_brute_force_filtered(Q, k, flt), oracle_subset(DM.Cosine, rows, ids, Q, k, sel, mode), "fresh")
        # removals after creation: the rows disappear, out_n shrinks below k
        for gone in sel[:3]:
            assert ix.remove(int(ids[gone]))
        got = ix.search_batch_brute_force_filtered(Q, k, flt)
        assert list(got[2]) == [9, 9, 9]
        assert_equal(got, oracle_subset(DM.Cosine, rows, ids, Q, k, sel[3:], mode), "after removals")
        # an id of the creation list that did not exist then is inserted now: not in the filter
        ix.upload(ids[n:n + 1], rows[n:n + 1])
        got = ix.search_batch_brute_force_filtered(Q, k, flt)
        assert ids[n] not in got[0]
        assert_equal(got, oracle_subset(DM.Cosine, rows, ids, Q, k, sel[3:], mode), "after an insert")
        # negate counts every row present (soft-deleted ones included) and drops the dead at search time
        with ix.create_filter(ids[sel[3:]], negate=True) as neg:
            assert neg.matched == n + 1 - 9
            live = np.setdiff1d(np.arange(n + 1), sel)
            assert_equal(ix.search_batch_brute_force_filtered(Q, k, neg), oracle_subset(DM.Cosine, rows, ids, Q, k, live, mode), "negate")
        # the empty filter
        with ix.create_filter(np.empty(0, np.uint64)) as empty:
            assert empty.matched == 0
            assert list(ix.search_batch_brute_force_filtered(Q, k, empty)[2]) == [0, 0, 0]
        # a filter of another handle
        with other.create_filter(ids[sel]) as foreign:
            with pytest.raises(va.VelesHipError) as e:
                ix.search_batch_brute_force_filtered(Q, k, foreign)
            assert e.value.code in (va._ffi.VDB_ERR_INVALID_ARG, va._ffi.VDB_ERR_STATE)
        # no filter at all
        with pytest.raises(va.VelesHipError) as e:
            ix.search_batch_brute_force_filtered(Q, k, None)
        assert e.value.code == va._ffi.VDB_ERR_INVALID_ARG
        # vacuum renumbers the rows: the old filter is stale
        ix.vacuum()
        with pytest.raises(va.VelesHipError) as e:
            ix.search_batch_brute_force_filtered(Q, k, flt)
        assert e.value.code == va._ffi.VDB_ERR_STATE
        flt.close()
        live = np.setdiff1d(np.arange(n + 1), sel[:3])
        keep = np.intersect1d(live, sel)
        with ix.create_filter(ids[keep]) as again:  # a new filter on the vacuumed handle works
            assert again.matched == 9
            assert_equal(ix.search_batch_brute_force_filtered(Q, k, again), oracle_subset(DM.Cosine, rows, ids, Q, k, keep, mode), "after vacuum")
    finally:
        ix.close()
        other.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(gpu_required):
    n, dim = 600, 32
    rng = np.random.default_rng(3)
    rows, ids = rand_rows(rng, n, dim, DM.Cosine), ext_ids(n)
    ix = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n))
    try:
        ix.insert_batch_parallel((int(i), r) for i, r in zip(ids, rows))
        with ix.create_filter(ids[:100]) as flt:
            for mode in (va.MODE_HNSW, va.MODE_BRUTE_BF16, va.MODE_BRUTE_SQ8, va.MODE_AUTO, va.MODE_HNSW_INT8):
                with pytest.raises(va.VelesHipError) as e:
                    ix.search_batch_brute_force_filtered(rows[:2], 5, flt, mode=mode)
                assert e.value.code == va._ffi.VDB_ERR_UNSUPPORTED, mode
            assert ix.search_batch_brute_force_filtered(rows[:2], 5, flt)[2].tolist() == [5, 5]
    finally:
        ix.close()
    sh = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    try:
        sh.upload(ids, rows)
        with pytest.raises(va.VelesHipError) as e:
            sh.create_filter(ids[:10])
        assert e.value.code == va._ffi.VDB_ERR_UNSUPPORTED
    finally:
        sh.close()


# ---- 8. callers -------------------------------------------------------------------------------------------------------------
def test_concurrent_filtered_and_unfiltered_callers(gpu_required):
    n, dim, k, rounds = 6000, 96, 10, 20
    rng = np.random.default_rng(21)
    rows, ids = rand_rows(rng, n, dim, DM.Cosine), ext_ids(n)
    Q = rand_rows(rng, rounds, dim, DM.Cosine)
    ix = va.HnswIndex(dim, DM.Cosine)
    try:
        ix.upload(ids, rows)
        sizes = [1, 9, 60, 300, 1500, 3000, 4500, 6000]
        filters = [ix.create_filter(ids[np.sort(rng.choice(n, size=s, replace=False))]) for s in sizes]
        # every call made alone first
        alone = [[ix.search_brute_force_filtered(Q[i], k, f) for i in range(rounds)] for f in filters]
        alone_plain = [ix.search_brute_force(Q[i], k) for i in range(rounds)]
        errors = []

        def filtered(t):
            try:
                for i in range(rounds):
                    if ix.search_brute_force_filtered(Q[i], k, filters[t]) != alone[t][i]:
                        errors.append(("filtered", t, i))
            except Exception as ex:  # noqa: BLE001
                errors.append(("filtered", t, repr(ex)))

        def plain():
            try:
                for r in range(3):
                    for i in range(rounds):
                        if ix.search_brute_force(Q[i], k) != alone_plain[i]:
                            errors.append(("plain", r, i))
            except Exception as ex:  # noqa: BLE001
                errors.append(("plain", repr(ex)))

        threads = [threading.Thread(target=filtered, args=(t,)) for t in range(8)] + [threading.Thread(target=plain)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:5]
        for f in filters:
            f.close()
    finally:
        ix.close()
