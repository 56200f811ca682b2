"""One filter per query on the exact sweep (vdb_hip_index_search_batch_filters).

The contract: query i of the call gets, bit for bit, what vdb_hip_index_search_batch_filtered returns for that query ALONE with
its filter and the same k (a query without a filter: what search_batch_brute_force returns for it alone) — ids, counts, score bits
and padding — whatever its companions, its position, VDB_OPT_FILTER_ROUTE and the grouping of the call are.  The expected answer
is therefore always a loop of single-query calls on the same handle, made once per (case, k) and shared; for one shape per
arithmetic mode it is also the oracle over each query's subset (tests/test_gpu_filtered.py::oracle_subset).  Nothing is compared
approximately.  Shapes, row generators and the oracle helper are tests/test_gpu_filtered.py's.

The plan diagnostic counts the GROUPED launches only: a call that runs the one-filter path itself reports out[4] = out[5] = 0 (its
launches are the one-filter call's, which last_kernels shows)."""
import threading

import numpy as np
import pytest

import test_gpu_filtered as tf

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
bits = tf.bits
K0 = tf.K0
KS = (1, 10, 64, 200)
GROUP_SIZES = (1, 2, 4, 5, 8, 9, 16, 17)  # the B classes 1 / 4 / 8 and the 8- and 16-query pass boundaries
N_UNFILTERED = 6
ROUTES = (va.FILTER_ROUTE_AUTO, va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK)


def filter_sets(rng, n):
    """[(internal rows handed to create_filter, negate, expected ascending rows)]: the boundaries of the row groups (RPG = 64 / B)
    and of the 64-row tile, the k boundaries for k = 10, the empty set, a dense set and a negated one"""
    sets = []
    for c in (0, 1, K0 - 1, K0, 15, 16, 17, 63, 64, 65, max(1, n // 100), n // 2):
        rows = np.sort(rng.choice(n, size=c, replace=False)).astype(np.int64)
        sets.append((rows, False, rows))
    excl = np.sort(rng.choice(n, size=n // 10, replace=False)).astype(np.int64)
    sets.append((excl, True, np.setdiff1d(np.arange(n, dtype=np.int64), excl)))
    return sets


def mixed_table(rng, n_sets):
    """filter index per query (None = unfiltered): group g has GROUP_SIZES[g % 8] queries, six queries have no filter, and the
    whole is shuffled so that no group is contiguous in the call"""
    fq = []
    for g in range(n_sets):
        fq += [g] * GROUP_SIZES[g % len(GROUP_SIZES)]
    fq += [None] * N_UNFILTERED
    return [fq[i] for i in rng.permutation(len(fq))]


_CASES = {}


def case(metric, n, dim):
    key = (int(metric), n, dim)
    if key not in _CASES:
        rng = np.random.default_rng(4100 * n + dim + int(metric))
        rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
        sets = filter_sets(rng, n)
        fq = mixed_table(rng, len(sets))
        Q = tf.rand_rows(rng, len(fq), dim, metric)
        _CASES[key] = dict(rows=rows, ids=ids, sets=sets, fq=fq, Q=Q)
    return _CASES[key]


class World:
    """a handle with the case's rows and one Filter object per set"""

    def __init__(self, metric, n, dim):
        self.c = case(metric, n, dim)
        self.ix = va.HnswIndex(dim, metric)
        assert self.ix.upload(self.c["ids"], self.c["rows"]) == n
        self.filters = [self.ix.create_filter(self.c["ids"][given], negate=neg) for given, neg, _ in self.c["sets"]]
        for f, (_, _, sel) in zip(self.filters, self.c["sets"]):
            assert f.matched == len(sel)

    def table(self, fq=None):
        return [None if g is None else self.filters[g] for g in (self.c["fq"] if fq is None else fq)]

    def alone(self, Q, fq, k):
        """the expected answer: every query alone through the one-filter call (or the plain call), route auto"""
        self.ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_AUTO)
        nq, kk = len(fq), max(k, 1)
        ids, sc, cnt = np.empty((nq, kk), np.uint64), np.empty((nq, kk), np.float32), np.zeros(nq, np.uint32)
        for i, g in enumerate(fq):
            if g is None:
                a, b, c = self.ix.search_batch_brute_force(Q[i:i + 1], k)
            else:
                a, b, c = self.ix.search_batch_brute_force_filtered(Q[i:i + 1], k, self.filters[g])
            ids[i], sc[i], cnt[i] = a[0], b[0], c[0]
        return ids, sc, cnt

    def close(self):
        for f in self.filters:
            f.close()
        self.ix.close()


PAD_ID, PAD_SCORE = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint32(0x7FC00000)  # what the merge writes behind a query's out_n results


def same(got, exp, what):
    """counts, ids and score bits of every query's results; behind them `got` holds the merge's padding — also for a query of an
    empty filter, where the one-filter call leaves its outputs unwritten (there is nothing to compare them to)"""
    assert np.array_equal(got[2], exp[2]), (what, got[2].tolist(), exp[2].tolist())
    gb, eb = bits(got[1]), bits(exp[1])
    for i, c in enumerate(got[2]):
        assert np.array_equal(got[0][i, :c], exp[0][i, :c]) and np.array_equal(gb[i, :c], eb[i, :c]), (what, i)
        assert (got[0][i, c:] == PAD_ID).all() and (gb[i, c:] == PAD_SCORE).all(), (what, i, "padding")
        if exp[2][i]:  # the reference merged this query: its padding is the same
            assert np.array_equal(got[0][i], exp[0][i]) and np.array_equal(gb[i], eb[i]), (what, i)


def run_mixed(metric, n, dim, oracle_too=False):
    w = World(metric, n, dim)
    try:
        ix, c = w.ix, w.c
        for k in KS:
            exp = w.alone(c["Q"], c["fq"], k)
            res = []
            for route in ROUTES:
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                got = ix.search_batch_brute_force_with_filters(c["Q"], k, w.table())
                plan = ix.last_filters_exact_plan()
                assert plan[0] == len(c["sets"]) and plan[3] == N_UNFILTERED and plan[1] + plan[2] == plan[0], plan
                if route == va.FILTER_ROUTE_LISTED:
                    # every group but the empty one is on the grouped route: a constant number of launches for 12 filters
                    assert plan[1] == len(c["sets"]) - 1 and 1 <= plan[4] <= 4 and plan[5] == 1, plan
                    assert ix.last_kernels() & va.KERNEL_SWEEP_LISTED_GROUPS
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                if route == va.FILTER_ROUTE_MASK:
                    assert plan[1] == 0 and plan[4] == 0 and plan[5] == 0, plan
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED_GROUPS
                same(got, exp, (str(metric), n, dim, k, route))
                res.append(got)
            for other in res[1:]:
                same(other, res[0], (str(metric), n, dim, k, "routes agree"))
            # the empty filter's queries: out_n = 0 while the others are answered
            empty = [i for i, g in enumerate(c["fq"]) if g == 0]
            assert empty and all(res[0][2][i] == 0 for i in empty)
            if oracle_too and k == 10:
                mode = tf.arith_mode(ix, k)
                for g, (_, _, sel) in enumerate(c["sets"] + [(None, None, np.arange(n, dtype=np.int64))]):
                    qi = [i for i, f in enumerate(c["fq"]) if f == (g if g < len(c["sets"]) else None)]
                    exp_o = tf.oracle_subset(metric, c["rows"], c["ids"], c["Q"][qi], k, sel, mode)
                    tf.assert_equal((res[0][0][qi], res[0][1][qi], res[0][2][qi]), exp_o, (str(metric), "oracle", g))
    finally:
        w.close()


# ---- 1. the mixed table: every float metric x shape, k in (1, 10, 64, 200), the three routes ---------------------------------
@pytest.mark.parametrize("metric", tf.FLOATS)
@pytest.mark.parametrize("n,dim", tf.FLOAT_SHAPES)
def test_mixed_table_bit_exact(gpu_required, metric, n, dim):
    # the oracle itself for one shape per arithmetic mode: Cosine 2500 x 768 (mode M), Euclidean 3000 x 17 (mode C)
    run_mixed(metric, n, dim, oracle_too=(metric, n, dim) in ((DM.Cosine, 2500, 768), (DM.Euclidean, 3000, 17)))


@pytest.mark.parametrize("n,dim", tf.FLOAT_SHAPES)
def test_mixed_table_cosine_mode_c_body(gpu_required, n, dim):
    """engine 0: a Cosine handle answers in mode C, so the grouped mode-C Cosine body serves the listed groups"""
    va.set_sweep_engine(0)
    try:
        ix = va.HnswIndex(dim, DM.Cosine)
        assert ix.sweep_arith_mode(10) == "C"
        ix.close()
        run_mixed(DM.Cosine, n, dim)
    finally:
        va.set_sweep_engine(1)


@pytest.mark.parametrize("metric,dim,engine", [(DM.Euclidean, 512, 1), (DM.Euclidean, 1024, 1), (DM.Cosine, 1024, 0), (DM.DotProduct, 1024, 0)])
def test_instances_with_fewer_rows_in_flight(gpu_required, metric, dim, engine):
    """the grouped mode-C instances that fetch 2 rows (or 1) at a time where the one-filter kernels fetch 4 — B = 1 at dim 512 /
    768 / 1024 (Euclidean) and 1024 (Cosine / DotProduct with the engine off), B = 4 at dim 1024 (Euclidean); dim 768 is in the
    mixed table: one-query and three-query groups on the forced listed route, against the single calls and the oracle"""
    n, k = 600, 10
    va.set_sweep_engine(engine)
    try:
        rng = np.random.default_rng(dim + int(metric))
        rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
        ix = va.HnswIndex(dim, metric)
        try:
            assert ix.sweep_arith_mode(k) == "C"
            ix.upload(ids, rows)
            ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_LISTED)
            sels = [np.sort(rng.choice(n, size=c, replace=False)) for c in (1, 63, 65, 300)]
            flts = [ix.create_filter(ids[s]) for s in sels]
            fq = [0, 1, 3, 2, 1, 3, 1, 3]  # groups of 1, 3, 1 and 3 queries: B = 1 and B = 4 passes
            Q = tf.rand_rows(rng, len(fq), dim, metric)
            got = ix.search_batch_brute_force_with_filters(Q, k, [flts[g] for g in fq])
            plan = ix.last_filters_exact_plan()
            assert plan[:4] == (4, 4, 0, 0) and plan[4] == 2 and plan[5] == 1, plan
            mode = tf.arith_mode(ix, k)
            for i, g in enumerate(fq):
                same(tuple(a[i:i + 1] for a in got), ix.search_batch_brute_force_filtered(Q[i:i + 1], k, flts[g]), (str(metric), dim, i))
                tf.assert_equal(tuple(a[i:i + 1] for a in got), tf.oracle_subset(metric, rows, ids, Q[i:i + 1], k, sels[g], mode), (str(metric), dim, i))
            for f in flts:
                f.close()
        finally:
            ix.close()
    finally:
        va.set_sweep_engine(1)


# ---- 2. Hamming / Jaccard: mask substitution per group -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", tf.BITS)
def test_bit_metrics_take_mask_substitution_per_group(gpu_required, metric):
    n, dim = 2500, 768
    w = World(metric, n, dim)
    try:
        ix, c = w.ix, w.c
        for k in (10, 64):
            exp = w.alone(c["Q"], c["fq"], k)
            for route in ROUTES:
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                got = ix.search_batch_brute_force_with_filters(c["Q"], k, w.table())
                plan = ix.last_filters_exact_plan()
                assert plan[1] == 0 and plan[4] == 0 and plan[2] == len(c["sets"]), plan
                same(got, exp, (str(metric), k, route))
    finally:
        w.close()


# ---- 3. a permutation of the queries permutes the outputs and changes no bit -------------------------------------------------
@pytest.mark.parametrize("metric,n,dim", [(DM.Cosine, 2500, 768), (DM.Euclidean, 5000, 100)])
def test_permutation_changes_no_bit(gpu_required, metric, n, dim):
    w = World(metric, n, dim)
    try:
        ix, c = w.ix, w.c
        rng = np.random.default_rng(8)
        for route in (va.FILTER_ROUTE_AUTO, va.FILTER_ROUTE_LISTED):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            base = ix.search_batch_brute_force_with_filters(c["Q"], 10, w.table())
            for _ in range(2):
                p = rng.permutation(len(c["fq"]))
                got = ix.search_batch_brute_force_with_filters(c["Q"][p], 10, w.table([c["fq"][i] for i in p]))
                same(got, tuple(a[p] for a in base), (str(metric), route, "permuted"))
            # a query among fewer companions: the first 11 queries only
            got = ix.search_batch_brute_force_with_filters(c["Q"][:11], 10, w.table(c["fq"][:11]))
            same(got, tuple(a[:11] for a in base), (str(metric), route, "prefix"))
    finally:
        w.close()


# ---- 4. exact copies of a row across two filters' lists keep insertion order per query -----------------------------------------
@pytest.mark.parametrize("metric", tf.FLOATS)
@pytest.mark.parametrize("route", [va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK])
def test_exact_copies_keep_insertion_order(gpu_required, metric, route):
    n, dim = 1200, 100
    rng = np.random.default_rng(5)
    rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
    rows[900] = rows[300]
    rows[40] = rows[300]
    rows[700] = rows[300]
    ix = va.HnswIndex(dim, metric)
    try:
        ix.upload(ids, rows)
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        a_rows = np.sort(np.concatenate([[40, 900], rng.choice(np.arange(1000, 1200), size=30, replace=False)]))
        b_rows = np.sort(np.concatenate([[700, 900, 40], rng.choice(np.arange(1000, 1200), size=70, replace=False)]))
        with ix.create_filter(ids[a_rows]) as fa, ix.create_filter(ids[b_rows]) as fb:
            Q = np.repeat(rows[300:301], 4, axis=0)
            gid, gsc, gcnt = ix.search_batch_brute_force_with_filters(Q, 5, [fa, fb, fb, fa])
            mode = tf.arith_mode(ix, 5)
            for qi, sel in enumerate((a_rows, b_rows, b_rows, a_rows)):
                exp = tf.oracle_subset(metric, rows, ids, Q[qi:qi + 1], 5, sel, mode)
                tf.assert_equal((gid[qi:qi + 1], gsc[qi:qi + 1], gcnt[qi:qi + 1]), exp, (str(metric), route, qi))
                copies = [int(ids[r]) for r in sorted(set(sel) & {40, 700, 900})]
                pos = {int(v): i for i, v in enumerate(gid[qi])}
                assert [pos[cid] for cid in copies] == list(range(pos[copies[0]], pos[copies[0]] + len(copies))), (qi, gid[qi])
    finally:
        ix.close()


# ---- 5. rows removed after the filters were made drop out of every query; rows inserted later are in no filter -----------------
@pytest.mark.parametrize("route", [va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK])
def test_dead_and_late_rows(gpu_required, route):
    n, dim, k = 1000, 64, 10
    rng = np.random.default_rng(9)
    rows, ids = tf.rand_rows(rng, n + 5, dim, DM.Cosine), tf.ext_ids(n + 5)
    ix = va.HnswIndex(dim, DM.Cosine)
    try:
        ix.upload(ids[:n], rows[:n])
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        mode = tf.arith_mode(ix, k)
        sa = np.sort(rng.choice(n, size=12, replace=False))
        sb = np.sort(np.concatenate([sa[:6], rng.choice(np.setdiff1d(np.arange(n), sa), size=80, replace=False)]))
        fa, fb = ix.create_filter(ids[sa]), ix.create_filter(ids[sb])
        for gone in sa[:3]:
            assert ix.remove(int(ids[gone]))
        ix.upload(ids[n:], rows[n:])
        fq = [0, 1, None, 1, 0, 1, None]
        Q = np.concatenate([tf.rand_rows(rng, 6, dim, DM.Cosine), rows[n:n + 1]])
        gid, gsc, gcnt = ix.search_batch_brute_force_with_filters(Q, k, [None if g is None else (fa, fb)[g] for g in fq])
        live = np.setdiff1d(np.arange(n + 5), sa[:3])
        sels = {0: np.setdiff1d(sa, sa[:3]), 1: np.setdiff1d(sb, sa[:3]), None: live}
        for qi, g in enumerate(fq):
            exp = tf.oracle_subset(DM.Cosine, rows, ids, Q[qi:qi + 1], k, sels[g], mode)
            tf.assert_equal((gid[qi:qi + 1], gsc[qi:qi + 1], gcnt[qi:qi + 1]), exp, (route, qi))
        assert gcnt[0] == 9 and gcnt[4] == 9  # 12 rows, 3 of them dead
        assert gid[6, 0] == ids[n]  # the unfiltered query finds the late row (itself)
        assert not np.isin(ids[n:], gid[[0, 1, 3, 4, 5]]).any()
        fa.close()
        fb.close()
    finally:
        ix.close()


# ---- 6. the number of launches does not follow the number of filters --------------------------------------------------------
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_launch_count_is_constant(gpu_required, metric):
    n, dim, nq, k = 5000, 100, 70, 10
    rng = np.random.default_rng(31 + int(metric))
    rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
    Q = tf.rand_rows(rng, nq, dim, metric)
    ix = va.HnswIndex(dim, metric)
    try:
        ix.upload(ids, rows)
        ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_LISTED)
        filters = [ix.create_filter(ids[np.sort(rng.choice(n, size=20 + 13 * j, replace=False))]) for j in range(35)]
        plans = {}
        for nf in (2, 35):
            table = [filters[i % nf] for i in range(nq)]
            got = ix.search_batch_brute_force_with_filters(Q, k, table)
            plans[nf] = ix.last_filters_exact_plan()
            assert plans[nf][0] == nf and plans[nf][1] == nf and 1 <= plans[nf][4] <= 4, plans[nf]
            assert ix.last_kernels() & va.KERNEL_SWEEP_LISTED_GROUPS and not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
            for i in range(nq):
                one = ix.search_batch_brute_force_filtered(Q[i:i + 1], k, table[i])
                same(tuple(a[i:i + 1] for a in got), one, (str(metric), nf, i))
        assert plans[2][5] == plans[35][5] == 1, plans
        # one filter for the whole call: the one-filter path itself — its kernels, its launches, none of the grouped ones
        one_call = ix.search_batch_brute_force_filtered(Q, k, filters[3])
        want_kernels = ix.last_kernels()
        got = ix.search_batch_brute_force_with_filters(Q, k, [filters[3]] * nq)
        assert ix.last_kernels() == want_kernels and want_kernels & va.KERNEL_SWEEP_LISTED
        plan = ix.last_filters_exact_plan()
        assert plan == (1, 1, 0, 0, 0, 0), plan
        same(got, one_call, (str(metric), "one filter"))
        for f in filters:
            f.close()
    finally:
        ix.close()


# ---- 7. the call leaves the handle's selection state as it found it ------------------------------------------------------------
@pytest.mark.parametrize("metric", tf.FLOATS)
def test_selection_state_is_left_alone(gpu_required, metric):
    """tests/test_gpu_filtered.py::test_mask_route_through_the_selection_stage's scheme: an unfiltered batch runs at the WIDE
    level; a per-query call with dense groups on mask substitution and with unfiltered queries comes between two of them"""
    n, dim, nq, k = 66000, 128, 64, 10
    rng = np.random.default_rng(77 + int(metric))
    rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
    Q = tf.rand_rows(rng, nq, dim, metric)
    ix = va.HnswIndex(dim, metric)
    try:
        assert ix.upload(ids, rows) == n
        before = ix.search_batch_brute_force(Q, k)
        level = ix.last_select_level()
        assert level == 4, level
        half = np.sort(rng.choice(n, size=n // 2, replace=False))
        third = np.sort(rng.choice(n, size=n // 3, replace=False))
        with ix.create_filter(ids[half]) as fh, ix.create_filter(ids[third]) as ft:
            table = [(fh, ft, None)[i % 3] for i in range(nq)]
            got = ix.search_batch_brute_force_with_filters(Q, k, table)
            plan = ix.last_filters_exact_plan()
            assert plan[:4] == (2, 0, 2, len([t for t in table if t is None])), plan
            mode = tf.arith_mode(ix, k)
            for g, sel in ((fh, half), (ft, third), (None, np.arange(n))):
                qi = [i for i, t in enumerate(table) if t is g]
                tf.assert_equal(tuple(a[qi] for a in got), tf.oracle_subset(metric, rows, ids, Q[qi], k, sel, mode), (str(metric), len(sel)))
        after = ix.search_batch_brute_force(Q, k)
        assert ix.last_select_level() == level, "a per-query filtered call moved the handle's selector"
        same(after, before, (str(metric), "unfiltered before and after"))
    finally:
        ix.close()


# ---- 8. refusals: outputs untouched ----------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu_required):
    import ctypes as C
    n, dim, k, nq = 600, 32, 5, 4
    rng = np.random.default_rng(3)
    rows, ids = tf.rand_rows(rng, n, dim, DM.Cosine), tf.ext_ids(n)
    ix, other = va.HnswIndex(dim, DM.Cosine), va.HnswIndex(dim, DM.Cosine)
    L = va._ffi.lib()
    Q = np.ascontiguousarray(rows[:nq])

    def call(handle, table, fq, mode=va.MODE_BRUTE):
        out_ids = np.full((nq, k), 0xA5A5A5A5A5A5A5A5, np.uint64)
        out_sc = np.full((nq, k), 1234.5, np.float32)
        out_n = np.full(nq, 0xDEAD, np.uint32)
        fqa = np.asarray(fq, np.uint32)
        arr = (C.c_void_p * max(len(table), 1))(*table)
        rc = L.vdb_hip_index_search_batch_filters(handle, arr if table else None, len(table), fqa.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p),
                                                  nq, k, mode, out_ids.ctypes.data_as(C.c_void_p), out_sc.ctypes.data_as(C.c_void_p),
                                                  out_n.ctypes.data_as(C.c_void_p))
        untouched = (out_ids == 0xA5A5A5A5A5A5A5A5).all() and (out_sc == 1234.5).all() and (out_n == 0xDEAD).all()
        return rc, untouched

    E = va._ffi
    try:
        ix.upload(ids, rows)
        other.upload(ids, rows)
        f1, f2, foreign = ix.create_filter(ids[:100]), ix.create_filter(ids[50:300]), other.create_filter(ids[:100])
        rc, untouched = call(ix._h, [f1._h, f2._h], [0, 1, 2, 1])
        assert rc == E.VDB_OK and not untouched
        # a filter of another handle — also when no query names it: the whole table is checked before anything runs
        assert call(ix._h, [f1._h, foreign._h], [0, 0, 2, 0]) == (E.VDB_ERR_INVALID_ARG, True)
        assert call(ix._h, [f1._h, None], [0, 0, 2, 0]) == (E.VDB_ERR_INVALID_ARG, True)      # a NULL table entry
        assert call(ix._h, [f1._h, f2._h], [0, 1, 3, 1]) == (E.VDB_ERR_INVALID_ARG, True)     # an index greater than n_filters
        for mode in (va.MODE_HNSW, va.MODE_AUTO, va.MODE_BRUTE_BF16, va.MODE_BRUTE_SQ8):
            assert call(ix._h, [f1._h, f2._h], [0, 1, 2, 1], mode) == (E.VDB_ERR_UNSUPPORTED, True), mode
        assert call(ix._h, [], [0, 0, 0, 0])[0] == E.VDB_OK                                   # no table: every query unfiltered
        ix.remove(int(ids[7]))
        ix.vacuum()                                                                           # the filters are stale now
        assert call(ix._h, [f1._h, f2._h], [0, 1, 2, 1]) == (E.VDB_ERR_STATE, True)
        assert call(ix._h, [f1._h, f2._h], [2, 2, 2, 2]) == (E.VDB_ERR_STATE, True)           # ... whether or not a query names them
        for f in (f1, f2, foreign):
            f.close()
    finally:
        ix.close()
        other.close()
    sh = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    try:
        sh.upload(ids, rows)
        assert call(sh._h, [], [0, 0, 0, 0]) == (E.VDB_ERR_UNSUPPORTED, True)                 # a multi-device handle
    finally:
        sh.close()


# ---- 9. callers --------------------------------------------------------------------------------------------------------------
def test_concurrent_per_query_callers(gpu_required):
    """two threads with different tables on one handle next to an unfiltered caller: each gets what it gets alone"""
    n, dim, k, nq, rounds = 6000, 96, 10, 24, 12
    rng = np.random.default_rng(21)
    rows, ids = tf.rand_rows(rng, n, dim, DM.Cosine), tf.ext_ids(n)
    Q = tf.rand_rows(rng, nq, dim, DM.Cosine)
    ix = va.HnswIndex(dim, DM.Cosine)
    try:
        ix.upload(ids, rows)
        filters = [ix.create_filter(ids[np.sort(rng.choice(n, size=s, replace=False))]) for s in (1, 9, 60, 300, 1500, 3000, 4500, 6000)]
        tables = [[(filters[(i * 3 + t) % 8] if (i + t) % 5 else None) for i in range(nq)] for t in range(2)]
        alone = [ix.search_batch_brute_force_with_filters(Q, k, tb) for tb in tables]
        for tb, res in zip(tables, alone):  # ... and that is the single calls' answer
            for i in (0, 5, 11, 23):
                one = ix.search_batch_brute_force_filtered(Q[i:i + 1], k, tb[i]) if tb[i] is not None else ix.search_batch_brute_force(Q[i:i + 1], k)
                same(tuple(a[i:i + 1] for a in res), one, ("alone", i))
        alone_plain = ix.search_batch_brute_force(Q, k)
        errors = []

        def per_query(t):
            try:
                for r in range(rounds):
                    got = ix.search_batch_brute_force_with_filters(Q, k, tables[t])
                    if not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, alone[t])):
                        errors.append(("per-query", t, r))
            except Exception as ex:  # noqa: BLE001
                errors.append(("per-query", t, repr(ex)))

        def plain():
            try:
                for r in range(rounds):
                    got = ix.search_batch_brute_force(Q, k)
                    if not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, alone_plain)):
                        errors.append(("plain", r))
            except Exception as ex:  # noqa: BLE001
                errors.append(("plain", repr(ex)))

        threads = [threading.Thread(target=per_query, args=(t,)) for t in range(2)] + [threading.Thread(target=plain)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors[:5]
        for f in filters:
            f.close()
    finally:
        ix.close()
