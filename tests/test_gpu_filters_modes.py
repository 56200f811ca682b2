"""One filter per query over the SQ8 codes, the sign bits and the half images (vdb_hip_index_search_batch_filters_mode).

The contract: in SQ8, Binary and Euclidean over a half image query i gets, bit for bit, what the one-filter call of that mode
(vdb_hip_index_search_batch_filtered_mode) returns for it ALONE with its filter and the same k — a query without a filter what the
plain call of that mode returns for it alone —, whatever its companions, its position and VDB_OPT_FILTER_ROUTE are.  Cosine /
DotProduct over a half image: bit for bit what the one-filter call returns for the query's GROUP (the queries that name the same
filter, in call order), within that mode's tolerance of the query alone, bit for bit on data whose partial sums are exact.

Every expected value comes from the oracle over the filter's live rows (tests/test_gpu_filtered_modes.py: sq8_subset,
binary_subset, half_subset) or from the existing one-filter and plain calls; none comes from the call under test.  Expected values
are computed once per case and shared between the routes.  The plan the tests predict is the rule of
velesdb_amd/csrc/vdb_filter_route.hpp (filters_mode_groups / mode_groups_plan), restated below."""
import ctypes as C

import numpy as np
import pytest

import half_ref as hr
import test_gpu_filtered as tf
import test_gpu_filtered_modes as fm
import test_gpu_filters_exact as fx
import test_gpu_half_precision as hp
from test_gpu_storage_modes import special_rows

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
SM = va.StorageMode
VP = va.VectorPrecision
LISTED, MASK, AUTO = va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK, va.FILTER_ROUTE_AUTO
N_CUS = 256  # (the restated plan below only decides whether a pass is cut into several chunks: far from any CU limit at these sizes)


# ---- the plan rule, restated ---------------------------------------------------------------------------------------------------------
def lds_bytes(half, B, k, dim):
    if half:
        return (B * ((dim + 7) // 8 * 8) * 4 + B * k * 8 + B * 8 + 15) & ~15
    return (((dim + 3) & ~3) * B * 4 + 4 * 64 * 80 + B * k * 8 + B * 16 + 15) & ~15


def passes_of(half, nq_g, k, dim):
    """[(B, queries)] of a group of nq_g queries: mode_listed_plan's loop"""
    out, left = [], nq_g
    while left:
        B = (16 if left > 4 else (4 if left > 1 else 1)) if half else (8 if left >= 8 else (4 if left >= 4 else 1))
        while B > 1 and lds_bytes(half, B, k, dim) > 160 * 1024:
            B = B // 4 if half else (4 if B == 8 else 1)
        assert lds_bytes(half, B, k, dim) <= 160 * 1024
        out.append((B, min(B, left)))
        left -= min(B, left)
    return out


def route_of(route, mode, metric, count, n, nq_g):
    """filter_mode_route: True = the listed kernels"""
    half = mode in (va.MODE_BRUTE_F16, va.MODE_BRUTE_BF16)
    has_listed = mode == va.MODE_BRUTE_SQ8 or (half and metric == DM.Euclidean)
    if not has_listed or count == 0 or route == MASK:
        return False
    if route == LISTED:
        return True
    if mode == va.MODE_BRUTE_SQ8 and nq_g > 3:
        return False
    return count * 4 <= n * 3


def predict(route, mode, metric, table, counts, n, k, dim):
    """the six values of last_filters_exact_plan, and the largest number of chunks a pass is cut into"""
    half = mode in (va.MODE_BRUTE_F16, va.MODE_BRUTE_BF16)
    groups = {}
    for g in table:
        groups[g] = groups.get(g, 0) + 1
    n_unf = groups.pop(None, 0)
    listed = [g for g, nq_g in groups.items() if route_of(route, mode, metric, counts[g], n, nq_g)]
    if all(g is not None for g in table) and len(groups) == 1:  # one filter: the one-filter call itself, no grouped launch
        return (1, len(listed), 1 - len(listed), 0, 0, 0), 0
    units = {}
    for g in listed:
        for B, _ in passes_of(half, groups[g], k, dim):
            rpu = 64 // B if half else 64
            units.setdefault(B, []).append((counts[g] + rpu - 1) // rpu)
    chunks = 0
    for B, us in units.items():
        per_cu = min(160 * 1024 // lds_bytes(half, B, k, dim), 3 if half else 4)
        want = max(1, min((sum(us) + 3) // 4, N_CUS * per_cu))
        per_block = (sum(us) + want - 1) // want
        chunks = max(chunks, max((u + per_block - 1) // per_block for u in us))
    return (len(groups), len(listed), len(groups) - len(listed), n_unf, len(units), 1 if listed else 0), chunks


# ---- the modes ---------------------------------------------------------------------------------------------------------------------
class Mode:
    def __init__(self, mode, prec=None):
        self.mode, self.prec = mode, prec

    def enable(self, ix):
        if self.mode == va.MODE_BRUTE_SQ8:
            ix.set_storage_mode(SM.SQ8)
        elif self.mode == va.MODE_BRUTE_BINARY:
            ix.set_storage_mode(SM.Binary)
        else:
            ix.enable_half_precision(fm.vp(self.prec))

    def table_call(self, ix, Q, k, table):
        if self.mode == va.MODE_BRUTE_SQ8:
            return ix.search_batch_with_filters_sq8(Q, k, table)
        if self.mode == va.MODE_BRUTE_BINARY:
            return ix.search_batch_with_filters_binary(Q, k, table)
        return ix.search_batch_brute_force_with_filters_half(Q, k, table, fm.vp(self.prec))

    def one(self, ix, Q, k, flt):
        """the existing calls: one filter (or none) for all of Q"""
        if self.mode == va.MODE_BRUTE_SQ8:
            return ix.search_batch_sq8(Q, k) if flt is None else ix.search_batch_filtered_sq8(Q, k, flt)
        if self.mode == va.MODE_BRUTE_BINARY:
            return ix.search_batch_binary(Q, k) if flt is None else ix.search_batch_filtered_binary(Q, k, flt)
        if flt is None:
            return ix.search_batch_brute_force_half(Q, k, fm.vp(self.prec))
        return ix.search_batch_filtered_half(Q, k, flt, fm.vp(self.prec))


SQ8, BINARY = Mode(va.MODE_BRUTE_SQ8), Mode(va.MODE_BRUTE_BINARY)
F16, BF16 = Mode(va.MODE_BRUTE_F16, hr.F16), Mode(va.MODE_BRUTE_BF16, hr.BF16)


def alone(M, ix, Q, k, table):
    """every query alone through the one-filter call of the mode (or its plain call), route auto"""
    ix.set_option(va.OPT_FILTER_ROUTE, AUTO)
    nq = len(table)
    ids, sc, cnt = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.zeros(nq, np.uint32)
    for i, f in enumerate(table):
        a, b, c = M.one(ix, Q[i:i + 1], k, f)
        ids[i], sc[i], cnt[i] = a[0], b[0], c[0]
    return ids, sc, cnt


def by_group(M, ix, Q, k, table):
    """every group through the one-filter call of the mode over the group's queries in call order (the unfiltered ones: the plain call)"""
    ix.set_option(va.OPT_FILTER_ROUTE, AUTO)
    nq = len(table)
    ids, sc, cnt = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.zeros(nq, np.uint32)
    for f in {id(t): t for t in table}.values():
        qi = [i for i, t in enumerate(table) if t is f]
        a, b, c = M.one(ix, np.ascontiguousarray(Q[qi]), k, f)
        ids[qi], sc[qi], cnt[qi] = a, b, c
    return ids, sc, cnt


def interleave(sizes, seed):
    """group index per query (None = unfiltered): `sizes` = [(group, queries)], shuffled so that no group is contiguous"""
    fq = [g for g, c in sizes for _ in range(c)]
    perm = np.random.default_rng(seed).permutation(len(fq))
    fq = [fq[i] for i in perm]
    blocks = 1 + sum(1 for i in range(1, len(fq)) if fq[i] != fq[i - 1])
    assert blocks > len(sizes) + 2  # interleaved, not sorted
    return fq


def oracle_check(got, table_idx, sels, subset):
    """got against the subset oracle, group by group: subset(Q rows of the group, sel) -> [(ids, scores)]"""
    for g in set(table_idx):
        qi = [i for i, t in enumerate(table_idx) if t == g]
        tf.assert_equal(tuple(a[qi] for a in got), subset(qi, sels[g]), ("oracle", g))


# ---- SQ8 -----------------------------------------------------------------------------------------------------------------------------
SQ8_SHAPES = [(900, 17), (1500, 100), (2000, 768)]
SQ8_KS = (3, 10, 25, 64)
_SQ8 = {}


def sq8_case(metric, n, dim):
    key = (int(metric), n, dim)
    if key not in _SQ8:
        rng = np.random.default_rng(11 * n + dim + int(metric))
        rows, ids = fm.with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
        long_set = fm.mode_sets(rng, n)["not10pct"]
        picks = {c: np.sort(rng.choice(n, size=c, replace=False)).astype(np.int64) for c in (1, 2, 9, 24, 63, 64, 65)}
        picks[66] = np.sort(rng.choice(n, size=63, replace=False)).astype(np.int64)  # (a second list of 63 rows: k - 1 at k = 64)
        Q = rng.standard_normal((23, dim)).astype(np.float32)  # 9 + 7 + five groups of one + 2 unfiltered
        Q[0], Q[1] = rows[n - 1], rows[fm.OUTSIDE]
        _SQ8[key] = dict(rows=rows, ids=ids, long_set=long_set, picks=picks, Q=Q, fq=None)
    return _SQ8[key]


@pytest.mark.parametrize("k", SQ8_KS)
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
@pytest.mark.parametrize("n,dim", SQ8_SHAPES)
def test_sq8_mixed_table_bit_exact(gpu_required, metric, n, dim, k):
    """groups of 9, 7 and 1 queries (pass widths 8 + 1, 4 + 1 + 1 + 1, 1: all three grouped launches in one call), lists of 65, 63,
    1, 64 and k - 1 rows, the negated 10 % set (long: its 8-query pass is cut into several chunks), one empty filter, two
    unfiltered queries; filter_of_query interleaved"""
    c = sq8_case(metric, n, dim)
    rows, ids, Q = c["rows"], c["ids"], c["Q"]
    km1 = {3: 2, 10: 9, 25: 24, 64: 66}[k]
    excl, _, long_sel = c["long_set"]
    sels = [long_sel, c["picks"][65], c["picks"][63], c["picks"][1], c["picks"][64], c["picks"][km1], np.empty(0, np.int64)]
    assert [len(s) for s in sels[1:5]] == [65, 63, 1, 64] and len(sels[5]) == k - 1
    sizes = [(0, 9), (1, 7), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (None, 2)]
    fq = interleave(sizes, 5)
    assert len(fq) == Q.shape[0]
    ix = va.HnswIndex(dim, metric)
    filters = []
    try:
        ix.set_storage_mode(SM.SQ8)
        assert ix.upload(ids, rows) == n
        filters = [ix.create_filter(ids[excl], negate=True)] + [ix.create_filter(ids[s]) for s in sels[1:]]
        assert [f.matched for f in filters] == [len(s) for s in sels]
        table = [None if g is None else filters[g] for g in fq]
        exp = alone(SQ8, ix, Q, k, table)
        all_rows = np.arange(n, dtype=np.int64)
        subset = lambda qi, sel: fm.sq8_subset(metric, rows, ids, Q[qi], k, sel)  # noqa: E731
        oracle_check(exp, fq, {**dict(enumerate(sels)), None: all_rows}, subset)   # (the reference calls themselves, once)
        counts = {f: len(s) for f, s in zip(filters, sels)}
        for route in (LISTED, MASK, AUTO):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = ix.search_batch_with_filters_sq8(Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            want, chunks = predict(route, va.MODE_BRUTE_SQ8, metric, table, counts, n, k, dim)
            assert plan == want, (route, plan, want)
            if route == LISTED:
                assert plan == (7, 6, 1, 2, 3, 1) and chunks > 1, (plan, chunks)
            elif route == AUTO:
                assert plan == (7, 4, 3, 2, 1, 1), plan   # (auto: an SQ8 group goes listed only with at most three queries)
            else:
                assert plan == (7, 0, 7, 2, 0, 0), plan
            assert bool(m & va.KERNEL_SWEEP_LISTED_GROUPS) == (plan[4] > 0) and m & va.KERNEL_SQ8 and not m & va.KERNEL_SWEEP_LISTED, hex(m)
            fx.same(got, exp, (str(metric), n, dim, k, route))
            oracle_check(got, fq, {**dict(enumerate(sels)), None: all_rows}, subset)
    finally:
        for f in filters:
            f.close()
        ix.close()


# ---- Euclidean over a half image -----------------------------------------------------------------------------------------------------
HALF_SHAPES = [(700, 17), (1200, 100), (2000, 768)]
# groups of 17, 5 and 1 queries — and one of 3: the pass rule (mode_listed_plan) takes the 16-query kernel from FIVE queries up, so 17
# runs as 16 + 1 and 5 as one 16-wide pass; the 4-wide kernel serves two to four queries, hence the group of 3
HALF_SIZES = [("not10pct", 17), ("half", 5), ("k", 3), ("1pct", 1), ("one", 1), ("empty", 1), (None, 2)]


def half_world(metric, M, rows, ids, sets):
    ix = fm.half_index(metric, M.prec, ids, rows)
    filters = {name: ix.create_filter(ids[given], negate=neg) for name, (given, neg, _) in sets.items()}
    return ix, filters


def half_sets(rng, n):
    sets = tf.allowed_sets(rng, n)
    sets["empty"] = (np.empty(0, np.int64), False, np.empty(0, np.int64))
    return sets


@pytest.mark.parametrize("M", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n,dim", HALF_SHAPES)
def test_half_euclidean_exact_data_bit_equal_on_both_routes(gpu_required, M, n, dim):
    k = 10
    rng = np.random.default_rng(37 * n + dim + M.prec)
    rows, ids = hp.ints(rng, (n, dim)), tf.ext_ids(n)
    rows[[5, n - 2]] = 0.0
    rows[[256, 257]] = rows[[1, 1]]
    sets = half_sets(rng, n)
    fq = interleave(HALF_SIZES, 9)
    Q = hp.ints(rng, (len(fq), dim))
    Q[0] = rows[n - 1]
    ix, filters = half_world(hr.EUCLIDEAN, M, rows, ids, sets)
    try:
        table = [None if g is None else filters[g] for g in fq]
        exp = alone(M, ix, Q, k, table)
        sels = {name: s[2] for name, s in sets.items()}
        sels[None] = np.arange(n, dtype=np.int64)
        subset = lambda qi, sel: fm.half_subset(hr.EUCLIDEAN, M.prec, rows, ids, Q[qi], k, sel)  # noqa: E731
        counts = {filters[name]: len(sels[name]) for name in filters}
        for route in (LISTED, MASK):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = M.table_call(ix, Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            want, chunks = predict(route, M.mode, DM.Euclidean, table, counts, n, k, dim)
            assert plan == want == ((6, 5, 1, 2, 3, 1) if route == LISTED else (6, 0, 6, 2, 0, 0)), (route, plan, want)
            assert route == MASK or chunks > 1
            assert m & va.KERNEL_SWEEP_HALF_L2 and bool(m & va.KERNEL_SWEEP_LISTED_GROUPS) == (route == LISTED) and not m & va.KERNEL_SWEEP_LISTED, hex(m)
            fx.same(got, exp, (M.prec, n, dim, route))
            oracle_check(got, fq, sels, subset)
    finally:
        for f in filters.values():
            f.close()
        ix.close()


def test_half_euclidean_gaussian_routes_agree_within_tol(gpu_required):
    n, dim, k, M = 1200, 100, 10, F16
    rng = np.random.default_rng(53)
    rows, ids = rng.standard_normal((n, dim)).astype(np.float32), np.arange(n, dtype=np.uint64)
    sets = half_sets(rng, n)
    fq = interleave(HALF_SIZES, 9)
    Q = rng.standard_normal((len(fq), dim)).astype(np.float32)
    ix, filters = half_world(hr.EUCLIDEAN, M, rows, ids, sets)
    try:
        table = [None if g is None else filters[g] for g in fq]
        exp = alone(M, ix, Q, k, table)
        ix.set_option(va.OPT_FILTER_ROUTE, LISTED)
        li = M.table_call(ix, Q, k, table)
        assert ix.last_kernels() & va.KERNEL_SWEEP_LISTED_GROUPS
        ix.set_option(va.OPT_FILTER_ROUTE, MASK)
        mi = M.table_call(ix, Q, k, table)
        assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED_GROUPS
        fx.same(li, mi, "listed against mask")
        fx.same(li, exp, "listed against the queries alone")
        for name, _ in HALF_SIZES:
            sel = np.arange(n) if name is None else sets[name][2]
            qi = [i for i, g in enumerate(fq) if g == name]
            if len(sel):
                gi, gs, gc = (a[qi] for a in li)
                hp.check(hr.EUCLIDEAN, M.prec, rows[sel], Q[qi], k, fm.positions(sel, gi, gc), gs, gc)
    finally:
        for f in filters.values():
            f.close()
        ix.close()


# ---- Binary ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(900, 17), (2000, 768)])
def test_binary_mixed_table_exact(gpu_required, n, dim):
    k = 12
    rng = np.random.default_rng(n + 3 * dim)
    rows, ids = fm.with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
    rows[50:80] = rows[49]                     # thirty equal codes: heavy ties at rank k, broken by row
    sets = half_sets(rng, n)
    fq = interleave([("not10pct", 6), ("half", 2), ("k-1", 1), ("empty", 1), (None, 2)], 3)
    Q = rng.standard_normal((len(fq), dim)).astype(np.float32)
    Q[0] = rows[49]
    ix = va.HnswIndex(dim, DM.Euclidean)
    filters = {}
    try:
        ix.upload(ids, rows)
        ix.set_storage_mode(SM.Binary)
        filters = {name: ix.create_filter(ids[given], negate=neg) for name, (given, neg, _) in sets.items()}
        table = [None if g is None else filters[g] for g in fq]
        exp = alone(BINARY, ix, Q, k, table)
        sels = {name: s[2] for name, s in sets.items()}
        sels[None] = np.arange(n, dtype=np.int64)
        for route in (AUTO, LISTED, MASK):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = ix.search_batch_with_filters_binary(Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            assert plan == (4, 0, 4, 2, 0, 0), (route, plan)   # no listed kernel for this mode: every group on mask substitution
            assert m & va.KERNEL_BITS and not m & (va.KERNEL_SWEEP_LISTED_GROUPS | va.KERNEL_SWEEP_LISTED), hex(m)
            fx.same(got, exp, (n, dim, route))
            oracle_check(got, fq, sels, lambda qi, sel: fm.binary_subset(rows, ids, Q[qi], k, sel))
    finally:
        for f in filters.values():
            f.close()
        ix.close()


# ---- Cosine / DotProduct over a half image -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,metric", [(F16, hr.COSINE), (F16, hr.DOT), (BF16, hr.COSINE), (BF16, hr.DOT)], ids=["f16-cos", "f16-dot", "bf16-cos", "bf16-dot"])
@pytest.mark.parametrize("data", ["ints", "gauss"])
def test_half_cosine_dot_per_group(gpu_required, M, metric, data):
    """exact-sum data: bit for bit the subset oracle; Gaussian data: bit for bit the one-filter call over each group's queries in call
    order, and within the mode's TOL (tie-aware) of the reference scan"""
    n, dim, k = 1200, 100, 10
    rng = np.random.default_rng(71 + 5 * M.prec + metric + len(data))
    make = (lambda shape: hp.ints(rng, shape)) if data == "ints" else (lambda shape: rng.standard_normal(shape).astype(np.float32))
    rows = make((n, dim))
    ids = tf.ext_ids(n) if data == "ints" else np.arange(n, dtype=np.uint64)
    sets = half_sets(rng, n)
    fq = interleave(HALF_SIZES, 9)
    Q = make((len(fq), dim))
    ix, filters = half_world(metric, M, rows, ids, sets)
    try:
        table = [None if g is None else filters[g] for g in fq]
        exp = by_group(M, ix, Q, k, table)
        sels = {name: s[2] for name, s in sets.items()}
        sels[None] = np.arange(n, dtype=np.int64)
        for route in (AUTO, LISTED):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = M.table_call(ix, Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            assert plan == (6, 0, 6, 2, 0, 0), (route, plan)   # no listed kernel for these metrics
            assert not m & (va.KERNEL_SWEEP_LISTED_GROUPS | va.KERNEL_SWEEP_LISTED), hex(m)
            fx.same(got, exp, (M.prec, metric, data, route))
            if data == "ints":
                oracle_check(got, fq, sels, lambda qi, sel: fm.half_subset(metric, M.prec, rows, ids, Q[qi], k, sel))
            else:
                for name in sels:
                    qi = [i for i, g in enumerate(fq) if g == name]
                    if len(sels[name]):
                        gi, gs, gc = (a[qi] for a in got)
                        hp.check(metric, M.prec, rows[sels[name]], Q[qi], k, fm.positions(sels[name], gi, gc), gs, gc)
    finally:
        for f in filters.values():
            f.close()
        ix.close()


# ---- rules that cut across the modes ---------------------------------------------------------------------------------------------------
CROSS = [(SQ8, DM.Cosine, 64, (LISTED, AUTO, MASK)), (BINARY, DM.Euclidean, 48, (AUTO,)), (F16, DM.Euclidean, 40, (LISTED, MASK)),
         (BF16, DM.DotProduct, 64, (AUTO,))]
CROSS_IDS = ["sq8", "binary", "f16-l2", "bf16-dot"]


def cross_world(M, metric, dim, n, seed):
    rng = np.random.default_rng(seed + M.mode)
    half = M.prec is not None
    rows = hp.ints(rng, (n, dim)) if half else rng.standard_normal((n, dim)).astype(np.float32)
    ids = tf.ext_ids(n)
    ix = va.HnswIndex(dim, metric)
    ix.upload(ids, rows)
    M.enable(ix)
    return rng, rows, ids, ix


@pytest.mark.parametrize("M,metric,dim,routes", CROSS, ids=CROSS_IDS)
def test_answers_do_not_depend_on_companions_or_position(gpu_required, M, metric, dim, routes):
    """the table permuted, and every companion replaced: a query's answer does not move.  Half Cosine / DotProduct: the group is kept
    whole and in call order (the permutation moves whole tables, the replacement leaves the probe's group alone)"""
    n, k = 1500, 10
    rng, rows, ids, ix = cross_world(M, metric, dim, n, 5)
    grouped_bits = M.prec is not None and metric != DM.Euclidean
    filters = []
    try:
        sels = [np.sort(rng.choice(n, size=c, replace=False)) for c in (1200, 300, 70, 9)]
        filters = [ix.create_filter(ids[s]) for s in sels]
        fq = interleave([(0, 9), (1, 5), (2, 3), (3, 1), (None, 2)], 17)
        nq = len(fq)
        Q = (hp.ints(rng, (nq, dim)) if M.prec is not None else rng.standard_normal((nq, dim)).astype(np.float32))
        table = [None if g is None else filters[g] for g in fq]
        for route in routes:
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            base = M.table_call(ix, Q, k, table)
            # 1. a permutation of the call (stable inside every group where the group is the unit of the contract)
            perm = np.array(sorted(range(nq), key=lambda i: (str(fq[i]), i))) if grouped_bits else rng.permutation(nq)
            got = M.table_call(ix, np.ascontiguousarray(Q[perm]), k, [table[i] for i in perm])
            fx.same(got, tuple(a[perm] for a in base), (route, "permuted"))
            # 2. the queries of group 1 stay, everything else is replaced: other vectors, and the other groups trade filters
            keep = [i for i, g in enumerate(fq) if g == 1]
            Q2 = (hp.ints(rng, (nq, dim)) if M.prec is not None else rng.standard_normal((nq, dim)).astype(np.float32))
            Q2[keep] = Q[keep]
            swap = {0: 2, 2: 0, 3: None, None: 3, 1: 1}
            table2 = [None if swap[g] is None else filters[swap[g]] for g in fq]
            got2 = M.table_call(ix, Q2, k, table2)
            fx.same(tuple(a[keep] for a in got2), tuple(a[keep] for a in base), (route, "companions replaced"))
    finally:
        for f in filters:
            f.close()
        ix.close()


@pytest.mark.parametrize("M,metric,dim,routes", CROSS, ids=CROSS_IDS)
def test_one_filter_is_the_one_filter_call(gpu_required, M, metric, dim, routes):
    n, k, nq = 1500, 10, 5
    rng, rows, ids, ix = cross_world(M, metric, dim, n, 6)
    try:
        Q = (hp.ints(rng, (nq, dim)) if M.prec is not None else rng.standard_normal((nq, dim)).astype(np.float32))
        with ix.create_filter(ids[np.sort(rng.choice(n, size=200, replace=False))]) as flt:
            for route in routes:
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                exp = M.one(ix, Q, k, flt)
                kernels = ix.last_kernels()
                got = M.table_call(ix, Q, k, [flt] * nq)
                listed = 1 if kernels & va.KERNEL_SWEEP_LISTED else 0
                assert ix.last_kernels() == kernels and not kernels & va.KERNEL_SWEEP_LISTED_GROUPS, (hex(kernels), hex(ix.last_kernels()))
                assert ix.last_filters_exact_plan() == (1, listed, 1 - listed, 0, 0, 0)
                assert listed == route_of(route, M.mode, metric, 200, n, nq)
                fx.same(got, exp, (route, "one filter"))
    finally:
        ix.close()


@pytest.mark.parametrize("M,metric,dim,routes", CROSS, ids=CROSS_IDS)
def test_snapshot_semantics(gpu_required, M, metric, dim, routes):
    """a row removed after create_filter is excluded from every query; rows inserted later are in no filter"""
    n, k = 1000, 10
    rng, rows, ids, ix = cross_world(M, metric, dim, n, 7)
    filters = []
    try:
        sels = [np.sort(rng.choice(n, size=c, replace=False)) for c in (400, 30)]
        filters = [ix.create_filter(ids[s]) for s in sels]
        gone = [int(sels[0][0]), int(sels[0][7]), int(sels[1][3])]
        for r in gone:
            assert ix.remove(int(ids[r]))
        fq = [0, 1, None, 0, 1, 0, 0, 0, 0]
        Q = (hp.ints(rng, (len(fq), dim)) if M.prec is not None else rng.standard_normal((len(fq), dim)).astype(np.float32))
        table = [None if g is None else filters[g] for g in fq]
        live = [np.setdiff1d(s, gone) for s in sels] + [np.setdiff1d(np.arange(n), gone)]
        exp = by_group(M, ix, Q, k, table)
        for route in routes:
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = M.table_call(ix, Q, k, table)
            fx.same(got, exp, (route, "after removals"))
            for i, g in enumerate(fq):
                sel = live[2 if g is None else g]
                assert got[2][i] == k and np.isin(got[0][i], ids[sel]).all(), (route, i)
    finally:
        for f in filters:
            f.close()
        ix.close()


def raw_call(ix_h, table, fq, mode, Q, k):
    """the C entry point with sentinel-filled outputs: (status, outputs untouched?)"""
    L = va._ffi.lib()
    nq = Q.shape[0]
    oi, osc, on = np.full((nq, k), 0xABCDEF, np.uint64), np.full((nq, k), -77.0, np.float32), np.full(nq, 0xFEED, np.uint32)
    fqa = np.asarray(fq, np.uint32)
    arr = (C.c_void_p * max(len(table), 1))(*table)
    rc = L.vdb_hip_index_search_batch_filters_mode(ix_h, arr if table else None, len(table), fqa.ctypes.data_as(C.c_void_p), mode,
                                                   Q.ctypes.data_as(C.c_void_p), nq, k, oi.ctypes.data_as(C.c_void_p),
                                                   osc.ctypes.data_as(C.c_void_p), on.ctypes.data_as(C.c_void_p))
    return rc, bool(np.all(oi == 0xABCDEF) and np.all(osc == -77.0) and np.all(on == 0xFEED))


@pytest.mark.parametrize("M,metric,dim,routes", CROSS, ids=CROSS_IDS)
def test_refusals_leave_the_outputs_untouched(gpu_required, M, metric, dim, routes):
    n, k, nq = 600, 5, 4
    rng = np.random.default_rng(3 + M.mode)
    half = M.prec is not None
    rows = hp.ints(rng, (n, dim)) if half else rng.standard_normal((n, dim)).astype(np.float32)
    ids = tf.ext_ids(n)
    Q = np.ascontiguousarray(rows[:nq])
    ix, other, bare = va.HnswIndex(dim, metric), va.HnswIndex(dim, metric), va.HnswIndex(dim, metric)
    E = va._ffi
    try:
        for h in (ix, other, bare):
            h.upload(ids, rows)
        M.enable(ix)
        M.enable(other)
        f1, f2, foreign = ix.create_filter(ids[:100]), ix.create_filter(ids[50:300]), other.create_filter(ids[:100])
        fb, fe = bare.create_filter(ids[:100]), bare.create_filter(np.empty(0, np.uint64))
        rc, untouched = raw_call(ix._h, [f1._h, f2._h], [0, 1, 2, 1], M.mode, Q, k)
        assert rc == E.VDB_OK and not untouched
        assert raw_call(ix._h, [], [0, 0, 0, 0], M.mode, Q, k)[0] == E.VDB_OK                       # no table: every query unfiltered
        # the table's errors: every filter is checked before anything runs, whether or not a query names it
        assert raw_call(ix._h, [f1._h, foreign._h], [0, 0, 2, 0], M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
        assert raw_call(ix._h, [f1._h, None], [0, 0, 2, 0], M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
        assert raw_call(ix._h, [f1._h, f2._h], [0, 1, 3, 1], M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
        assert raw_call(None, [f1._h, f2._h], [0, 1, 2, 1], M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
        # the mode's: VDB_SEARCH_BRUTE has the call of DESIGN 4.1n, the graph modes theirs
        for bad in (va.MODE_BRUTE, va.MODE_HNSW, va.MODE_AUTO, va.MODE_HNSW_INT8, va.MODE_HNSW_F16, va.MODE_HNSW_BF16, 77):
            assert raw_call(ix._h, [f1._h, f2._h], [0, 1, 2, 1], bad, Q, k) == (E.VDB_ERR_UNSUPPORTED, True), bad
        # the state's: the mode's storage mode / image is not enabled — checked before an empty filter's out_n = 0, with and without filters
        assert raw_call(bare._h, [fb._h, fe._h], [0, 1, 2, 1], M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        assert raw_call(bare._h, [fe._h], [0, 0, 0, 0], M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        assert raw_call(bare._h, [], [0, 0, 0, 0], M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        ix.remove(int(ids[7]))
        ix.vacuum()                                                                                 # the filters are stale now
        assert raw_call(ix._h, [f1._h, f2._h], [0, 1, 2, 1], M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        assert raw_call(ix._h, [f1._h, f2._h], [2, 2, 2, 2], M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        for f in (f1, f2, foreign, fb, fe):
            f.close()
    finally:
        for h in (ix, other, bare):
            h.close()
    sh = va.HnswIndex(dim, metric, va.HnswParams(8, 50, n), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    try:
        sh.upload(ids, rows)
        assert raw_call(sh._h, [], [0, 0, 0, 0], M.mode, Q, k) == (E.VDB_ERR_UNSUPPORTED, True)     # a multi-device handle
    finally:
        sh.close()


@pytest.mark.parametrize("k,selector,level", [(10, 2, 3), (50, -1, 4)])
def test_selection_state_is_left_alone(gpu_required, k, selector, level):
    """tests/test_gpu_filtered_modes.py::test_sq8_mask_route_through_the_selection_stage's scheme (the smallest corpus and batch at
    which the SQ8 selection stage runs): an unfiltered batch takes the stage; a per-query call with a dense group on mask
    substitution (which keeps the stage), a sparse one and an unfiltered job of six queries comes between two of them — the hold
    counters and the verdict sequence it leaves decide the level and the bits of the batch behind it"""
    n, dim, nq = 65_600, 128, 6
    rng = np.random.default_rng(n + k)
    rows, ids = rng.standard_normal((n, dim)).astype(np.float32), tf.ext_ids(n)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n))
    try:
        ix.set_storage_mode(SM.SQ8)
        ix.upload(ids, rows)
        ix.set_option(va.OPT_SELECTOR_LEVEL, selector)
        before = ix.search_batch_sq8(Q, k)
        assert ix.last_select_level() == level, "the unfiltered batch does not take the stage at this size"
        half, few = np.sort(rng.choice(n, size=n // 2, replace=False)), np.sort(rng.choice(n, size=500, replace=False))
        with ix.create_filter(ids[half]) as fh, ix.create_filter(ids[few]) as ff:
            table = [fh] * nq + [None] * nq + [ff] * nq
            Q3 = np.ascontiguousarray(np.concatenate([Q, Q, Q]))
            for route in (AUTO, MASK, LISTED):
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                got = ix.search_batch_with_filters_sq8(Q3, k, table)
                fx.same(tuple(a[nq:2 * nq] for a in got), before, (route, "the unfiltered job"))
                tf.assert_equal(tuple(a[:2] for a in got), fm.sq8_subset(DM.Cosine, rows, ids, Q[:2], k, half), (route, "half"))
                tf.assert_equal(tuple(a[2 * nq:2 * nq + 2] for a in got), fm.sq8_subset(DM.Cosine, rows, ids, Q[:2], k, few), (route, "few"))
                after = ix.search_batch_sq8(Q, k)
                assert ix.last_select_level() == level, (route, ix.last_select_level())
                fx.same(after, before, (route, "unfiltered before and after"))
    finally:
        ix.close()
