"""Filtered exact search over the SQ8 codes, the sign bits and the half images (vdb_hip_index_search_batch_filtered_mode).

The contract: the call returns what the plain search in that mode returns on an index that holds only the filter's live rows,
inserted in the same order under the same ids.  The expected answer is always an independent CPU scan over the subset rows[sel]
with the ids mapped back through sel (the pattern of tests/test_gpu_filtered.py::oracle_subset): po.scan_topk_sq8 for SQ8,
po.scan_topk_binary for Binary, tests/half_ref.py::scan_topk for the half images.  SQ8, Binary and Euclidean over a half image are
compared bit for bit on both routes; Cosine / DotProduct over a half image bit for bit on data whose partial sums are exact and
with tests/test_gpu_half_precision.py's `check` (its TOL, tie-aware) on Gaussian data.  References are computed once per case and
shared."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_ref as hr  # noqa: E402
import test_gpu_filtered as tf  # noqa: E402
import test_gpu_half_precision as hp  # noqa: E402
from test_gpu_storage_modes import special_rows  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
SM = va.StorageMode
VP = va.VectorPrecision
PM = {DM.Cosine: po.COSINE, DM.Euclidean: po.EUCLIDEAN, DM.DotProduct: po.DOT}
LISTED, MASK, AUTO = va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK, va.FILTER_ROUTE_AUTO
SPECIAL = np.array([3, 7, 10, 11, 13])     # special_rows: constant row, zero row, duplicate pair, a -0.0
COPIES = SPECIAL + 20                       # the same rows once more: these stay OUTSIDE the large filters
OUTSIDE = 40                                # an ordinary row that stays outside them as well (one query equals it)


def mode_sets(rng, n):
    """tests/test_gpu_filtered.py::allowed_sets, with the large sets ("1pct", "half", the negated 10 %) holding every special row
    and none of its copies nor row OUTSIDE"""
    sets = tf.allowed_sets(rng, n)
    out_rows = np.concatenate([COPIES, [OUTSIDE]])
    for name in ("1pct", "half"):
        sel = np.union1d(np.setdiff1d(sets[name][2], out_rows), SPECIAL).astype(np.int64)
        if len(sel) % 64 == 0:                 # list lengths are no multiple of the 64-row group: one more ordinary row leaves
            sel = np.setdiff1d(sel, sel[(sel > OUTSIDE) & (sel < n - 1)][:1])
        sets[name] = (sel, False, sel)
    excl = np.union1d(np.setdiff1d(sets["not10pct"][0], SPECIAL), out_rows).astype(np.int64)
    if (n - len(excl)) % 64 == 0:
        allowed = np.setdiff1d(np.arange(n, dtype=np.int64), excl)
        excl = np.union1d(excl, allowed[(allowed > OUTSIDE) & (allowed < n - 1)][:1])
    sets["not10pct"] = (excl, True, np.setdiff1d(np.arange(n, dtype=np.int64), excl))
    assert all(len(sets[name][2]) % 64 for name in ("1pct", "half", "not10pct"))
    return sets


def with_copies(rows):
    rows[COPIES] = rows[SPECIAL]
    return rows


def subset_answer(scan, ids, nq, k, sel):
    """[(ids, scores)] per query from scan(rows_subset_index_array, n) -> (rows, scores) over the subset"""
    n = min(k, len(sel))
    if n == 0:
        return [(np.empty(0, np.uint64), np.empty(0, np.float32)) for _ in range(nq)]
    r, s = scan(n)
    return [(ids[sel[r[qi, :n].astype(np.int64)]], s[qi, :n]) for qi in range(nq)]


def sq8_subset(metric, rows, ids, Q, k, sel):
    return subset_answer(lambda n: po.scan_topk_sq8(PM[metric], rows[sel], Q, n, nthreads=po.host_threads()), ids, Q.shape[0], k, sel)


def binary_subset(rows, ids, Q, k, sel):
    return subset_answer(lambda n: po.scan_topk_binary(rows[sel], Q, n), ids, Q.shape[0], k, sel)


def half_subset(metric, prec, rows, ids, Q, k, sel):
    return subset_answer(lambda n: hr.scan_topk(metric, prec, rows[sel], Q, n)[:2], ids, Q.shape[0], k, sel)


def auto_is_listed(mode, metric, count, n, nq):
    """the stated auto rule (csrc/vdb_filter_route.hpp filter_mode_route), restated"""
    if count == 0 or (mode == va.MODE_BRUTE_SQ8 and nq > 3):
        return False
    return count * 4 <= n * 3


# ---- SQ8: bit for bit, both forced routes and auto ---------------------------------------------------------------------------------
SQ8_SHAPES = [(2000, 768), (1500, 100), (900, 17), (1500, 66)]  # twelve full 64-code chunks; a 36-code tail chunk; a partial word; a chunk + 2
SQ8_NQ_K = [(1, 10), (4, 10), (7, 3), (9, 25), (17, 5), (3, 64)]  # passes 1; 4; 4+1+1+1; 8+1; 8+8+1; k above most set sizes
_SQ8 = {}


def sq8_case(metric, n, dim):
    key = (int(metric), n, dim)
    if key not in _SQ8:
        rng = np.random.default_rng(7 * n + dim + int(metric))
        rows, ids = with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
        sets = mode_sets(rng, n)
        qs = {}
        for nq, k in SQ8_NQ_K:
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
            Q[0] = rows[n - 1]                # an allowed row of every set
            if nq > 1:
                Q[1] = rows[OUTSIDE]          # a row the large sets leave out
            qs[(nq, k)] = Q
        exp = {(name, nq, k): sq8_subset(metric, rows, ids, qs[(nq, k)], k, sets[name][2]) for name in sets for nq, k in SQ8_NQ_K}
        _SQ8[key] = dict(rows=rows, ids=ids, sets=sets, qs=qs, exp=exp)
    return _SQ8[key]


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
@pytest.mark.parametrize("n,dim", SQ8_SHAPES)
def test_sq8_routes_bit_exact(gpu_required, metric, n, dim):
    c = sq8_case(metric, n, dim)
    ix = va.HnswIndex(dim, metric)
    try:
        ix.set_storage_mode(SM.SQ8)
        assert ix.upload(c["ids"], c["rows"]) == n
        for name, (given, negate, sel) in c["sets"].items():
            assert len(sel) % 64 != 0 or name == "all", (name, len(sel))
            with ix.create_filter(c["ids"][given], negate=negate) as flt:
                assert flt.matched == len(sel), name
                for route in (LISTED, MASK, AUTO):
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    for nq, k in SQ8_NQ_K:
                        got = ix.search_batch_filtered_sq8(c["qs"][(nq, k)], k, flt)
                        m = ix.last_kernels()
                        want = route == LISTED or (route == AUTO and auto_is_listed(va.MODE_BRUTE_SQ8, metric, len(sel), n, nq))
                        assert bool(m & va.KERNEL_SWEEP_LISTED) == want, (name, route, nq, k, hex(m))
                        assert m & va.KERNEL_SQ8, hex(m)
                        tf.assert_equal(got, c["exp"][(name, nq, k)], (str(metric), n, dim, name, route, nq, k))
    finally:
        ix.close()


# ---- SQ8 under mask substitution through the selection stage (level 3, WIDE) -----------------------------------------------------
# select_level_sq8 / select_level_wide: dim % 64 == 0 and >= 128, n_rows >= 65 536, >= 6 queries; k <= 10 takes level 3 with the
# selector at 2, 10 < k <= 128 the WIDE selection.  These are the smallest n and nq at which the stage runs.
@pytest.mark.parametrize("k,selector,level", [(10, 2, 3), (50, -1, 4)])
def test_sq8_mask_route_through_the_selection_stage(gpu_required, k, selector, level):
    n, dim, nq = 65_600, 128, 6
    rng = np.random.default_rng(n + k)
    rows, ids = with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
    sets = mode_sets(rng, n)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n))
    try:
        ix.set_storage_mode(SM.SQ8)
        ix.upload(ids, rows)
        ix.set_option(va.OPT_SELECTOR_LEVEL, selector)
        ix.set_option(va.OPT_FILTER_ROUTE, MASK)
        before = ix.search_batch_sq8(Q, k)
        assert ix.last_select_level() == level, "the unfiltered batch does not take the stage at this size"
        for name, want_stage in (("half", True), ("not10pct", True), ("1pct", False)):
            given, negate, sel = sets[name]
            with ix.create_filter(ids[given], negate=negate) as flt:
                got = ix.search_batch_filtered_sq8(Q, k, flt)
                assert (ix.last_select_level() == level) == want_stage, (name, ix.last_select_level())
                if not want_stage:
                    assert ix.last_select_level() == 0 and ix.last_kernels() & va.KERNEL_SQ8
                assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                tf.assert_equal(got, sq8_subset(DM.Cosine, rows, ids, Q, k, sel), (name, k))
            # state left as found: the unfiltered batch behind each filtered call takes the stage again and returns what it returned
            after = ix.search_batch_sq8(Q, k)
            assert ix.last_select_level() == level, (name, ix.last_select_level())
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), name
    finally:
        ix.close()


# ---- Binary: exact integers, mask substitution ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(2500, 768), (600, 17), (300, 33)])
def test_binary_mask_route_exact(gpu_required, n, dim):
    rng = np.random.default_rng(n + 7 * dim)
    rows, ids = with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
    rows[50:80] = rows[49]                     # thirty equal codes: heavy ties at rank k, broken by row
    sets = mode_sets(rng, n)
    k = 12
    ix = va.HnswIndex(dim, DM.Euclidean)
    try:
        ix.upload(ids, rows)
        ix.set_storage_mode(SM.Binary)
        for nq in (1, 2, 6):                   # one or two queries: the one-launch kernel; six: the planned sweep
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
            Q[0] = rows[49]
            for name, (given, negate, sel) in sets.items():
                with ix.create_filter(ids[given], negate=negate) as flt:
                    for route in (AUTO, LISTED):  # (no listed kernel for this mode: both run mask substitution)
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        got = ix.search_batch_filtered_binary(Q, k, flt)
                        m = ix.last_kernels()
                        assert m & va.KERNEL_BITS and not m & va.KERNEL_SWEEP_LISTED and not m & va.KERNEL_BITS_GEMM, hex(m)
                        tf.assert_equal(got, binary_subset(rows, ids, Q, k, sel), (n, dim, nq, name, route))
    finally:
        ix.close()


def test_binary_mask_route_on_the_bit_gemm(gpu_required):
    """bits_gemm_chunk: k <= 10, n_rows >= 65 536, >= 32 queries — the smallest batch that takes the four-bit GEMM"""
    n, dim, nq, k = 65_600, 64, 32, 10
    rng = np.random.default_rng(n + dim)
    rows, ids = with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
    rows[1000:1030] = rows[999]
    sets = mode_sets(rng, n)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q[1] = rows[999]
    ix = va.HnswIndex(dim, DM.Cosine, va.HnswParams(8, 50, n))
    try:
        ix.upload(ids, rows)
        ix.set_storage_mode(SM.Binary)
        for name in ("one", "k-1", "1pct", "half", "not10pct"):
            given, negate, sel = sets[name]
            with ix.create_filter(ids[given], negate=negate) as flt:
                got = ix.search_batch_filtered_binary(Q, k, flt)
                assert ix.last_kernels() & va.KERNEL_BITS_GEMM, "the matrix-core path did not serve the batch"
                tf.assert_equal(got, binary_subset(rows, ids, Q, k, sel), name)
    finally:
        ix.close()


# ---- half images ------------------------------------------------------------------------------------------------------------------------
HALF_SHAPES = [(2000, 768), (1200, 100), (700, 17), (600, 1024)]  # stride 104 at dim 100; a partial chunk at 17; two chunks per lane at 1024
HALF_NQ_K = [(1, 10), (4, 10), (5, 3), (16, 10), (17, 5), (70, 10)]
HMETRIC = {hr.COSINE: DM.Cosine, hr.DOT: DM.DotProduct, hr.EUCLIDEAN: DM.Euclidean}


def vp(prec):
    return VP.F16 if prec == hr.F16 else VP.BF16


def half_index(metric, prec, ids, rows):
    ix = va.HnswIndex(rows.shape[1], HMETRIC[metric])
    n = len(ids)
    ix.upload(ids[: n // 2], rows[: n // 2])
    ix.enable_half_precision(vp(prec))
    ix.upload(ids[n // 2:], rows[n // 2:])
    return ix


def half_data(kind, rng, shape):
    if kind == "ints":
        return hp.ints(rng, shape)
    if kind == "grid":
        return hp.grid_f16(rng, shape)
    return rng.standard_normal(shape).astype(np.float32)


def positions(sel, gids, gcnt):
    """the returned ids (here: internal rows) as positions in sel; every one of them must be an allowed row"""
    out = np.zeros(gids.shape, np.uint64)
    for qi in range(gids.shape[0]):
        g = gids[qi, :gcnt[qi]].astype(np.int64)
        p = np.searchsorted(sel, g)
        assert np.all(p < len(sel)) and np.array_equal(sel[np.minimum(p, len(sel) - 1)], g), "a row outside the filter was returned"
        out[qi, :gcnt[qi]] = p
    return out


# Euclidean, exact data: integers in [-4, 4] (squared differences <= 64, 1 024 of them stay far below 2^24) for both precisions on every
# shape; the f16 grid of odd multiples of 1 / 256 where its sums stay exact — dim 17: a squared difference is at most 1022^2 units of
# 2^-16, seventeen of them reach 2^24 only if nearly all are extreme; the test asserts the bound on the data it uses
@pytest.mark.parametrize("prec,kind,n,dim", [(p, "ints", n, d) for p in (hr.F16, hr.BF16) for n, d in HALF_SHAPES] + [(hr.F16, "grid", 700, 17)])
def test_half_euclidean_exact_data_bit_equal_on_both_routes(gpu_required, prec, kind, n, dim):
    rng = np.random.default_rng(31 * n + dim + prec + len(kind))
    rows, ids = half_data(kind, rng, (n, dim)), tf.ext_ids(n)
    rows[[5, n - 2]] = 0.0
    rows[[256, 257]] = rows[[1, 1]]            # duplicates: exact ties, by row
    sets = tf.allowed_sets(rng, n)
    qs = {(nq, k): half_data(kind, rng, (nq, dim)) for nq, k in HALF_NQ_K}
    for Q in qs.values():
        Q[0] = rows[n - 1]
    if kind == "grid":
        units = np.rint(np.concatenate([rows] + list(qs.values())).astype(np.float64) * 256.0)
        d2 =((units[:, None, :] - units[None, -128:, :]) ** 2).sum(-1)   # every row against the last 128 vectors (queries among them)
        assert d2.max() <= 2.0 ** 24, "the grid data would not keep its sums exact"
    ix = half_index(hr.EUCLIDEAN, prec, ids, rows)
    try:
        for name, (given, negate, sel) in sets.items():
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq, k in HALF_NQ_K:
                    exp = half_subset(hr.EUCLIDEAN, prec, rows, ids, qs[(nq, k)], k, sel)
                    for route in (LISTED, MASK):
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        got = ix.search_batch_filtered_half(qs[(nq, k)], k, flt, vp(prec))
                        m = ix.last_kernels()
                        assert m & va.KERNEL_SWEEP_HALF_L2 and bool(m & va.KERNEL_SWEEP_LISTED) == (route == LISTED), hex(m)
                        tf.assert_equal(got, exp, (prec, kind, n, dim, name, nq, k, route))
    finally:
        ix.close()


@pytest.mark.parametrize("prec", [hr.F16, hr.BF16])
@pytest.mark.parametrize("n,dim", HALF_SHAPES)
def test_half_euclidean_gaussian_routes_agree_within_tol(gpu_required, prec, n, dim):
    rng = np.random.default_rng(17 * n + dim + prec)
    rows, ids = rng.standard_normal((n, dim)).astype(np.float32), np.arange(n, dtype=np.uint64)
    sets = tf.allowed_sets(rng, n)
    ix = half_index(hr.EUCLIDEAN, prec, ids, rows)
    try:
        for nq, k in HALF_NQ_K:
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
            Q[0] = rows[n - 1]                 # distance exactly 0 to an allowed row
            for name, (given, negate, sel) in sets.items():
                with ix.create_filter(ids[given], negate=negate) as flt:
                    ix.set_option(va.OPT_FILTER_ROUTE, LISTED)
                    li, ls, lc = ix.search_batch_filtered_half(Q, k, flt, vp(prec))
                    assert ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                    ix.set_option(va.OPT_FILTER_ROUTE, MASK)
                    mi, ms, mc = ix.search_batch_filtered_half(Q, k, flt, vp(prec))
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                    assert np.array_equal(lc, mc), (name, nq, k)
                    for qi in range(nq):
                        assert np.array_equal(li[qi, :lc[qi]], mi[qi, :lc[qi]]), (name, nq, k, qi)
                        assert np.array_equal(tf.bits(ls[qi, :lc[qi]]), tf.bits(ms[qi, :lc[qi]])), (name, nq, k, qi)
                    assert ls[0, 0] == 0.0 and li[0, 0] == n - 1
                    # within TOL of half_ref: every query of the small batches, a sample of the 70 (first / last of the batch, the last
                    # query of a 16-query pass, the first and last of the 6-query tail)
                    sample = None if nq <= 17 else [0, 1, 15, 16, 63, 64, nq - 1]
                    hp.check(hr.EUCLIDEAN, prec, rows[sel], Q, k, positions(sel, li, lc), ls, lc, sample)
    finally:
        ix.close()


# Cosine / DotProduct over a half image: mask substitution (no listed kernel).  tier_bits gives the tier a batch takes: nq < 64 the
# streaming matrix-core kernel, nq >= 64 with dim % 64 == 0 the 128 x 128 GEMM — (70, 10) at dims 768 and 1024 —, the seeded 256 x 256 tier
# from 224 queries over >= 65 536 rows (its own test below).
@pytest.mark.parametrize("prec,metric", [(hr.F16, hr.COSINE), (hr.F16, hr.DOT), (hr.BF16, hr.COSINE), (hr.BF16, hr.DOT)])
@pytest.mark.parametrize("n,dim", HALF_SHAPES)
def test_half_cosine_dot_exact_data_bit_equal(gpu_required, prec, metric, n, dim):
    rng = np.random.default_rng(13 * n + dim + 5 * prec + metric)
    rows, ids = hp.ints(rng, (n, dim)), tf.ext_ids(n)
    rows[[5, n - 2]] = 0.0
    rows[[256, 257]] = rows[[1, 1]]
    sets = tf.allowed_sets(rng, n)
    ix = half_index(metric, prec, ids, rows)
    try:
        for route in (AUTO, LISTED):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            for nq, k in HALF_NQ_K if route == AUTO else HALF_NQ_K[:2]:
                Q = hp.ints(rng, (nq, dim))
                Q[0] = rows[n - 1]
                Q[nq // 2] = 0.0 if nq > 2 else Q[nq // 2]
                for name, (given, negate, sel) in sets.items():
                    with ix.create_filter(ids[given], negate=negate) as flt:
                        got = ix.search_batch_filtered_half(Q, k, flt, vp(prec))
                        hp.served_by(ix, hp.tier_bits(metric, prec, nq, n, dim, k), va.KERNEL_SWEEP_LISTED)
                        tf.assert_equal(got, half_subset(metric, prec, rows, ids, Q, k, sel), (prec, metric, n, dim, name, nq, k))
    finally:
        ix.close()


@pytest.mark.parametrize("prec,metric", [(hr.F16, hr.COSINE), (hr.F16, hr.DOT), (hr.BF16, hr.COSINE), (hr.BF16, hr.DOT)])
@pytest.mark.parametrize("n,dim", HALF_SHAPES)
def test_half_cosine_dot_gaussian_within_tol(gpu_required, prec, metric, n, dim):
    rng = np.random.default_rng(19 * n + dim + 5 * prec + metric)
    rows, ids = rng.standard_normal((n, dim)).astype(np.float32), np.arange(n, dtype=np.uint64)
    sets = tf.allowed_sets(rng, n)
    ix = half_index(metric, prec, ids, rows)
    try:
        for nq, k in HALF_NQ_K:
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
            for name, (given, negate, sel) in sets.items():
                with ix.create_filter(ids[given], negate=negate) as flt:
                    gi, gs, gc = ix.search_batch_filtered_half(Q, k, flt, vp(prec))
                    hp.served_by(ix, hp.tier_bits(metric, prec, nq, n, dim, k), va.KERNEL_SWEEP_LISTED)
                    sample = None if nq <= 17 else [0, 1, nq // 2, nq - 1]
                    hp.check(metric, prec, rows[sel], Q, k, positions(sel, gi, gc), gs, gc, sample)
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [hr.DOT, hr.COSINE])
def test_half_cosine_dot_on_the_seeded_big_tier(gpu_required, metric):
    """224 queries over >= 65 536 rows at dim 128: the 256 x 256 tier, whose bounds are seeded from a sweep of the first 16 384 rows
    — under a filter of one row, of k - 1 rows, of 1 % and of half the rows.  Integers: bit for bit."""
    n, dim, nq, k = 65_600, 128, 224, 10
    rng = np.random.default_rng(n + metric)
    rows, ids = hp.ints(rng, (n, dim)), tf.ext_ids(n)
    rows[[5, 20_000]] = 0.0
    sets = tf.allowed_sets(rng, n)
    Q = hp.ints(rng, (nq, dim))
    Q[0] = rows[n - 1]
    sample = np.array([0, 1, 100, 223])
    ix = va.HnswIndex(dim, HMETRIC[metric], va.HnswParams(16, 100, n))
    try:
        ix.upload(ids, rows)
        ix.enable_half_precision(VP.F16)
        for name in ("one", "k-1", "1pct", "half"):
            given, negate, sel = sets[name]
            with ix.create_filter(ids[given], negate=negate) as flt:
                gi, gs, gc = ix.search_batch_filtered_half(Q, k, flt, VP.F16)
                hp.served_by(ix, va.KERNEL_F16 | va.KERNEL_GEMM_BF16_GLDS, va.KERNEL_SWEEP_LISTED)
                exp = half_subset(metric, hr.F16, rows, ids, Q[sample], k, sel)
                tf.assert_equal((gi[sample], gs[sample], gc[sample]), exp, (metric, name))
                assert np.all(gc == min(k, len(sel)))
    finally:
        ix.close()


# ---- semantics, one metric per mode -----------------------------------------------------------------------------------------------------
class Sq8Mode:
    mode, metric, dim = va.MODE_BRUTE_SQ8, DM.Cosine, 64
    routes = (LISTED, MASK)

    @staticmethod
    def enable(ix):
        ix.set_storage_mode(SM.SQ8)

    @staticmethod
    def search(ix, Q, k, flt):
        return ix.search_batch_filtered_sq8(Q, k, flt)

    @staticmethod
    def plain(ix, Q, k):
        return ix.search_batch_sq8(Q, k)

    @staticmethod
    def subset(rows, ids, Q, k, sel):
        return sq8_subset(DM.Cosine, rows, ids, Q, k, sel)


class BinaryMode(Sq8Mode):
    mode, metric, dim = va.MODE_BRUTE_BINARY, DM.Euclidean, 48
    routes = (MASK,)

    @staticmethod
    def enable(ix):
        ix.set_storage_mode(SM.Binary)

    @staticmethod
    def search(ix, Q, k, flt):
        return ix.search_batch_filtered_binary(Q, k, flt)

    @staticmethod
    def plain(ix, Q, k):
        return ix.search_batch_binary(Q, k)

    @staticmethod
    def subset(rows, ids, Q, k, sel):
        return binary_subset(rows, ids, Q, k, sel)


class F16Mode(Sq8Mode):
    mode, metric, dim = va.MODE_BRUTE_F16, DM.Euclidean, 40
    routes = (LISTED, MASK)

    @staticmethod
    def enable(ix):
        ix.enable_half_precision(VP.F16)

    @staticmethod
    def search(ix, Q, k, flt):
        return ix.search_batch_filtered_half(Q, k, flt, VP.F16)

    @staticmethod
    def plain(ix, Q, k):
        return ix.search_batch_brute_force_half(Q, k, VP.F16)

    @staticmethod
    def subset(rows, ids, Q, k, sel):
        return half_subset(hr.EUCLIDEAN, hr.F16, rows, ids, Q, k, sel)


class Bf16Mode(Sq8Mode):
    mode, metric, dim = va.MODE_BRUTE_BF16, DM.DotProduct, 64
    routes = (MASK,)

    @staticmethod
    def enable(ix):
        ix.enable_half_precision(VP.BF16)

    @staticmethod
    def search(ix, Q, k, flt):
        return ix.search_batch_filtered_half(Q, k, flt, VP.BF16)

    @staticmethod
    def plain(ix, Q, k):
        return ix.search_batch_brute_force_half(Q, k, VP.BF16)

    @staticmethod
    def subset(rows, ids, Q, k, sel):
        return half_subset(hr.DOT, hr.BF16, rows, ids, Q, k, sel)


MODES = [Sq8Mode, BinaryMode, F16Mode, Bf16Mode]


def mode_rows(M, rng, n):
    # (integers: every mode's arithmetic is exact on them, so the half Cosine / DotProduct tiers compare bit for bit too)
    return hp.ints(rng, (n, M.dim)) if M.mode in (va.MODE_BRUTE_F16, va.MODE_BRUTE_BF16) else rng.standard_normal((n, M.dim)).astype(np.float32)


def raw_call(ix, flt_handle, mode, Q, k):
    """the C entry point with sentinel-filled outputs: (status, outputs untouched?)"""
    L = va._ffi.lib()
    nq = Q.shape[0]
    oi, osc, on = np.full((nq, k), 0xABCDEF, np.uint64), np.full((nq, k), -77.0, np.float32), np.full(nq, 0xFEED, np.uint32)
    rc = L.vdb_hip_index_search_batch_filtered_mode(ix._h, flt_handle, mode, Q.ctypes.data_as(C.c_void_p), nq, k, oi.ctypes.data_as(C.c_void_p),
                                                    osc.ctypes.data_as(C.c_void_p), on.ctypes.data_as(C.c_void_p))
    return rc, bool(np.all(oi == 0xABCDEF) and np.all(osc == -77.0) and np.all(on == 0xFEED))


@pytest.mark.parametrize("M", MODES, ids=lambda M: M.__name__)
def test_snapshot_semantics_and_errors(gpu_required, M):
    n, k = 1000, 10
    rng = np.random.default_rng(9 + M.mode)
    rows, ids = mode_rows(M, rng, n + 1), tf.ext_ids(n + 1)
    Q = np.ascontiguousarray(mode_rows(M, rng, 3))
    ix, other, bare = va.HnswIndex(M.dim, M.metric), va.HnswIndex(M.dim, M.metric), va.HnswIndex(M.dim, M.metric)
    try:
        for h in (ix, other, bare):
            h.upload(ids[:n], rows[:n])
        M.enable(ix)
        M.enable(other)
        sel = np.sort(rng.choice(n, size=12, replace=False))
        flt = ix.create_filter(np.concatenate([ids[sel], ids[sel[:4]], [ids[n]], [7, 8]]).astype(np.uint64))
        assert flt.matched == 12
        before = M.plain(ix, Q, k)
        for route in M.routes:
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            tf.assert_equal(M.search(ix, Q, k, flt), M.subset(rows, ids, Q, k, sel), ("fresh", route))
        after = M.plain(ix, Q, k)             # an unfiltered call after filtered ones: what it returned before them
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        for gone in sel[:3]:                  # rows removed after creation disappear, on both routes
            assert ix.remove(int(ids[gone]))
        ix.upload(ids[n:n + 1], rows[n:n + 1])  # a row inserted after creation never appears (its id was in the creation list)
        for route in M.routes:
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = M.search(ix, Q, k, flt)
            assert list(got[2]) == [9, 9, 9] and ids[n] not in got[0][:, :9]
            tf.assert_equal(got, M.subset(rows, ids, Q, k, sel[3:]), ("after removals and an insert", route))
            with ix.create_filter(ids[sel[3:]], negate=True) as neg:
                assert neg.matched == n + 1 - 9
                live = np.setdiff1d(np.arange(n + 1), sel)
                tf.assert_equal(M.search(ix, Q, k, neg), M.subset(rows, ids, Q, k, live), ("negate", route))
            with ix.create_filter(np.empty(0, np.uint64)) as empty:
                assert list(M.search(ix, Q, k, empty)[2]) == [0, 0, 0]
        E = va._ffi
        with other.create_filter(ids[sel]) as foreign:
            assert raw_call(ix, foreign._h, M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
            assert raw_call(bare, foreign._h, M.mode, Q, k)[0] == E.VDB_ERR_INVALID_ARG
        assert raw_call(ix, None, M.mode, Q, k) == (E.VDB_ERR_INVALID_ARG, True)
        for bad in (va.MODE_BRUTE, va.MODE_HNSW, va.MODE_AUTO, va.MODE_HNSW_INT8, va.MODE_HNSW_F16, va.MODE_HNSW_BF16, 77):
            assert raw_call(ix, flt._h, bad, Q, k) == (E.VDB_ERR_UNSUPPORTED, True), bad
        with bare.create_filter(ids[sel]) as fb:  # the mode's storage mode / image is not enabled on this handle
            assert raw_call(bare, fb._h, M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        ix.vacuum()                              # renumbers the rows: the old filter is stale
        assert raw_call(ix, flt._h, M.mode, Q, k) == (E.VDB_ERR_STATE, True)
        flt.close()
    finally:
        for h in (ix, other, bare):
            h.close()
    sh = va.HnswIndex(M.dim, M.metric, devices=[0, 0], shard_mode=va.SHARD_RANGE)
    one = va.HnswIndex(M.dim, M.metric)
    try:
        sh.upload(ids[:n], rows[:n])
        one.upload(ids[:n], rows[:n])
        with one.create_filter(ids[:10]) as f1:  # (a multi-device handle cannot make a filter: any filter is refused there)
            assert raw_call(sh, f1._h, M.mode, Q, k) == (va._ffi.VDB_ERR_UNSUPPORTED, True)
    finally:
        sh.close()
        one.close()


@pytest.mark.parametrize("M", MODES, ids=lambda M: M.__name__)
def test_two_threads_share_a_filter(gpu_required, M):
    n, k, rounds = 3000, 10, 12
    rng = np.random.default_rng(21 + M.mode)
    rows, ids = mode_rows(M, rng, n), tf.ext_ids(n)
    Qs = [np.ascontiguousarray(mode_rows(M, rng, 1 + i % 5)) for i in range(rounds)]
    ix = va.HnswIndex(M.dim, M.metric)
    try:
        ix.upload(ids, rows)
        M.enable(ix)
        ix.set_option(va.OPT_FILTER_ROUTE, M.routes[0])
        with ix.create_filter(ids[np.sort(rng.choice(n, size=700, replace=False))]) as flt:
            alone = [M.search(ix, Q, k, flt) for Q in Qs]
            errors = []

            def worker(t):
                try:
                    for r in range(3):
                        for i, Q in enumerate(Qs):
                            got = M.search(ix, Q, k, flt)
                            if not all(np.array_equal(a, b) for a, b in zip(got, alone[i])):
                                errors.append((t, r, i))
                except Exception as ex:  # noqa: BLE001
                    errors.append((t, repr(ex)))

            threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            assert not errors, errors[:5]
    finally:
        ix.close()
