"""The gathered f32 matrix-core tier of filtered exact search (FILTER_ROUTE_GATHERED over the f32 rows): Cosine / DotProduct on
a handle that answers in mode M.  sweep_topk_f32_gathered reads only the rows of the filter's list and runs mode M's chain on
v_mfma_f32_16x16x4_f32.  Reference: the oracle's mode-M scan over rows[sel] (tests/test_gpu_filtered.py oracle_subset), once per filter
set; ids, counts and score BITS.  Every gathered call asserts the tier's kernel bits."""
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_filtered as tf  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
METRICS = [DM.Cosine, DM.DotProduct]


def index(metric, ids, rows):
    ix = va.HnswIndex(rows.shape[1], metric)
    ix.upload(ids, rows)
    ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_GATHERED)
    return ix


def gathered(ix, Q, k, flt=None, table=None):
    got = ix.search_batch_brute_force_filtered(Q, k, flt) if table is None else ix.search_batch_brute_force_with_filters(Q, k, table)
    tier = va.KERNEL_SWEEP_LISTED | va.KERNEL_GEMM_F32_GATHERED
    assert ix.last_kernels() & tier == tier, hex(ix.last_kernels())
    return got


def prefix(exp, nq, k):
    """the answer for the first nq queries at a smaller k: the front of every list (best first, ties by row)"""
    return [(i[:k], s[:k]) for i, s in exp[:nq]]


@pytest.mark.parametrize("dim", [3, 32, 136, 768])  # one partial slot; exactly one slice; a 128-block + a partial slot; 24 slices
@pytest.mark.parametrize("metric", METRICS)
def test_bit_for_bit(gpu_required, metric, dim):
    n = 9000
    rng = np.random.default_rng(dim + 31 * int(metric))
    rows, ids, Q = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n), tf.rand_rows(rng, 130, dim, metric)
    rows[[5, n - 1]] = 0.0                               # zero rows (Cosine: score 0.0)
    rows[[256, 257]] = rows[[1, 1]]                      # duplicates: exact ties, by row
    Q[0] = rows[0]                                       # a query equal to a row
    sets = tf.allowed_sets(rng, n)
    for m in (63, 64, 65):                               # the 64-row tile's edge
        sel = np.sort(np.concatenate([[0, 1, 5, 256, 257, n - 1], rng.choice(np.arange(300, n - 1), m - 6, replace=False)])).astype(np.int64)
        sets[str(m)] = (sel, False, sel)
    ix = index(metric, ids, rows)
    try:
        assert ix.sweep_arith_mode(64) == ix.sweep_arith_mode(500) == "M"
        for name, (given, negate, sel) in sets.items():
            exp = tf.oracle_subset(metric, rows, ids, Q, 64, sel, po.MODE_M)
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq, k in [(1, 10), (16, 1), (17, 10), (130, 64), (130, 10)]:
                    tf.assert_equal(gathered(ix, Q[:nq], k, flt), prefix(exp, nq, k), (str(metric), dim, name, nq, k))
                if dim < 768 and name == "not10pct":     # eight query tiles of 128; a block with more than one tile
                    pick = np.arange(1024) % 130
                    tf.assert_equal(gathered(ix, Q[pick], 10, flt), [prefix(exp, 130, 10)[i] for i in pick], (str(metric), dim, name, 1024))
                if dim < 768 and name == "all":          # the 16-query instance with long lists
                    tf.assert_equal(gathered(ix, Q[:17], 500, flt), tf.oracle_subset(metric, rows, ids, Q[:17], 500, sel, po.MODE_M), (str(metric), dim, name, 500))
    finally:
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_special_values_dead_rows_and_later_rows(gpu_required, metric):
    """Every infinity sits in column 1 and no vector holds two, so no pair adds opposite infinities; DotProduct leaves the zero row out
    of the list, where 0 * inf would be a NaN the two machines sign differently (Cosine answers 0.0 for a zero norm before it looks)."""
    n, dim, k = 400, 136, 10
    rng = np.random.default_rng(77 + int(metric))
    rows, ids, Q = tf.rand_rows(rng, n + 70, dim, metric), tf.ext_ids(n + 70), tf.rand_rows(rng, 20, dim, metric)
    for v in (rows, Q):                                  # one component each, vectors 2 .. 6
        v[2, 1], v[3, 1], v[4, 3], v[5, 133], v[6, 135] = np.inf, -np.inf, np.nan, 1e-41, -0.0
    rows[7] = 0.0
    rows[n:n + 3] = Q[10:13]                             # rows uploaded later: the best there would be
    sel = np.concatenate([np.arange(2, 7 if metric == DM.DotProduct else 8), np.arange(20, n, 3)]).astype(np.int64)
    ix = index(metric, ids[:n], rows[:n])
    try:
        with ix.create_filter(ids[sel]) as flt:
            tf.assert_equal(gathered(ix, Q, k, flt), tf.oracle_subset(metric, rows, ids, Q, k, sel, po.MODE_M), (str(metric), "special"))
            dead = sel[[8, 70]]
            assert all(ix.remove(int(ids[r])) for r in dead) and ix.upload(ids[n:], rows[n:]) == 70
            left = np.setdiff1d(sel, dead)
            for nq in (20, 3):
                tf.assert_equal(gathered(ix, Q[:nq], k, flt), tf.oracle_subset(metric, rows, ids, Q[:nq], k, left, po.MODE_M), (str(metric), "later", nq))
    finally:
        ix.close()


def test_one_call_with_three_filters_and_unfiltered_queries(gpu_required):
    n, dim, k = 3000, 136, 10
    rng = np.random.default_rng(11)
    rows, ids, Q = tf.rand_rows(rng, n, dim, DM.Cosine), tf.ext_ids(n), tf.rand_rows(rng, 40, dim, DM.Cosine)
    sets = tf.allowed_sets(rng, n)
    ix = index(DM.Cosine, ids, rows)
    try:
        flts = [ix.create_filter(ids[sets[name][0]], negate=sets[name][1]) for name in ("half", "1pct", "not10pct")]
        table = [flts[i % 4] if i % 4 < 3 else None for i in range(40)]
        mi, ms, mc = gathered(ix, Q, k, table=table)
        for i in range(40):
            if table[i] is None:
                (oi,), (os_,), (oc,) = ix.search_batch_brute_force(Q[i:i + 1], k)
            else:
                (oi,), (os_,), (oc,) = gathered(ix, Q[i:i + 1], k, table[i])
            assert oc == mc[i] and np.array_equal(oi, mi[i]) and np.array_equal(tf.bits(os_), tf.bits(ms[i])), i
        for f in flts:
            f.close()
    finally:
        ix.close()


@pytest.mark.parametrize("who", ["euclidean", "engine0", "hamming"])
def test_who_does_not_take_it(gpu_required, who):
    n, dim, k = 2000, 136, 10
    metric = {"euclidean": DM.Euclidean, "engine0": DM.Cosine, "hamming": DM.Hamming}[who]
    rng = np.random.default_rng(5)
    rows, ids, Q = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n), tf.rand_rows(rng, 17, dim, metric)
    given, negate, sel = tf.allowed_sets(rng, n)["1pct"]
    if who == "engine0":
        va.set_sweep_engine(0)
    try:
        ix = index(metric, ids, rows)
        try:
            with ix.create_filter(ids[given], negate=negate) as flt:
                got = ix.search_batch_brute_force_filtered(Q, k, flt)
                assert not ix.last_kernels() & va.KERNEL_GEMM_F32_GATHERED, hex(ix.last_kernels())
                tf.assert_equal(got, tf.oracle_subset(metric, rows, ids, Q, k, sel, tf.arith_mode(ix, k)), who)
        finally:
            ix.close()
    finally:
        va.set_sweep_engine(1)
