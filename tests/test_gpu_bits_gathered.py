"""The gathered four-bit matrix-core tier of filtered search over packed bits (FILTER_ROUTE_GATHERED): Hamming / Jaccard
indexes and the Binary storage mode.  sweep_topk_bits_gathered reads only the packed rows of the filter's list.  Reference: plain numpy
integers — bit counts from an int64 matrix product over ALL rows, once per case; every filter's answer is the top-k over the filter's
columns, ties by row.  Every gathered call asserts the tier's kernel bits (on a library without the tier value 3 is auto: no such bits)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_filtered as tf  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
KINDS = ["hamming", "jaccard", "binary"]
DIMS = [48, 256, 264, 768, 1000]  # half a second word; one slice; a slice + one word; three slices; no multiple of 32 (zero padding nibbles)
TIER = va.KERNEL_BITS | va.KERNEL_SWEEP_LISTED | va.KERNEL_BITS_GATHERED


def data(kind, rng, shape):
    return rng.standard_normal(shape).astype(np.float32) if kind == "binary" else (rng.random(shape) > 0.6915).astype(np.float32)


def index(kind, ids, rows):
    ix = va.HnswIndex(rows.shape[1], {"hamming": DM.Hamming, "jaccard": DM.Jaccard, "binary": DM.Euclidean}[kind])
    ix.upload(ids, rows)
    if kind == "binary":
        ix.set_storage_mode(va.StorageMode.Binary)
    ix.set_option(va.OPT_FILTER_ROUTE, 3)
    return ix


def call(kind, ix, Q, k, flt=None, table=None):
    if table is not None:
        return ix.search_batch_with_filters_binary(Q, k, table) if kind == "binary" else ix.search_batch_brute_force_with_filters(Q, k, table)
    if flt is None:
        return ix.search_batch_binary(Q, k) if kind == "binary" else ix.search_batch_brute_force(Q, k)
    return ix.search_batch_filtered_binary(Q, k, flt) if kind == "binary" else ix.search_batch_brute_force_filtered(Q, k, flt)


def gathered(kind, ix, Q, k, flt=None, table=None):
    got = call(kind, ix, Q, k, flt, table)
    m = ix.last_kernels()
    assert m & TIER == TIER and not m & va.KERNEL_BITS_GEMM, hex(m)
    return got


def scores(kind, rows, Q):
    """[nq][n] f32, SMALLER = better (Jaccard negated: exact)"""
    b, q = ((rows >= 0, Q >= 0) if kind == "binary" else (rows > 0.5, Q > 0.5))
    b, q = b.astype(np.int64), q.astype(np.int64)
    inter, nb, nq = q @ b.T, b.sum(1)[None, :], q.sum(1)[:, None]
    if kind != "jaccard":
        return (nq + nb - 2 * inter).astype(np.float32)
    uni = nq + nb - inter
    return -np.where(uni == 0, np.float32(1.0), inter.astype(np.float32) / np.maximum(uni, 1).astype(np.float32)).astype(np.float32)


def expected(kind, sc, ids, k, sel):
    """[(ids, scores)] per query: the top-k over the filter's columns (ascending rows), ties by row"""
    s = sc[:, sel]
    order = np.argsort(s, axis=1, kind="stable")[:, :k]
    sign = np.float32(-1.0 if kind == "jaccard" else 1.0)
    return [(ids[sel[order[qi]]], sign * s[qi, order[qi]]) for qi in range(sc.shape[0])]


def tile_edge_sets(rng, n):
    sets = tf.allowed_sets(rng, n)                       # one row, k - 1 rows, half the rows, a negated one, ...
    for m in (63, 64, 65):                               # the 64-row tile's edge
        rows = np.sort(np.concatenate([[0, 1, 5, 256, 257, n - 1], rng.choice(np.arange(300, n - 1), m - 6, replace=False)])).astype(np.int64)
        sets[str(m)] = (rows, False, rows)
    return sets


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_for_bit(gpu_required, kind, dim):
    """n = 9 000: the large sets span several blocks; the negated set under 1 024 queries (eight query tiles) and every row under
    k = 500 (the 16-query instance at one resident block) give a block more than one tile at both instances."""
    n = 9000
    rng = np.random.default_rng(dim + 7 * KINDS.index(kind))
    rows, ids, Q = data(kind, rng, (n, dim)), tf.ext_ids(n), data(kind, rng, (130, dim))
    rows[5] = 0.0                                        # an all-zero row (Binary: every sign bit set)
    rows[[256, 257]] = rows[[1, 1]]                      # duplicates: exact ties, by row
    Q[0], Q[8] = rows[n - 1], 0.0                        # a query equal to a row; an all-zero query (Jaccard: an empty union with row 5)
    sc = scores(kind, rows, Q)
    ix = index(kind, ids, rows)
    try:
        for name, (given, negate, sel) in tile_edge_sets(rng, n).items():
            shapes = [(1, 10), (16, 1), (17, 10), (130, 64), (130, 10)] + {"not10pct": [(1024, 10)], "all": [(17, 500)]}.get(name, [])
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq, k in shapes:
                    pick = np.arange(nq) % 130            # (the 1 024 queries: the 130, repeated)
                    tf.assert_equal(gathered(kind, ix, Q[pick], k, flt), expected(kind, sc[pick], ids, k, sel), (kind, dim, name, nq, k))
    finally:
        ix.close()


@pytest.mark.parametrize("kind", KINDS)
def test_one_call_with_three_filters_and_unfiltered_queries(gpu_required, kind):
    n, dim, k = 3000, 264, 10
    rng = np.random.default_rng(11 + KINDS.index(kind))
    rows, ids, Q = data(kind, rng, (n, dim)), tf.ext_ids(n), data(kind, rng, (40, dim))
    sets = tile_edge_sets(rng, n)
    ix = index(kind, ids, rows)
    try:
        flts = [ix.create_filter(ids[sets[name][0]], negate=sets[name][1]) for name in ("half", "65", "not10pct")]
        table = [flts[i % 4] if i % 4 < 3 else None for i in range(40)]
        mi, ms, mc = gathered(kind, ix, Q, k, table=table)
        none = [i for i in range(40) if table[i] is None]
        pi, ps, pc = call(kind, ix, Q[none], k)             # the unfiltered queries: the plain call over them, in call order
        for i in range(40):
            if table[i] is None:
                oi, os_, oc = pi[none.index(i)], ps[none.index(i)], pc[none.index(i)]
            else:
                (oi,), (os_,), (oc,) = gathered(kind, ix, Q[i:i + 1], k, table[i])
            assert oc == mc[i] and np.array_equal(oi, mi[i]) and np.array_equal(tf.bits(os_), tf.bits(ms[i])), i
        for f in flts:
            f.close()
    finally:
        ix.close()


@pytest.mark.parametrize("kind", KINDS)
def test_rows_removed_after_the_filter_was_made_are_absent(gpu_required, kind):
    n, dim, k = 600, 72, 10
    rng = np.random.default_rng(3 + KINDS.index(kind))
    rows, ids, Q = data(kind, rng, (n, dim)), tf.ext_ids(n), data(kind, rng, (17, dim))
    sc = scores(kind, rows, Q)
    sel = np.arange(0, n, 50, dtype=np.int64)               # twelve listed rows ...
    ix = index(kind, ids, rows)
    try:
        with ix.create_filter(ids[sel]) as flt:
            best = int(np.flatnonzero(ids == gathered(kind, ix, Q, k, flt)[0][0, 0])[0])
            dead = np.array([best, int(sel[sel != best][-1])])   # ... two removed: query 0's best one and the last of the others
            assert all(ix.remove(int(ids[r])) for r in dead)
            left = np.setdiff1d(sel, dead)
            got = gathered(kind, ix, Q, k, flt)
            assert np.all(got[2] == 10) and len(left) == 10
            tf.assert_equal(got, expected(kind, sc, ids, k, left), kind)
    finally:
        ix.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_k_without_a_plan_answers_through_mask_substitution(gpu_required, kind):
    n, dim, nq = 3000, 48, 3
    k = next(k for k in range(1, 1 << 16) if va.bits_gather_plan(k, n // 2, nq, 256) is None)
    assert va.bits_gather_plan(k - 1, n // 2, nq, 256)["tn"] == 16
    rng = np.random.default_rng(5 + KINDS.index(kind))
    rows, ids, Q = data(kind, rng, (n, dim)), tf.ext_ids(n), data(kind, rng, (nq, dim))
    sc = scores(kind, rows, Q)
    given, negate, sel = tf.allowed_sets(rng, n)["half"]
    ix = index(kind, ids, rows)
    try:
        with ix.create_filter(ids[given], negate=negate) as flt:
            got = call(kind, ix, Q, k, flt)
            m = ix.last_kernels()
            assert m & va.KERNEL_BITS and not m & (va.KERNEL_SWEEP_LISTED | va.KERNEL_BITS_GATHERED), hex(m)
            tf.assert_equal(got, expected(kind, sc, ids, k, sel), (kind, k))
            tf.assert_equal(gathered(kind, ix, Q, k - 1, flt), expected(kind, sc, ids, k - 1, sel), (kind, k - 1))
    finally:
        ix.close()
