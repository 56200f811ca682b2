"""The gathered matrix-core tier of filtered Cosine / DotProduct search over the f16 / bf16 image (FILTER_ROUTE_GATHERED):
sweep_topk_half_gathered reads only the filter's rows and must return what the plain half-precision search returns on an index that
holds only those rows.  Reference: tests/half_ref.py — the score matrix of a case is computed ONCE over all rows (a score depends on
the row and the query only) and every filter's answer is its top-k over the filter's columns.  Integer data: bit for bit; Gaussian
data: tests/test_gpu_half_precision.py::check (its TOL, tie-aware, against the float64 truth).  Every call runs under route value 3 and
asserts the kernel bits of the tier."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_ref as hr  # noqa: E402
import test_gpu_filtered as tf  # noqa: E402
import test_gpu_filtered_modes as fm  # noqa: E402
import test_gpu_half_precision as hp  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
CASES = [(hr.F16, hr.COSINE), (hr.F16, hr.DOT), (hr.BF16, hr.COSINE), (hr.BF16, hr.DOT)]
DIMS = [64, 72, 200, 768]      # one 64-element slice; a stride that is no multiple of 32; a tail slice; twelve slices


def bits_of(prec):
    return va.KERNEL_SWEEP_LISTED | va.KERNEL_GEMM_HALF_GATHERED | (va.KERNEL_F16 if prec == hr.F16 else 0)


def gathered(ix, Q, k, flt, prec):
    ix.set_option(va.OPT_FILTER_ROUTE, 3)
    got = ix.search_batch_filtered_half(Q, k, flt, fm.vp(prec))
    hp.served_by(ix, bits_of(prec))
    return got


def expected(sc, ids, k, sel):
    """[(ids, scores)] per query: the top-k of the score matrix over the filter's columns, ties by row"""
    r, s, kk = hr.topk(sc[:, sel], min(k, len(sel)), True)
    return [(ids[sel[r[qi, :kk].astype(np.int64)]], s[qi, :kk]) for qi in range(sc.shape[0])]


def tile_edge_sets(rng, n):
    sets = tf.allowed_sets(rng, n)                       # one row, k - 1 rows, half the rows, a negated one, ...
    for m in (63, 64, 65):                               # the 64-row tile's edge
        rows = np.sort(np.concatenate([[0, 1, 5, 256, 257, n - 1], rng.choice(np.arange(300, n - 1), m - 6, replace=False)])).astype(np.int64)
        sets[str(m)] = (rows, False, rows)
    return sets


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("prec,metric", CASES)
def test_exact_data_bit_for_bit(gpu_required, prec, metric, dim):
    """n = 9 000: half of them span several blocks; the negated set under 1 024 queries (eight query tiles) and every row under k = 500
    (one resident block a CU) give a block more than one tile at both instances — at dim 64 with one slice a tile."""
    n = 9000
    rng = np.random.default_rng(dim + 7 * prec + metric)
    rows, ids, Q = hp.ints(rng, (n, dim)), tf.ext_ids(n), hp.ints(rng, (130, dim))
    rows[[5, n - 2]] = 0.0
    rows[[256, 257]] = rows[[1, 1]]                      # duplicates: exact ties, by row
    Q[0], Q[8] = rows[n - 1], 0.0
    sc = hr.scores(metric, prec, rows, Q)
    sets = tile_edge_sets(rng, n)
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        for name, (given, negate, sel) in sets.items():
            big = len(sel) > 1000
            shapes = [(17, 10), (130, 64)] if big else [(1, 10), (16, 1), (17, 10), (130, 64), (1, 1), (130, 10)]
            if dim < 768:
                shapes += {"not10pct": [(1024, 10)], "all": [(17, 500)]}.get(name, [])
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq, k in shapes:
                    pick = np.arange(nq) % 130            # (the 1 024 queries: the 130, repeated)
                    tf.assert_equal(gathered(ix, Q[pick], k, flt, prec), expected(sc[pick], ids, k, sel), (prec, metric, dim, name, nq, k))
    finally:
        ix.close()


@pytest.fixture(scope="module")
def gauss():
    made = {}

    def get(prec, metric, dim, n=3000):
        key = (prec, metric, dim)
        if key not in made:
            rng = np.random.default_rng(100 + dim + 7 * prec + metric)
            rows, Q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((130, dim)).astype(np.float32)
            made[key] = (rows, Q, tile_edge_sets(rng, n))
        return made[key]
    return get


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("prec,metric", CASES)
def test_gaussian_within_the_modes_tolerance(gpu_required, gauss, prec, metric, dim):
    rows, Q, sets = gauss(prec, metric, dim)
    ids = np.arange(len(rows), dtype=np.uint64)
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        for name in ("65", "half", "not10pct"):
            given, negate, sel = sets[name]
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq in (17, 130):
                    gi, gs, gc = gathered(ix, Q[:nq], 10, flt, prec)
                    hp.check(metric, prec, rows[sel], Q[:nq], 10, fm.positions(sel, gi, gc), gs, gc, [0, 15, 16, nq - 1])
    finally:
        ix.close()


@pytest.mark.parametrize("prec,metric", CASES)
def test_a_querys_bits_do_not_depend_on_its_batch(gpu_required, gauss, prec, metric):
    """Gaussian data, dim 200: query i of 130 (128-query tiles) against the same query alone (the 16-query instance); then one call
    with three filters and unfiltered queries against each query's one-filter call."""
    rows, Q, sets = gauss(prec, metric, 200)
    ids = np.arange(len(rows), dtype=np.uint64)
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        flts = [ix.create_filter(ids[sets[name][0]], negate=sets[name][1]) for name in ("half", "65", "not10pct")]
        gi, gs, gc = gathered(ix, Q, 10, flts[0], prec)
        for qi in (0, 77, 127, 128, 129):
            ai, as_, ac = gathered(ix, Q[qi:qi + 1], 10, flts[0], prec)
            assert ac[0] == gc[qi] and np.array_equal(ai[0], gi[qi]) and np.array_equal(tf.bits(as_[0]), tf.bits(gs[qi])), qi
        table = [flts[i % 4] if i % 4 < 3 else None for i in range(40)]
        mi, ms, mc = ix.search_batch_brute_force_with_filters_half(Q[:40], 10, table, fm.vp(prec))
        hp.served_by(ix, bits_of(prec))
        none = [i for i in range(40) if table[i] is None]
        pi, ps, pc = hp.search(ix, Q[none], 10, prec)       # the unfiltered queries: the plain call over them, in call order
        for i in range(40):
            if table[i] is None:
                oi, os_, oc = pi[none.index(i)], ps[none.index(i)], pc[none.index(i)]
            else:
                (oi,), (os_,), (oc,) = gathered(ix, Q[i:i + 1], 10, table[i], prec)
            assert oc == mc[i] and np.array_equal(oi, mi[i]) and np.array_equal(tf.bits(os_), tf.bits(ms[i])), i
        for f in flts:
            f.close()
    finally:
        ix.close()


@pytest.mark.parametrize("prec,metric", CASES)
def test_rows_deleted_after_the_filter_was_made_are_absent(gpu_required, prec, metric):
    n, dim, k = 600, 72, 10
    rng = np.random.default_rng(prec + metric)
    rows, ids, Q = hp.ints(rng, (n, dim)), tf.ext_ids(n), hp.ints(rng, (17, dim))
    sc = hr.scores(metric, prec, rows, Q)
    sel = np.arange(0, n, 50, dtype=np.int64)               # twelve listed rows ...
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        with ix.create_filter(ids[sel]) as flt:
            best = int(np.flatnonzero(ids == gathered(ix, Q, k, flt, prec)[0][0, 0])[0])
            dead = np.array([best, int(sel[sel != best][-1])])   # ... two removed: query 0's best one and the last of the others
            assert all(ix.remove(int(ids[r])) for r in dead)
            left = np.setdiff1d(sel, dead)
            got = gathered(ix, Q, k, flt, prec)
            assert np.all(got[2] == len(left)) and len(left) == 10
            tf.assert_equal(got, expected(sc, ids, k, left), (prec, metric))
    finally:
        ix.close()


@pytest.mark.parametrize("prec,metric", CASES)
def test_a_k_without_a_plan_answers_through_mask_substitution(gpu_required, prec, metric):
    n, dim, nq = 3000, 64, 3
    k = next(k for k in range(1, 1 << 16) if va.half_gather_plan(dim, k, n // 2, nq, 256) is None)
    assert va.half_gather_plan(dim, k - 1, n // 2, nq, 256)["tn"] == 16
    rng = np.random.default_rng(3 * prec + metric)
    rows, ids, Q = hp.ints(rng, (n, dim)), tf.ext_ids(n), hp.ints(rng, (nq, dim))
    sc = hr.scores(metric, prec, rows, Q)
    given, negate, sel = tf.allowed_sets(rng, n)["half"]
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        with ix.create_filter(ids[given], negate=negate) as flt:
            ix.set_option(va.OPT_FILTER_ROUTE, 3)
            got = ix.search_batch_filtered_half(Q, k, flt, fm.vp(prec))
            hp.served_by(ix, hp.tier_bits(metric, prec, nq, n, dim, k), va.KERNEL_SWEEP_LISTED | va.KERNEL_GEMM_HALF_GATHERED)
            tf.assert_equal(got, expected(sc, ids, k, sel), (prec, metric, k))
            tf.assert_equal(gathered(ix, Q, k - 1, flt, prec), expected(sc, ids, k - 1, sel), (prec, metric, k - 1))
    finally:
        ix.close()
