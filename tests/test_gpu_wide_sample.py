"""GPU parity tests of the WIDE selection's seed taken by the selection kernel itself (csrc/g16_sample.inc: the SAMPLE instance of the
ping-pong kernel; csrc/vdb_wide_sample.hpp; select_stage.hip brute_wide_dev): the first 16 384 rows (32 768 for k > 32) are swept once
by `sweep_topk_sample_bf16_pp`, which keeps the best approximate score of every 64 rows as a sample key; the k-th best key is the
first bound, and the selection launches start at row 0 again under it.  Any sample yields a valid bound as long as a key reflects only
rows that exist and are alive — what these cases aim at: ragged corpora and batches (a batch with no head launch at all), dead rows
inside the sample range, the best rows packed into few sample groups, non-finite rows in the sample range.

Bar: ids, ranks and score bits of the exact kernels (oracle mode M; Euclidean: mode C), `last_select_level() == 4`.  The equality is
bitwise, no tolerance is involved."""
import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
PO = {DM.Cosine: po.COSINE, DM.DotProduct: po.DOT, DM.Euclidean: po.EUCLIDEAN}
LEVEL_WIDE = 4
DIM = 768


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle(ix, metric, rows, qs, k, alive=None):
    mode = po.MODE_C if metric == DM.Euclidean else (po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C)
    if alive is None:
        return po.scan_topk(PO[metric], rows, qs, k, mode, nthreads=po.host_threads())
    keep = np.nonzero(alive)[0]
    eid, esc = po.scan_topk(PO[metric], rows[keep], qs, k, mode, nthreads=po.host_threads())
    return keep[eid.astype(np.int64)].astype(np.uint64), esc


def check(ix, qs, k, expected):
    """one batch against the oracle's answer for (at least) these queries; returns (queries, unproven) of the batch"""
    eid, esc = expected
    nq = len(qs)
    ids, sc, cnt = ix.search_batch_brute_force(qs, k)
    assert ix.last_select_level() == LEVEL_WIDE, f"select level {ix.last_select_level()} served k = {k}"
    assert np.all(cnt == k)
    assert np.array_equal(ids, eid[:nq]), f"ids / ranks differ from the oracle at nq = {nq}, k = {k}"
    assert np.array_equal(bits(sc), bits(esc[:nq])), f"score bits differ from the oracle at nq = {nq}, k = {k}"
    return ix.last_split_stats()


# ---- 1. ragged corpus and batches -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(gpu_required):
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((66_001, DIM), dtype=np.float32)
    qs = rng.standard_normal((1000, DIM), dtype=np.float32)
    return rows, qs


@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct, DM.Euclidean])
def test_ragged_corpus_and_batches(ragged, metric):
    """66 001 rows (a ragged last row tile); 1 000 queries = a partly filled last query tile, 300 = two query tiles, 96 = one query tile
    on a chip that holds more row groups than the corpus has row tiles: no head launch at all (sample, then one launch)"""
    rows, qs = ragged
    cases = ((300, 10), (96, 64)) if metric == DM.Euclidean else ((1000, 10), (300, 10), (300, 50), (96, 128))
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(len(rows), dtype=np.uint64), rows)
    ref = {}
    for nq, k in cases:  # (largest batch of a k first: its oracle answer serves the smaller ones)
        if k not in ref:
            ref[k] = oracle(ix, metric, rows, qs[:nq], k)
        check(ix, qs[:nq], k, ref[k])
    ix.close()


# ---- 2. dead rows inside the sample range -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_dead(gpu_required):
    """query 0's 40 nearest rows in rows 100 .. 139, query 1's in rows 9 000 .. 9 039 (near-copies, sigma 0.05) — all inside the sample"""
    rng = np.random.default_rng(5150)
    n = 70_003
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((96, DIM), dtype=np.float32)
    rows[100:140] = qs[0] + 0.05 * rng.standard_normal((40, DIM)).astype(np.float32)
    rows[9000:9040] = qs[1] + 0.05 * rng.standard_normal((40, DIM)).astype(np.float32)
    alive = np.ones(n, dtype=bool)
    alive[100:140] = False
    alive[9000:9040] = False
    return rows, qs, alive


@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct])
def test_dead_rows_inside_the_sample_range(planted_dead, metric):
    """All 80 planted rows are soft-deleted through the index's own remove call.  A sample that counted them would set a bound that no
    live row reaches: the lists of queries 0 and 1 would stay short of k and their answers would lack rows.  Unproven queries: none —
    seed_scores_bf16 skipped dead rows the same way, the data is finite, and Gaussian rows with 40 deleted neighbours per query leave
    lists far below their capacity (a few hundred entries of 4 096), so nothing gives a query up.  k = 2 is this file's own addition: 40 consecutive rows fall
    into 4 of the sample's 64-row groups, so a bound taken from the k-th best group with k <= 4 is the one a counted dead row spoils."""
    rows, qs, alive = planted_dead
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(len(rows), dtype=np.uint64), rows)
    for r in np.nonzero(~alive)[0]:
        assert ix.remove(int(r))
    for k in (10, 64, 2):
        nq_l, unproven = check(ix, qs, k, oracle(ix, metric, rows, qs, k, alive=alive))
        print(f"{metric} k = {k}: (queries, unproven) = {(nq_l, unproven)}")
        assert (nq_l, unproven) == (96, 0), f"{unproven} unproven queries at k = {k}"
    ix.close()


# ---- 3. the best rows packed into few sample groups --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed(gpu_required):
    """300 near-copies of query 0 in rows 512 .. 811 (inside the sample: a handful of its groups hold them all), 200 of query 1 in rows
    40 100 .. 40 299 (outside it)"""
    rng = np.random.default_rng(6001)
    n = 70_003
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((96, DIM), dtype=np.float32)
    rows[512:812] = qs[0] + 0.05 * rng.standard_normal((300, DIM)).astype(np.float32)
    rows[40_100:40_300] = qs[1] + 0.05 * rng.standard_normal((200, DIM)).astype(np.float32)
    return rows, qs


@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct, DM.Euclidean])
def test_best_rows_packed_into_few_sample_groups(packed, metric):
    """at k = 128 the k-th best group maximum is far weaker than the k-th best row (query 0's 300 best rows sit in ~10 groups): the
    first bound is loose, and the lists must still hold every candidate"""
    rows, qs = packed
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(len(rows), dtype=np.uint64), rows)
    for k in (10, 64, 128):
        check(ix, qs, k, oracle(ix, metric, rows, qs, k))
    ix.close()


# ---- 4. non-finite rows in the sample range ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct])
def test_non_finite_rows_in_the_sample_range(gpu_required, metric):
    """a NaN component, an inf component and a norm of 1e30 among the first 256 rows (the first row tile of the sample): a NaN score
    drops out of a group's maximum, a +inf score closes the query's bound and the gathered exact pass answers it — the oracle's answer
    either way"""
    rng = np.random.default_rng(808)
    n = 66_000
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((96, DIM), dtype=np.float32)
    rows[17, 5] = np.nan
    rows[130, 700] = np.inf
    rows[201] *= np.float32(1e30 / np.linalg.norm(rows[201].astype(np.float64)))
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(n, dtype=np.uint64), rows)
    check(ix, qs, 10, oracle(ix, metric, rows, qs, 10))
    ix.close()
