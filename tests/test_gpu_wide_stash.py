"""GPU parity tests of the WIDE selection's block-local stash (csrc/g16_protocol.inc, csrc/g16_writeout.inc): every survivor of a row
tile goes into its query's slots of the block's LDS stash, an entry that finds them full goes to the query's global list on its own,
and the stash is flushed behind the block's last row tile (one counter update per query, then the keys).  The lists must come out as
they did when every survivor went to the global list: every survivor counted, entries past the list's capacity dropped, a count above
it sending the query to the gathered exact pass.

Bar: ids, ranks and score bits of the exact kernels (oracle mode M; Euclidean: mode C), `last_select_level() == 4`."""
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


def check(ix, metric, rows, qs, k):
    ids, sc, cnt = ix.search_batch_brute_force(qs, k)
    assert ix.last_select_level() == LEVEL_WIDE, f"select level {ix.last_select_level()} served k = {k}"
    if metric == DM.Euclidean:
        mode = po.MODE_C
    else:
        mode = po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C
    eid, esc = po.scan_topk(PO[metric], rows, qs, k, mode, nthreads=po.host_threads())
    assert np.all(cnt == k)
    assert np.array_equal(ids, eid), f"ids / ranks differ from the oracle at k = {k}"
    assert np.array_equal(bits(sc), bits(esc)), f"score bits differ from the oracle at k = {k}"
    return ix.last_split_stats()


@pytest.fixture(scope="module")
def near_copies(gpu_required):
    """3 000 near-copies of query 0 in consecutive rows past the seed sample: every row tile they fill holds 256 survivors of one query
    (20 times a stash row), in the blocks of one launch; 200 of query 1 in one row tile"""
    rng = np.random.default_rng(4242)
    n = 70_003
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((96, DIM), dtype=np.float32)
    rows[20_000:23_000] = qs[0] + 0.05 * rng.standard_normal((3000, DIM)).astype(np.float32)
    rows[40_100:40_300] = qs[1] + 0.05 * rng.standard_normal((200, DIM)).astype(np.float32)
    return rows, qs


@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct, DM.Euclidean])
def test_stash_overflow_inside_one_launch(near_copies, metric):
    rows, qs = near_copies
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(len(rows), dtype=np.uint64), rows)
    for k in (10, 64, 128):
        check(ix, metric, rows, qs, k)
    ix.close()


def test_global_list_overflow_takes_the_gathered_pass(gpu_required):
    """5 000 exact copies of query 0: more survivors than a global list holds — the count says so, the query is unproven and the
    gathered exact pass answers it (ties ranked by id, as the oracle ranks them)"""
    rng = np.random.default_rng(77)
    n = 66_560
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((64, DIM), dtype=np.float32)
    rows[30_000:35_000] = qs[0]
    ix = va.HnswIndex(DIM, DM.Cosine)
    ix.upload(np.arange(n, dtype=np.uint64), rows)
    for k in (10, 100):
        nq_l, unproven = check(ix, DM.Cosine, rows, qs, k)
        assert nq_l == 64 and 1 <= unproven <= 4, f"{unproven} unproven queries at k = {k} (expected: query 0's)"
    ix.close()


@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct])
def test_ragged_rows_and_batches(gpu_required, metric):
    """a corpus that is not a whole number of 256-row tiles, batches of 1 000 and 300 queries (partial query tiles)"""
    rng = np.random.default_rng(31)
    n = 66_001
    rows = rng.standard_normal((n, DIM), dtype=np.float32)
    qs = rng.standard_normal((1000, DIM), dtype=np.float32)
    ix = va.HnswIndex(DIM, metric)
    ix.upload(np.arange(n, dtype=np.uint64), rows)
    for nq, k in ((1000, 10), (300, 10), (300, 50)):
        check(ix, metric, rows, qs[:nq], k)
    ix.close()
