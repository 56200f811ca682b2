"""CPU test of tests/shard_merge_ref.py, the references of tests/test_gpu_sharded_modes.py: R-merge (`merge_lists`) against the oracle's
`vo_merge_shard_records` (a stable sort of the wire records) and against ONE `sort_results` call over the concatenation, on lists with
ties inside and across shards, short and empty lists, both zeros, both infinities and NaN of either sign.  The direction of every metric
is read off `sort_results` itself (which of two scores it puts first), not off the product's `mode_higher_is_better`."""
import numpy as np
import pytest

from oracle import pyoracle as po
from velesdb_amd.sharded import pack_records

import shard_merge_ref as smr

SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0, -1.0, 2.5, 1e-45, -1e-45], dtype=np.float32)
NAN_BITS = np.array([0x7FC00000, 0xFFC00000], dtype=np.uint32).view(np.float32)   # +NaN sorts past +inf, -NaN before -inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def direction(metric):
    """True when sort_results puts the larger of two scores first"""
    return po.sort_results(metric, [(0, 1.0), (1, 2.0)])[0][0] == 1


def random_lists(rng, S, nq, k, nan):
    pool = np.concatenate([SPECIALS, NAN_BITS]) if nan else SPECIALS
    lists = []
    for s in range(S):
        cnt = rng.integers(0, k + 1, size=nq).astype(np.uint32)
        cnt[0] = k                       # a full list ...
        if nq > 1:
            cnt[1] = 0 if s % 2 else 1   # ... and empty / one-entry ones
        sc = np.where(rng.random((nq, k)) < 0.6, pool[rng.integers(0, len(pool), (nq, k))],
                      rng.standard_normal((nq, k)).astype(np.float32)).astype(np.float32)
        ids = (np.uint64(s) << np.uint64(40)) + rng.permutation(nq * k).astype(np.uint64).reshape(nq, k)   # past 32 bits, unordered
        lists.append((ids, sc, cnt))
    return lists


def test_direction_of_every_metric_comes_from_sort_results():
    assert [direction(m) for m in (po.COSINE, po.EUCLIDEAN, po.DOT, po.HAMMING, po.JACCARD)] == [True, False, True, False, True]
    for m in (po.COSINE, po.EUCLIDEAN, po.DOT, po.HAMMING, po.JACCARD):
        assert direction(m) == po.higher_is_better(m)


def test_total_key_is_total_cmp():
    v = np.concatenate([SPECIALS, NAN_BITS, np.array([3.0e38, -3.0e38, 1.17e-38], dtype=np.float32)])
    key = smr.total_key(v)
    for a in range(len(v)):
        for b in range(len(v)):
            want = po.total_cmp(v[a], v[b]) if not (np.isnan(v[a]) or np.isnan(v[b])) else None
            got = int(np.sign(key[a] - key[b]))
            if want is not None:   # (a NaN does not survive the float argument of vo_total_cmp with its sign: checked below instead)
                assert got == want, (v[a], v[b])
    assert key[-5] > smr.total_key(np.float32(np.inf)) and key[-4] < smr.total_key(np.float32(-np.inf))   # +NaN last, -NaN first
    assert smr.total_key(np.float32(-0.0)) < smr.total_key(np.float32(0.0))


@pytest.mark.parametrize("metric", [po.COSINE, po.EUCLIDEAN, po.DOT, po.HAMMING, po.JACCARD])
@pytest.mark.parametrize("S,nq,k", [(1, 3, 1), (2, 5, 10), (3, 9, 25), (4, 4, 128), (8, 6, 7)])
@pytest.mark.parametrize("nan", [False, True])
def test_merge_lists_equals_the_oracles_merge_and_one_stable_sort(metric, S, nq, k, nan):
    rng = np.random.default_rng(1000 * metric + 10 * S + k + int(nan))
    hib = direction(metric)
    lists = random_lists(rng, S, nq, k, nan)
    gi, gs, gc = smr.merge_lists(lists, k, hib)
    # the oracle's merge over the wire records of the same lists
    rec = np.stack([pack_records(i, s, c).view(np.uint32).reshape(nq, k, 3) for i, s, c in lists])
    oi, osc, oc = po.merge_shard_records(rec, k, hib)
    assert np.array_equal(gc, oc)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gs), bits(osc))       # whole arrays: the filler is the oracle's too
    # one stable sort of the concatenation (DistanceMetric::sort_results)
    for q in range(nq):
        concat = [(int(i[q, p]), s[q, p]) for i, s, c in lists for p in range(int(c[q]))]
        exp = po.sort_results(metric, concat)[:k]
        assert int(gc[q]) == len(exp) == min(k, len(concat))
        assert gi[q, :len(exp)].tolist() == [a for a, _ in exp]
        eb = bits(np.array([b for _, b in exp], dtype=np.float32))
        assert np.array_equal(bits(gs[q, :len(exp)]), eb)
        assert np.all(gi[q, len(exp):] == smr.FILL_ID) and np.all(bits(gs[q, len(exp):]) == smr.FILL_BITS)


def test_merge_lists_ties_keep_shard_then_position_order():
    one = np.ones((1, 3), dtype=np.float32)
    lists = [(np.array([[10, 11, 12]], dtype=np.uint64), one, np.array([3], dtype=np.uint32)),
             (np.array([[20, 21, 22]], dtype=np.uint64), one, np.array([2], dtype=np.uint32)),
             (np.array([[30, 31, 32]], dtype=np.uint64), np.array([[2.0, 1.0, 0.0]], dtype=np.float32), np.array([3], dtype=np.uint32))]
    for hib, want in ((False, [32, 10, 11, 12, 20, 21, 31, 30]), (True, [30, 10, 11, 12, 20, 21, 31, 32])):
        ids, sc, cnt = smr.merge_lists(lists, 10, hib)
        assert cnt[0] == 8 and ids[0, :8].tolist() == want and np.all(ids[0, 8:] == smr.FILL_ID)
    zeros = [(np.array([[1, 2]], dtype=np.uint64), np.array([[0.0, -0.0]], dtype=np.float32), np.array([2], dtype=np.uint32)),
             (np.array([[3, 4]], dtype=np.uint64), np.array([[-0.0, 0.0]], dtype=np.float32), np.array([2], dtype=np.uint32))]
    assert smr.merge_lists(zeros, 4, False)[0][0].tolist() == [2, 3, 1, 4]     # -0.0 before +0.0
    assert smr.merge_lists(zeros, 4, True)[0][0].tolist() == [1, 4, 2, 3]


def test_shard_ranges_is_the_range_rule():
    assert smr.shard_ranges(3000, 3, 3000) == [(0, 1000), (1000, 2000), (2000, 3000)]
    assert smr.shard_ranges(4000, 4, 1100) == [(0, 1000), (1000, 1100), (1100, 1100), (1100, 1100)]
    assert smr.shard_ranges(23, 4, 23) == [(0, 6), (6, 12), (12, 18), (18, 23)]
    assert smr.shard_ranges(102, 2, 101) == [(0, 51), (51, 101)]
    assert smr.shard_ranges(100, 2, 130) == [(0, 50), (50, 130)]               # past S * C: the last shard takes the rest
    assert smr.shard_ranges(0, 2, 3) == [(0, 1), (1, 3)]


def test_pad_lists_and_lists_of_tuples():
    ids, sc, cnt = smr.pad_lists(np.array([[7, 8]], dtype=np.uint64), np.array([[1.0, 2.0]], dtype=np.float32), [2], 4)
    assert ids[0].tolist() == [7, 8, int(smr.FILL_ID), int(smr.FILL_ID)] and bits(sc)[0, 2:].tolist() == [0x7FC00000] * 2 and cnt[0] == 2
    ids, sc, cnt = smr.lists_of_tuples([[(5, 0.5)], []], 3)
    assert cnt.tolist() == [1, 0] and ids[0, 0] == 5 and sc[0, 0] == np.float32(0.5)
