"""What a multi-device handle has to return, stated without it (the references of tests/test_gpu_sharded_modes.py).

  * `shard_ranges`: the range rule of DESIGN 5 — global row r lives on shard min(r / C, S - 1), C = ceil(max_elements / S).
  * `merge_lists` (R-merge): the per-shard result lists concatenated in shard order, ONE stable sort by score in the direction the
    caller names, cut to k, the tail filled like a single-device result (id ~0, score bits 0x7FC00000).  The order of scores is
    f32::total_cmp (NaN, infinities and the two zeros all have their place), restated here on the bit patterns — not taken from the
    product's `vdb_shard_wire.hpp`.  Equal scores keep the concatenation's order = (shard, position in the shard's list) = global
    row order, which is what DistanceMetric::sort_results (a stable sort) gives one index over all rows.
  * `pad_lists`: a k-wide single-device style block from lists that are shorter than k (the oracle's scan over fewer than k rows).

tests/test_shard_merge_ref_cpu.py holds `merge_lists` to the oracle's `vo_merge_shard_records` and to one `sort_results` call."""
import numpy as np

FILL_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
FILL_BITS = np.uint32(0x7FC00000)


def shard_ranges(max_elements, n_shards, n_rows):
    """[lo, hi) of the global rows every shard holds once n_rows rows are inserted (the last shard takes what is past S * C)"""
    c = max(1, (max(int(max_elements), 1) + n_shards - 1) // n_shards)
    out = []
    for s in range(n_shards):
        lo = min(s * c, n_rows)
        hi = n_rows if s == n_shards - 1 else min((s + 1) * c, n_rows)
        out.append((lo, hi))
    return out


def total_key(scores):
    """int64 whose order is f32::total_cmp's: the sign-magnitude bits as a two's complement number"""
    i = np.ascontiguousarray(scores, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, i ^ 0x7FFFFFFF, i)


def pad_lists(ids, scores, counts, k):
    """(ids [nq, <= k], scores, counts) -> k-wide arrays, everything at and past a query's count holding the filler"""
    ids = np.asarray(ids, dtype=np.uint64)
    scores = np.asarray(scores, dtype=np.float32)
    nq = ids.shape[0]
    oi = np.full((nq, k), FILL_ID, dtype=np.uint64)
    ob = np.full((nq, k), FILL_BITS, dtype=np.uint32)
    cnt = np.asarray(counts, dtype=np.uint32).copy()
    for q in range(nq):
        c = int(cnt[q])
        oi[q, :c] = ids[q, :c]
        ob[q, :c] = scores[q, :c].view(np.uint32)
    return oi, ob.view(np.float32), cnt


def merge_lists(lists, k, higher_is_better):
    """R-merge.  lists: per shard, in shard order, (ids [nq, w_s], scores [nq, w_s], counts [nq]) — only the first counts[q] entries
    of a row are read.  Returns (ids [nq, k] u64, scores [nq, k] f32, counts [nq] u32)."""
    nq = len(lists[0][2])
    oi = np.full((nq, k), FILL_ID, dtype=np.uint64)
    ob = np.full((nq, k), FILL_BITS, dtype=np.uint32)
    cnt = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ci = np.concatenate([np.asarray(i, dtype=np.uint64)[q, :int(c[q])] for i, _, c in lists])
        cs = np.concatenate([np.asarray(s, dtype=np.float32)[q, :int(c[q])] for _, s, c in lists])
        key = total_key(cs)
        order = np.argsort(-key if higher_is_better else key, kind="stable")[:k]
        m = len(order)
        oi[q, :m] = ci[order]
        ob[q, :m] = cs[order].view(np.uint32)
        cnt[q] = m
    return oi, ob.view(np.float32), cnt


def lists_of_tuples(results, k):
    """[[(id, score), ...] per query] (what search_batch_parallel / search_with_rerank return) -> (ids, scores, counts) arrays"""
    nq = len(results)
    ids = np.zeros((nq, max(k, 1)), dtype=np.uint64)
    sc = np.zeros((nq, max(k, 1)), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint32)
    for q, r in enumerate(results):
        cnt[q] = len(r)
        for p, (i, s) in enumerate(r):
            ids[q, p], sc[q, p] = i, s
    return ids, sc, cnt
