"""numpy-float32 restatement of Collection::hybrid_search (collection/search/text.rs:113-203) and hybrid_search_with_filter
(text.rs:221-299) over id lists: what tests/test_hybrid_cpu.py holds the product's rule (csrc/vdb_hybrid.hpp through
tests/hybrid_model.cpp) to, and what tests/test_gpu_hybrid.py holds the kernel to.  Written after the reference's own text: a dict in
insertion order for the fused scores, a heap of size k on (score, id) for the cut, a sort of the survivors.

The two stated deviations are restated here as the product states them:
  * the order among equal fused scores — unspecified in the reference (a stable sort of a heap's drain) — is id descending, the order
    consistent with the heap's membership key;
  * the filtered form drops text hits outside (filter AND live) BEFORE ranks are assigned; the reference post-filters behind the sort;
  * a NaN weight is refused (ValueError).
"""
import heapq

import numpy as np

F = np.float32
PAD_ID, PAD_SCORE = 0xFFFFFFFFFFFFFFFF, 0x7FC00000
MAX_RECORDS = 8192


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def total_key(x):
    """int whose order is f32::total_cmp's"""
    b = bits(x)
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def clamp_weight(vector_weight=None):
    """vector_weight.unwrap_or(0.5).clamp(0.0, 1.0) in f32 (text.rs:133); NaN is refused"""
    w = F(0.5) if vector_weight is None else F(vector_weight)
    if np.isnan(w):
        raise ValueError("vector_weight is NaN")
    if w < F(0.0):
        return F(0.0)
    if w > F(1.0):
        return F(1.0)
    return w


def fused_scores(V, T, w):
    """text.rs:144-162: {id: fused score} in insertion order; every occurrence adds"""
    tw = F(F(1.0) - w)
    fused = {}
    with np.errstate(all="ignore"):
        for weight, ids in ((w, V), (tw, T)):
            for rank, i in enumerate(ids):
                rrf = F(weight / F(F(rank) + F(60.0)))
                fused[int(i)] = F(fused.get(int(i), F(0.0)) + rrf)
    return fused


def cut(fused, k):
    """text.rs:166-180: a min-heap of size k on (score, id) keeps the k largest; then descending by score — equal scores by id
    descending (the stated order)"""
    heap = []
    for i, s in fused.items():
        heapq.heappush(heap, (total_key(s), i, s))
        if len(heap) > k:
            heapq.heappop(heap)
    return [(i, s) for _, i, s in sorted(heap, key=lambda e: (e[0], e[1]), reverse=True)]


def hybrid(V, T, k, vector_weight=None, live=None):
    """hybrid_search: [(id, fused score)], best first.  live(id) -> bool: the id is in the vector storage (None: every id is)"""
    out = cut(fused_scores(V, T, clamp_weight(vector_weight)), k)
    return [(i, s) for i, s in out if live is None or live(i)]      # text.rs:186-200: behind the cut


def hybrid_filtered(V, T, k, vector_weight, keep):
    """hybrid_search_with_filter as the product states it: V is the in-walk allow-list's list, keep(id) -> the id's row is known, live
    and inside the filter; text hits that are not kept take no rank"""
    return cut(fused_scores(V, [t for t in T if keep(int(t))], clamp_weight(vector_weight)), k)


def top(pairs, k):
    """[(id, score)] -> (ids u64, score bits u32, n) padded to max(k, 1) as the library pads"""
    kk = max(k, 1)
    ids = np.full(kk, PAD_ID, dtype=np.uint64)
    sb = np.full(kk, PAD_SCORE, dtype=np.uint32)
    for j, (i, s) in enumerate(pairs):
        ids[j], sb[j] = i, bits(s)
    return ids, sb, len(pairs)
