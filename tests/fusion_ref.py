"""FusionStrategy::fuse (fusion/strategy.rs:138-300) and the over-fetch rule of multi_query_search (collection/search/batch.rs:270-275),
restated in numpy float32 — the reference of tests/test_fusion_cpu.py and tests/test_gpu_fusion.py.

Written from the reference's text the way the other *_ref.py helpers are: the same maps in the same order (a per-query map for the
in-query de-duplication, a per-document list of scores pushed query after query), every f32 operation a numpy float32 operation so
that each one is rounded on its own.  Where the reference leaves something open, this file fixes it the way the product declares it:
  * equal fused scores come out by id ascending (the reference: HashMap iteration order);
  * `f32::max` is taken as the maximum in the IEEE total order (identical for scores that are not NaN and do not mix +0.0 / -0.0
    under one id; both are outside the contract);
  * `scores.iter().sum::<f32>()` is a left fold that starts at the first term.
A strategy is a tuple: ("average",), ("maximum",), ("rrf", k), ("weighted", avg, max, hit).
"""
import numpy as np

F = np.float32
MAX_VECTORS = 10
NEG_INF = F(-np.inf)


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def total_key(x) -> int:
    """u32 whose unsigned order is f32::total_cmp's"""
    b = bits(F(x))
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def fmax(a, b):
    return b if total_key(b) > total_key(a) else a


def overfetch(top_k: int) -> int:
    if top_k <= 10:
        return top_k * 20
    if top_k <= 50:
        return top_k * 10
    if top_k <= 100:
        return top_k * 5
    return top_k * 2


def weighted_error(avg, mx, hit):
    """FusionStrategy::weighted: None when valid, else "negative" / "sum" (NaN weights: "sum" — refused here, let through there)"""
    a, m, h = F(avg), F(mx), F(hit)
    if np.isnan(a) or np.isnan(m) or np.isnan(h):
        return "sum"
    if a < 0 or m < 0 or h < 0:
        return "negative"
    s = F(F(a + m) + h)
    return "sum" if np.abs(F(s - F(1.0))) > F(0.001) else None


def _query_best(results):
    """per query: {id: best score} in first-occurrence order, and {id: first rank}"""
    out = []
    for query_results in results:
        best, rank = {}, {}
        for r, (i, s) in enumerate(query_results):
            i, s = int(i), F(s)
            if i in best:
                best[i] = fmax(best[i], s)
            else:
                best[i] = s
                rank[i] = r
        out.append((best, rank))
    return out


def _sum(scores):
    acc = scores[0]
    for s in scores[1:]:
        acc = F(acc + s)
    return acc


def fuse(strategy, results):
    """-> [(id, fused score as np.float32)], descending by total order, ties by id ascending"""
    if len(results) == 0 or all(len(r) == 0 for r in results):
        return []
    total_queries = len(results)
    kind = strategy[0]
    per_query = _query_best(results)
    fused = {}
    if kind == "maximum":
        for best, _ in per_query:
            for i, s in best.items():
                fused[i] = fmax(fused[i], s) if i in fused else s
    elif kind == "rrf":
        k_f32 = F(strategy[1])
        for _, rank in per_query:
            for i, r in rank.items():
                fused[i] = F(fused.get(i, F(0.0)) + F(F(1.0) / F(k_f32 + F(r + 1))))
    else:
        doc_scores = {}
        for best, _ in per_query:
            for i, s in best.items():
                doc_scores.setdefault(i, []).append(s)
        for i, scores in doc_scores.items():
            avg = F(_sum(scores) / F(len(scores)))
            if kind == "average":
                fused[i] = avg
            else:
                assert kind == "weighted"
                aw, mw, hw = F(strategy[1]), F(strategy[2]), F(strategy[3])
                mx = NEG_INF
                for s in scores:
                    mx = fmax(mx, s)
                hit = F(F(len(scores)) / F(total_queries))
                fused[i] = F(F(F(aw * avg) + F(mw * mx)) + F(hw * hit))
    return sorted(fused.items(), key=lambda t: (-total_key(t[1]), t[0]))


def fuse_top(strategy, results, top_k):
    """(ids u64 [max(top_k, 1)], score bits u32, n) as the library pads them: id 2^64 - 1, NaN 0x7FC00000"""
    f = fuse(strategy, results)[:top_k]
    kk = max(top_k, 1)
    ids = np.full(kk, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    sb = np.full(kk, 0x7FC00000, dtype=np.uint32)
    for j, (i, s) in enumerate(f):
        ids[j] = i
        sb[j] = bits(F(s))
    return ids, sb, len(f)
