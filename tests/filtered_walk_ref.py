"""The filtered graph walk (vdb_hip_index_search_graph_filtered) restated in Python over an oracle graph — no new
oracle code: links from `g.neighbors(layer, node)`, distances from `po.batch_distance(metric, q, rows, po.MODE_C)`.

Semantics: NativeHnsw::search (native/graph.rs:251-270) — the greedy descent search_layer_single (graph.rs:405-428) unchanged and
unfiltered, then layer 0 = search_layer (graph.rs:438-520) with ONE change: `results` receives allowed nodes only; `candidates` and
`visited` receive what they receive there.  Heaps are ordered by (total-order(dist), node), the project's canonical tie order.

Two forms of layer 0:
  (a) `walk_two_heap`   as the reference writes it: two heaps;
  (b) `walk_single_list` the kernel's form: ONE sorted list of bounded capacity with two flag bits per entry (expanded, allowed), the
      ef-th allowed entry as the pivot, truncation behind the pivot, and an overflow report when an entry fell off the full list that
      form (a) still needs — an unexpanded candidate, or an allowed entry while the results are not full.
Also the exact pass (a plain sort of batch_distance over the allowed live rows) and `over_fetch`, the reference's post-filter rule
(collection/search/vector.rs:180-215) over `g.search`.
"""
import bisect
import heapq

import numpy as np

from oracle import pyoracle as po

F32_MAX = np.float32(np.finfo(np.float32).max)
EXPANDED, ALLOWED = 1, 2


def tkey(d) -> int:
    """u32 whose unsigned order is f32::total_cmp's"""
    b = int(np.float32(d).view(np.uint32))
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def ef_rule(k, ef):
    """HnswIndex's: 0 = Balanced max(128, 4k); then max(ef, k)"""
    if ef == 0:
        ef = max(128, 4 * k)
    return max(ef, k)


def round64(v):
    return (v + 63) // 64 * 64


def min_list(ef_eff):
    return round64(ef_eff + max(64, ef_eff // 2))


def sized_list(ef_eff, matched, n_rows):
    """the first capacity of the auto / walk route (csrc/vdb_filter_route.hpp fg_sized_list)"""
    return max(round64(2 * ef_eff * n_rows // matched + 64), min_list(ef_eff))


class Graph:
    """links of an oracle graph, fetched once; rows = the vectors the graph was built on"""

    def __init__(self, g, rows, metric):
        self.g, self.rows, self.metric = g, np.ascontiguousarray(rows, dtype=np.float32), metric
        self.n = len(g)
        self.max_layer, self.entry_point = g.max_layer, g.entry_point
        self._links = {}

    def links(self, layer, node):
        key = (layer, node)
        if key not in self._links:
            self._links[key] = self.g.neighbors(layer, node)
        return self._links[key]

    def dist(self, q, nodes):
        if len(nodes) == 0:
            return np.empty(0, dtype=np.float32)
        return po.batch_distance(self.metric, q, self.rows[np.asarray(nodes, dtype=np.int64)], po.MODE_C)


def descent(G, q):
    """search_layer_single on layers max_layer..1 -> (layer-0 entry point, n_dist)"""
    cur, n_dist = G.entry_point, 0
    for layer in range(G.max_layer, 0, -1):
        best_d = G.dist(q, [cur])[0]
        n_dist += 1
        while True:
            nbrs = G.links(layer, cur)
            ds = G.dist(q, nbrs)
            n_dist += len(nbrs)
            improved = False
            for nb, d in zip(nbrs, ds):
                if d < best_d:  # raw compare: NaN never improves
                    cur, best_d, improved = nb, d, True
            if not improved:
                break
    return cur, n_dist


def walk_two_heap(G, q, k, ef, allowed):
    """form (a).  allowed: bool per row (filter AND live).  -> (ids, dists, n_dist, n_expand)"""
    if G.n == 0 or G.entry_point < 0:
        return [], [], 0, 0
    ep, n_dist = descent(G, q)
    visited = {ep}
    d = G.dist(q, [ep])[0]
    n_dist += 1
    n_expand = 0
    cand = [(tkey(d), ep, d)]
    res = []  # max-heap through negated keys
    if allowed[ep]:
        heapq.heappush(res, (-tkey(d), -ep, d))
    while cand:
        _, c, c_dist = heapq.heappop(cand)
        furthest = res[0][2] if res else F32_MAX
        if c_dist > furthest and len(res) >= ef:
            break
        n_expand += 1
        new = [nb for nb in G.links(0, c) if nb not in visited]
        new = list(dict.fromkeys(new))
        visited.update(new)
        ds = G.dist(q, new)
        n_dist += len(new)
        for nb, dn in zip(new, ds):
            furthest = res[0][2] if res else F32_MAX
            if dn < furthest or len(res) < ef:
                heapq.heappush(cand, (tkey(dn), nb, dn))
                if allowed[nb]:
                    heapq.heappush(res, (-tkey(dn), -nb, dn))
                    if len(res) > ef:
                        heapq.heappop(res)
    out = sorted((-a, -b, dd) for a, b, dd in res)[:k]
    return [n for _, n, _ in out], [dd for _, _, dd in out], n_dist, n_expand


def walk_single_list(G, q, k, ef, allowed, cap):
    """form (b), the kernel's.  -> (ids, dists, n_dist, n_expand, overflow, info); info: 'peak' = the longest the list got,
    'lost' = [(node, flags, results_full_after)] for every entry that fell off the full list."""
    info = {"peak": 0, "lost": []}
    if G.n == 0 or G.entry_point < 0:
        return [], [], 0, 0, False, info
    keys, ds, flags = [], [], []  # sorted by key = (tkey, node)
    akeys = []                    # the keys of the allowed entries, sorted: the pivot is akeys[ef - 1]
    dist_of = {}
    state = {"pivot": None, "overflow": False, "scan": 0}  # scan: no unexpanded entry lies in front of this position

    def find_pivot():
        return bisect.bisect_left(keys, akeys[ef - 1]) if len(akeys) >= ef else None

    def forget(key, flag):
        if flag & ALLOWED:
            del akeys[bisect.bisect_left(akeys, key)]

    def admit(d, node):
        flag = ALLOWED if allowed[node] else 0
        key = (tkey(d), node)
        dist_of[node] = d
        pos = bisect.bisect_left(keys, key)
        lost = None
        if pos >= cap:
            lost = (node, flag)
        else:
            if len(keys) == cap:
                lost = (keys[-1][1], flags[-1])
                forget(keys[-1], flags[-1])
                keys.pop(), ds.pop(), flags.pop()
            keys.insert(pos, key), ds.insert(pos, d), flags.insert(pos, flag)
            state["scan"] = min(state["scan"], pos)
            if flag:
                bisect.insort(akeys, key)
        pivot = state["pivot"] = find_pivot()
        if lost is not None:
            info["lost"].append((lost[0], lost[1], pivot is not None))
            if not (lost[1] & EXPANDED) or ((lost[1] & ALLOWED) and pivot is None):
                state["overflow"] = True
        info["peak"] = max(info["peak"], len(keys))
        if pivot is not None:  # entries behind the pivot stay up to the last one that is not further (raw compare: ties stay)
            last = len(keys) - 1
            while last > pivot and ds[last] > ds[pivot]:
                last -= 1
            for e in range(last + 1, len(keys)):
                forget(keys[e], flags[e])
            del keys[last + 1:], ds[last + 1:], flags[last + 1:]

    ep, n_dist = descent(G, q)
    visited = {ep}
    admit(G.dist(q, [ep])[0], ep)
    n_dist += 1
    n_expand = 0
    while True:
        idx = state["scan"]
        while idx < len(flags) and flags[idx] & EXPANDED:
            idx += 1
        state["scan"] = idx
        if idx >= len(flags):
            break
        pivot = state["pivot"]
        if pivot is not None and ds[idx] > ds[pivot]:
            break
        flags[idx] |= EXPANDED
        n_expand += 1
        new = list(dict.fromkeys(nb for nb in G.links(0, keys[idx][1]) if nb not in visited))
        visited.update(new)
        dn = G.dist(q, new)
        n_dist += len(new)
        for nb, d in zip(new, dn):
            pivot = state["pivot"]
            if pivot is None or d < ds[pivot]:
                admit(d, nb)
    out = [(node, dist_of[node]) for _, node in akeys[:k]]
    return [n for n, _ in out], [d for _, d in out], n_dist, n_expand, state["overflow"], info


def exact_pass(G, q, k, allowed):
    """top-k of the allowed rows by (total-order(distance), row) -> (ids, dists, rows evaluated)"""
    rows = np.flatnonzero(allowed)
    ds = G.dist(q, rows)
    order = sorted(range(len(rows)), key=lambda i: (tkey(ds[i]), int(rows[i])))[:k]
    return [int(rows[i]) for i in order], [ds[i] for i in order], len(rows)


def over_fetch(g, q, k, allowed, ef=0):
    """the reference's post-filter rule: max(4k, k + 10) unfiltered candidates at HnswIndex's ef rule, rejected ones dropped, cut to k"""
    kk = max(4 * k, k + 10)
    ids, ds = g.search(q, kk, ef_rule(kk, ef), po.TIE_CANONICAL)
    keep = [(int(i), d) for i, d in zip(ids, ds) if allowed[int(i)]][:k]
    return [i for i, _ in keep], [d for _, d in keep]


def score_bits(metric, dists):
    return np.array([np.float32(po.transform_score(metric, float(d))) for d in dists], dtype=np.float32).view(np.uint32)


def random_filter(rng, n, density):
    """exactly round(n * density) rows, uniformly drawn"""
    allowed = np.zeros(n, dtype=bool)
    allowed[rng.choice(n, max(1, int(round(n * density))), replace=False)] = True
    return allowed
