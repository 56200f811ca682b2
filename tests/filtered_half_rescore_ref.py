"""What the tests of the half-precision filtered walk with the exact f32 re-score (vdb_hip_index_search_graph_filters_half_rescore,
DESIGN 4.1m) share: the reference, the worlds and the whole-call protocol.  No new oracle code and no tolerances — everything is
built from what exists:

  * the walk: tests/filtered_walk_ref.py over the graph of tests/filtered_half_world.half_graph (the handle's links, the rows
    ROUNDED to the precision), asked with the ROUNDED query at (cand_k, ef_w);
  * the re-score: fw.Graph over the f32 rows with the UNROUNDED query (the `rescore` of tests/filtered_int8_ref.py);
  * the exact pass: fw.exact_pass over that f32 graph;
  * the whole-call protocol: that of filtered_int8_ref.expect_call.

Steps 1-4 of the call for one query:
  1. ef_s = ef_search or Balanced max(128, 4k); ratio = oversampling or 4; cand_k = k * ratio; ef_w = max(ef_s, cand_k)
  2. the half walk at ef_w: rounded query against the rows' image, the descent unfiltered, layer 0 the filtered search_layer
  3. the first min(cand_k, results) allowed entries re-scored with the exact f32 engine distance (unrounded query, f32 row),
     stable-sorted by total_cmp — equal exact distances keep the coarse order — and cut to k
  4. n_dist counts the half evaluations only.
"""
import os

import numpy as np

import filtered_half_world as fh
import filtered_walk_ref as fw
import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po

BASE = fh.BASE
NQ = 8
PRECISIONS = fh.PRECISIONS
METRICS = fh.METRICS
PAD_ID = fh.PAD_ID
ROUTE_AUTO, ROUTE_WALK, ROUTE_EXACT = 0, 1, 2
KEF = [(10, 64), (1, 16), (25, 50), (10, 300)]
RATIOS = [1, 4]
FILTERS = ["all", "half", "tenth", "clustered", "few"]
# (n, dim, M, efc): CPL 0 with a tail; CPL 1 / 2 / 3 / 4; generic just under the register layout's limit
SHAPES = [(1200, 37, 6, 40), (1500, 256, 8, 60), (1500, 512, 8, 60), (1500, 768, 8, 60), (1500, 1024, 8, 60), (1200, 1000, 8, 60)]
LDS_BUDGET = 160 * 1024


def widths(k, ef, ratio):
    """-> (cand_k, ef_w)"""
    ratio = ratio or 4
    ef_s = max(128, 4 * k) if ef == 0 else ef
    return k * ratio, max(ef_s, k * ratio)


# ---- the documented LDS layout of a walk launch (include/velesdb_hip.h) ---------------------------------------------------
def lds_bytes(cap, nbmax, dim):
    """list keys [cap] u64 | neighbour ids [nbmax] u32 | neighbour distances [nbmax] f32 | 16 control bytes | flags [cap rounded to 16]
    u8 | f32 query scratch (generic dimensions only: 4 * dim rounded to 16) | pad to 16 | re-score output [nbmax] u64"""
    s = cap * 8 + nbmax * 4 + nbmax * 4 + 16 + (cap + 15) // 16 * 16
    if dim not in (256, 512, 768, 1024):
        s += (dim + 3) // 4 * 16
    s = (s + 15) // 16 * 16
    return s + nbmax * 8


def nbmax_of(longest, cand_k):
    return fw.round64(max(longest, cand_k))


def largest_list(nbmax, dim):
    """the largest multiple of 64 entries whose launch stays within 160 KB"""
    cap = LDS_BUDGET // 9 // 64 * 64
    while cap and lds_bytes(cap, nbmax, dim) > LDS_BUDGET:
        cap -= 64
    return cap


class View:
    """one precision of a world: G = the graph over the rounded rows (the walk), F = the same links over the f32 rows (the re-score
    and the exact pass), qs = the unrounded queries"""

    def __init__(self, world, precision):
        self.precision, self.metric, self.n = precision, hw.PO_METRIC[world.metric], world.n
        self.G = fh.half_graph(world.dir, precision, world.metric, world.dim)
        self.F = fw.Graph(self.G.g, world.rows, self.metric)
        self.F._links = self.G._links
        self.qs = world.qs

    def rounded(self, q):
        return hr.round_half(np.asarray(q, dtype=np.float32), self.precision)


def rescore(F, q, nodes, k):
    """step 3: exact f32 engine distances of the coarse candidates, stable sort by total_cmp, cut to k -> (ids, dists)"""
    nodes = [int(n) for n in nodes]
    ds = F.dist(q, nodes)
    order = sorted(range(len(nodes)), key=lambda i: fw.tkey(ds[i]))  # (stable: equal exact distances keep the coarse order)
    return [nodes[i] for i in order[:k]], [ds[i] for i in order[:k]]


def coarse(v, q, k, ef, ratio, allowed, cap):
    """step 2 alone, the kernel's single-list form -> fw.walk_single_list's tuple at (cand_k, ef_w)"""
    cand_k, ef_w = widths(k, ef, ratio)
    return fw.walk_single_list(v.G, v.rounded(q), cand_k, ef_w, allowed, cap)


def walk(v, q, k, ef, ratio, allowed, cap):
    """steps 1-4, the kernel's single-list form -> (ids, exact dists, n_dist, n_expand, overflow, info)"""
    r = coarse(v, q, k, ef, ratio, allowed, cap)
    ids, ds = rescore(v.F, q, r[0], k)
    return ids, ds, r[2], r[3], r[4], r[5]


def walk_two_heap(v, q, k, ef, ratio, allowed):
    """steps 1-4 as the reference writes layer 0: two heaps -> (ids, exact dists, n_dist, n_expand)"""
    cand_k, ef_w = widths(k, ef, ratio)
    r = fw.walk_two_heap(v.G, v.rounded(q), cand_k, ef_w, allowed)
    ids, ds = rescore(v.F, q, r[0], k)
    return ids, ds, r[2], r[3]


def protocol(v, q, k, ef, ratio, allowed, first, cap_max):
    """one query on the walk / auto route: the walk at `first`, four times the room while it overflows, up to cap_max
    -> (result of the last attempt, overflowed at cap_max)"""
    cap = first
    while True:
        r = walk(v, q, k, ef, ratio, allowed, cap)
        if not r[4] or cap >= cap_max:
            return r, r[4]
        cap = min(4 * cap, cap_max)


def expect_call(v, allowed, k, ef, ratio, route, max_list=0, matched=None, qs=None):
    """the whole call -> (ids, score bits, routes, (n_dist, n_expand)); asserts nothing.  allowed = filter AND live; matched = the rows
    in the filter (what sizes the list), when that differs; qs UNROUNDED.  Without max_list the largest list is taken as unbounded:
    the callers assert that no query overflows."""
    _, ef_w = widths(k, ef, ratio)
    matched = int(allowed.sum()) if matched is None else matched
    ids, sbits, routes, nd, ne = [], [], [], 0, 0
    cap_max = max_list if max_list else 1 << 30
    sized = fw.sized_list(ef_w, matched, v.n) if matched else None
    whole_exact = route == ROUTE_EXACT or (route == ROUTE_AUTO and (matched < ef_w or sized > cap_max))
    for q in (v.qs if qs is None else qs):
        over = True
        if not whole_exact:
            r, over = protocol(v, q, k, ef, ratio, allowed, min(sized, cap_max), cap_max)
            nd, ne = nd + r[2], ne + r[3]
        if over:
            e = fw.exact_pass(v.F, q, k, allowed)
            r, nd = (e[0], e[1]), nd + e[2]
        ids.append(list(r[0]))
        sbits.append(fw.score_bits(v.metric, r[1]))
        routes.append(2 if over else 1)
    return ids, sbits, routes, (nd, ne)


assert_call = fh.assert_call


class World(fh.World):
    """filtered_half_world.World with the first NQ queries and this module's views"""

    def __init__(self, root, metric, shape):
        super().__init__(root, metric, shape)
        self.qs = np.ascontiguousarray(self.qs[:NQ])

    def view(self, precision):
        if precision not in self._views:
            self._views[precision] = View(self, precision)
        return self._views[precision]


# ---- the overflow case: an end-clustered filter and shifted queries (tests/test_gpu_filtered_graph.py's recipe) ---------------------
def overflow_case(w, v, k, ef, ratio):
    """-> (allowed, queries, max_list, over): a largest list, chosen from the peaks the reference's lists reach when nothing bounds
    them, that some but not all of the queries overflow; max_list None when no size splits them"""
    allowed = np.zeros(w.n, dtype=bool)
    allowed[np.argsort(w.rows[:, 0])[-w.n // 10:]] = True
    qs = w.qs.copy()
    qs[:, 0] += np.resize(np.array([30, -30, 0, -4, -8, -2], dtype=np.float32), NQ)
    _, ef_w = widths(k, ef, ratio)
    sized = fw.sized_list(ef_w, int(allowed.sum()), w.n)
    peaks = sorted({fw.round64(walk(v, q, k, ef, ratio, allowed, 1 << 30)[5]["peak"]) for q in qs})
    for max_list in peaks:
        if max_list < sized:  # (below `sized` the auto rule sends the whole call to the exact pass)
            continue
        over = [protocol(v, q, k, ef, ratio, allowed, sized, max_list)[1] for q in qs]
        if 0 < sum(over) < len(qs):
            return allowed, qs, max_list, over
    return allowed, qs, None, None


# ---- TieWorld: coarse distances tie across a whole cluster ----------------------------------------------------------------------------
TIE_SHAPE = (1200, 256, 16, 100)  # (M = 16: with 8 links per node the DotProduct graph reaches one such cluster whole)
TIE_K, TIE_EF = 10, 64
TIE_SEED = 0


class TieWorld:
    """1200 x 256, 40 centres whose entries are drawn from +-{0.25, 0.5, ..., 2.0}; rows = centre[label] + U(-1, 1) * 2^-15, so the
    f16 AND the bf16 image of every row is its centre exactly: the coarse distances tie across a cluster and order by row.  The 8
    queries are centre + 0.01 * N(0, 1).  At ratio 1 the cut to cand_k = k is made in coarse (row) order — a kernel that sorts by
    the exact distance before it cuts answers differently; at ratio 4 the whole cluster is re-scored.

    Which 8 centres: rows this tight link to their own cluster first, so a graph over them leaves some clusters unreachable from
    the entry point, and a cluster of more than 40 rows does not fit cand_k = 40.  The queries sit at the first 8 centres (in
    centre order) whose cluster has at most 37 rows and comes back whole, before any other row, from the REFERENCE's coarse walk at
    ef 64 — a choice made with the reference alone; tests/test_filtered_half_rescore_ref_cpu.py asserts what it buys."""

    def __init__(self, root, metric):
        n, dim, M, efc = TIE_SHAPE
        self.metric, self.shape, self.n, self.dim = metric, TIE_SHAPE, n, dim
        rng = np.random.default_rng(TIE_SEED)
        self.centres = (rng.integers(1, 9, (40, dim)) * 0.25 * rng.choice([-1.0, 1.0], (40, dim))).astype(np.float32)
        self.labels = rng.integers(0, 40, n)
        self.rows = (self.centres[self.labels] + rng.uniform(-1.0, 1.0, (n, dim)) * 2.0 ** -15).astype(np.float32)
        candidates = (self.centres + 0.01 * rng.standard_normal((40, dim))).astype(np.float32)
        g = po.NativeHnsw(dim, hw.PO_METRIC[metric], M, efc, po.MODE_C)
        g.set_build_tie(po.TIE_CANONICAL)
        for r in self.rows:
            g.insert(r)
        self.dir = os.path.join(root, f"tie_m{metric}")
        os.makedirs(self.dir)
        g.file_dump(self.dir, BASE)
        self.filters = {"all": np.ones(n, dtype=bool), "half": fw.random_filter(np.random.default_rng(TIE_SEED + 1), n, 0.5)}
        self._views = {}
        self.qs = candidates  # (View keeps a reference; replaced below)
        v, chosen = self.view(hr.F16), []
        for c in range(40):
            size = int((self.labels == c).sum())
            if size <= 37 and len(chosen) < NQ:
                got = coarse(v, candidates[c], TIE_K, TIE_EF, 4, self.filters["all"], 1 << 30)[0]
                if len(got) >= size and all(self.labels[i] == c for i in got[:size]):
                    chosen.append(c)
        assert len(chosen) == NQ, "fewer than 8 clusters the reference walk reaches whole"
        self.qlabels = np.array(chosen)
        self.qs = np.ascontiguousarray(candidates[chosen])
        v.qs = self.qs

    def view(self, precision):
        if precision not in self._views:
            self._views[precision] = View(self, precision)
        return self._views[precision]
