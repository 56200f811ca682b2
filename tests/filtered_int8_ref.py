"""What the tests of the filtered graph walk over the u8 codes (vdb_hip_index_search_graph_filters_int8) share: the
reference, the worlds and the whole-call protocol.  No new oracle code: links from an oracle graph, codes from po.ScalarQuantizer,
exact distances from po.batch_distance(.., MODE_C); the walk itself is tests/filtered_walk_ref.py, unchanged.

The walk's distances are INTEGERS: d8(r) = the L2^2 between the quantised query and row r's codes.  filtered_walk_ref orders f32
values, so CodeGraph.dist hands it the integer as the f32 WITH THAT BIT PATTERN (`d.astype(np.uint32).view(np.float32)`): for
integers below 0x7F800000 — a 1024-dimension L2^2 is below 2^27 — the order of those floats, denormals included, is the order of the
integers, ties are ties, and fw.tkey is a bit cast of them.  Never by value: float(d) rounds above 2^24 (CodeGraph(by_value=True)
does exactly that, for the test that shows the difference).

Steps 1-4 of the call for one query (dual_precision.rs:223-441 with the allow-list inside the walk):
  1. ef_s = ef_search or Balanced max(128, 4k); cand_k = k * ratio; ef_w = max(ef_s, cand_k)
  2. qc = quantize(q); greedy descent unfiltered over d8
  3. layer 0 = the filtered search_layer over d8 at ef_w, keys (d8, row)
  4. the first min(cand_k, results) allowed entries re-scored with the exact f32 engine distance, stable-sorted by total_cmp, cut
     to k.  n_dist counts int8 evaluations only.
The exact pass is filtered_walk_ref.exact_pass over the f32 rows.
"""
import os

import numpy as np

import filtered_walk_ref as fw
from oracle import pyoracle as po

BASE = "native_hnsw"
NQ = 8
COSINE, EUCLIDEAN, DOT = 0, 1, 2           # the library's metric codes
PO_METRIC = {COSINE: po.COSINE, EUCLIDEAN: po.EUCLIDEAN, DOT: po.DOT}
METRICS = [COSINE, EUCLIDEAN, DOT]
PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
ROUTE_AUTO, ROUTE_WALK, ROUTE_EXACT = 0, 1, 2
KEF = [(10, 64), (1, 16), (25, 50), (10, 300)]
# (n, dim, M, efc): the generic layout with a tail word (CPL 0, 10 code words); CPL 1 / 2 / 3 / 4 (1024 = the walk's limit); generic
# just under the limit (250 code words: a partial fourth word per lane)
SHAPES = [(1200, 37, 6, 40), (1500, 256, 8, 60), (1500, 512, 8, 60), (1500, 768, 8, 60), (1500, 1024, 8, 60), (1200, 1000, 8, 60)]
CONST_DIM_SHAPE = SHAPES[0]  # the world whose dimension 0 is constant: the quantiser's scale falls back to 1.0


def widths(k, ef, ratio):
    """-> (cand_k, ef_w)"""
    ef_s = max(128, 4 * k) if ef == 0 else ef
    return k * ratio, max(ef_s, k * ratio)


class CodeGraph(fw.Graph):
    """fw.Graph whose `dist(qc, nodes)` is the integer L2^2 between the query's codes qc and the rows' codes, bit-cast to f32;
    `.f32` is the plain graph over the f32 rows (same links) for the re-score and the exact pass"""

    def __init__(self, g, rows, metric, sq, codes, by_value=False):
        super().__init__(g, rows, metric)
        self.sq, self.codes, self.by_value = sq, np.ascontiguousarray(codes, dtype=np.uint8).astype(np.int64), by_value
        self.f32 = fw.Graph(g, rows, metric)
        self.f32._links = self._links

    def dist(self, qc, nodes):
        if len(nodes) == 0:
            return np.empty(0, dtype=np.float32)
        diff = self.codes[np.asarray(nodes, dtype=np.int64)] - np.asarray(qc, dtype=np.int64)[None, :]
        d = (diff * diff).sum(axis=1)
        assert d.max() < 0x7F800000
        if self.by_value:
            return d.astype(np.float32)  # WRONG on purpose: rounds above 2^24
        return d.astype(np.uint32).view(np.float32)


def d8_of(dists):
    """the integers behind CodeGraph's bit-cast distances"""
    return np.asarray(dists, dtype=np.float32).view(np.uint32)


def rescore(G, q, nodes, k):
    """step 4: exact f32 engine distances of the coarse candidates, stable sort by total_cmp, cut to k -> (ids, dists)"""
    nodes = [int(n) for n in nodes]
    ds = G.f32.dist(q, nodes)
    order = sorted(range(len(nodes)), key=lambda i: fw.tkey(ds[i]))  # (stable: equal exact distances keep the coarse order)
    return [nodes[i] for i in order[:k]], [ds[i] for i in order[:k]]


def walk(G, q, k, ef, ratio, allowed, cap):
    """steps 1-4, the kernel's single-list form -> (ids, exact dists, n_dist, n_expand, overflow, info)"""
    cand_k, ef_w = widths(k, ef, ratio)
    qc = G.sq.quantize(q)[0]
    r = fw.walk_single_list(G, qc, cand_k, ef_w, allowed, cap)
    ids, ds = rescore(G, q, r[0], k)
    return ids, ds, r[2], r[3], r[4], r[5]


def walk_two_heap(G, q, k, ef, ratio, allowed):
    """steps 1-4 as the reference writes layer 0: two heaps -> (ids, exact dists, n_dist, n_expand)"""
    cand_k, ef_w = widths(k, ef, ratio)
    qc = G.sq.quantize(q)[0]
    r = fw.walk_two_heap(G, qc, cand_k, ef_w, allowed)
    ids, ds = rescore(G, q, r[0], k)
    return ids, ds, r[2], r[3]


def protocol(G, q, k, ef, ratio, allowed, first, cap_max):
    """one query on the walk / auto route: the walk at `first`, four times the room while it overflows, up to cap_max
    -> (result of the last attempt, overflowed at cap_max)"""
    cap = first
    while True:
        r = walk(G, q, k, ef, ratio, allowed, cap)
        if not r[4] or cap >= cap_max:
            return r, r[4]
        cap = min(4 * cap, cap_max)


def expect_call(G, qs, allowed, k, ef, ratio, route, max_list=0, matched=None):
    """the whole call -> (ids, score bits, routes, (n_dist, n_expand)); asserts nothing.  allowed = filter AND live; matched = the rows
    in the filter (what sizes the list), when that differs.  Without max_list the largest list is taken as unbounded: the callers
    assert that no query overflows."""
    _, ef_w = widths(k, ef, ratio)
    matched = int(allowed.sum()) if matched is None else matched
    ids, sbits, routes, nd, ne = [], [], [], 0, 0
    cap_max = max_list if max_list else 1 << 30
    sized = fw.sized_list(ef_w, matched, G.n) if matched else None
    whole_exact = route == ROUTE_EXACT or (route == ROUTE_AUTO and (matched < ef_w or sized > cap_max))
    for q in qs:
        over = True
        if not whole_exact:
            r, over = protocol(G, q, k, ef, ratio, allowed, min(sized, cap_max), cap_max)
            nd, ne = nd + r[2], ne + r[3]
        if over:
            e = fw.exact_pass(G.f32, q, k, allowed)
            r, nd = (e[0], e[1]), nd + e[2]
        ids.append(list(r[0]))
        sbits.append(fw.score_bits(G.metric, r[1]))
        routes.append(2 if over else 1)
    return ids, sbits, routes, (nd, ne)


def assert_call(got, want, ctx):
    """got = ((ids, scores, counts), routes, stats) of the GPU call: ids, score bits, counts, padding, routes and counters"""
    (ids, sc, cnt), routes, stats = got
    wi, wb, wr, ws = want
    assert routes.tolist() == wr, ctx
    for qi in range(len(wi)):
        c = int(cnt[qi])
        assert c == len(wi[qi]) and ids[qi, :c].tolist() == wi[qi], (ctx, qi)
        assert np.array_equal(sc[qi, :c].view(np.uint32), wb[qi]), (ctx, qi)
        assert np.all(ids[qi, c:] == PAD_ID) and np.all(sc[qi, c:].view(np.uint32) == 0x7FC00000), (ctx, qi)
    assert tuple(stats) == tuple(ws), (ctx, stats, ws)


def build_graph(rows, metric, M, efc):
    g = po.NativeHnsw(rows.shape[1], PO_METRIC[metric], M, efc, po.MODE_C)
    g.set_build_tie(po.TIE_CANONICAL)
    for v in rows:
        g.insert(v)
    return g


class World:
    """Gaussian rows and queries, the oracle graph on them (canonical build ties), the quantiser trained on the first min(1000, n)
    rows as DualPrecisionHnsw trains it, the codes, the named filters.  root: where to dump the graph for a GPU handle (None: no dump)"""

    def __init__(self, root, metric, shape, const_dim=False):
        n, dim, M, efc = shape
        self.metric, self.shape, self.n, self.dim = metric, shape, n, dim
        rng = np.random.default_rng(7000 + 100 * metric + n + dim)
        self.rows = rng.standard_normal((n, dim)).astype(np.float32)
        if const_dim:
            self.rows[:, 0] = 1.5  # scale must fall back to 1.0 (quantization.rs:219-221), as tests/test_gpu_int8.py
        self.qs = rng.standard_normal((NQ, dim)).astype(np.float32)
        self.g = build_graph(self.rows, metric, M, efc)
        self.sq = po.ScalarQuantizer(self.rows[:1000])
        self.codes = self.sq.quantize(self.rows)
        self.G = CodeGraph(self.g, self.rows, PO_METRIC[metric], self.sq, self.codes)
        if root is not None:
            self.dir = os.path.join(root, f"m{metric}_{n}_{dim}")
            os.makedirs(self.dir)
            self.g.file_dump(self.dir, BASE)
        frng = np.random.default_rng(n + dim + 1)
        self.filters = {"all": np.ones(n, dtype=bool), "half": fw.random_filter(frng, n, 0.5), "tenth": fw.random_filter(frng, n, 0.1),
                        "clustered": self.rows[:, 1] > 0.0, "few": fw.random_filter(frng, n, 40 / n)}


# ---- the overflow case: an end-clustered filter and shifted queries (tests/test_gpu_filtered_graph.py's recipe) ---------------------
def overflow_case(w, k, ef, ratio):
    """-> (allowed, queries, max_list, over): a largest list, chosen from the peaks the reference's lists reach when nothing bounds
    them, that some but not all of the queries overflow; max_list None when no size splits them"""
    allowed = np.zeros(w.n, dtype=bool)
    allowed[np.argsort(w.rows[:, 1])[-w.n // 10:]] = True
    qs = w.qs.copy()
    qs[:, 1] += np.resize(np.array([30, -30, 0, -4, -8, -2], dtype=np.float32), NQ)
    _, ef_w = widths(k, ef, ratio)
    sized = fw.sized_list(ef_w, int(allowed.sum()), w.n)
    peaks = sorted({fw.round64(walk(w.G, q, k, ef, ratio, allowed, 1 << 30)[5]["peak"]) for q in qs})
    for max_list in peaks:
        if max_list < sized:  # (below `sized` the auto rule sends the whole call to the exact pass)
            continue
        over = [protocol(w.G, q, k, ef, ratio, allowed, sized, max_list)[1] for q in qs]
        if 0 < sum(over) < len(qs):
            return allowed, qs, max_list, over
    return allowed, qs, None, None


# ---- integers beyond 2^24, and ties -------------------------------------------------------------------------------------------------
BIG_SHAPE = (1200, 1024, 8, 60)
# (ratio 1: ef_w = 64 and the cut to cand_k = 40 of the 64 results is made in COARSE order, so the order of the integers shows in the
# ids; at ratio 4 every result is re-scored and a wrong coarse order would hide behind the exact sort)
BIG_K, BIG_EF, BIG_RATIO = 40, 64, 1


class BigWorld:
    """Euclidean 1200 x 1024: rows drawn from 40 centres with entries +-3.0, their first 16 dimensions set to 3.0 - j * 6 / 255 with
    j in 0..3; rows 0 and 1 are all -3.0 and all +3.0, so the training sample spans the range and a code step is 6 / 255.  Queries are
    centres with the first 16 dimensions at -3.0: a row of another centre lies about 500 * 255^2 > 2^24 away, rows of one centre
    differ by a few units in a distance of eight digits, and many tie."""

    def __init__(self, root):
        n, dim, M, efc = BIG_SHAPE
        self.metric, self.shape, self.n, self.dim = EUCLIDEAN, BIG_SHAPE, n, dim
        rng = np.random.default_rng(4242)
        centres = np.where(rng.random((40, dim)) < 0.5, np.float32(-3.0), np.float32(3.0)).astype(np.float32)
        self.rows = centres[rng.integers(0, 40, n)].copy()
        self.rows[:, :16] = (3.0 - rng.integers(0, 4, (n, 16)) * 6.0 / 255.0).astype(np.float32)
        self.rows[0, :], self.rows[1, :] = -3.0, 3.0
        self.qs = centres[rng.choice(40, NQ, replace=False)].copy()
        self.qs[:, :16] = -3.0
        self.g = build_graph(self.rows, EUCLIDEAN, M, efc)
        self.sq = po.ScalarQuantizer(self.rows[:1000])
        self.codes = self.sq.quantize(self.rows)
        self.G = CodeGraph(self.g, self.rows, po.EUCLIDEAN, self.sq, self.codes)
        self.G_by_value = CodeGraph(self.g, self.rows, po.EUCLIDEAN, self.sq, self.codes, by_value=True)
        self.G_by_value._links = self.G._links
        if root is not None:
            self.dir = os.path.join(root, "big")
            os.makedirs(self.dir)
            self.g.file_dump(self.dir, BASE)
        self.allowed = fw.random_filter(np.random.default_rng(4243), n, 0.5)
