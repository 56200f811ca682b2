"""What the tests of the filtered graph walk over the half-precision images (vdb_hip_index_search_graph_filters_half)
share: worlds and the whole-call reference.

The walk's distances are the plain half walk's (tests/half_walk_ref.py): over an image H they are bit for bit the mode-C distances
between the f32 vectors dequant(H) and the rounded query.  So the reference of the filtered half walk is tests/filtered_walk_ref.py
over an oracle graph with the SAME links and ROUNDED vectors (half_walk_ref.patch_vectors + load_graph), asked with rounded queries;
the GPU side gets the unrounded queries and rounds them itself.  No new oracle code, no tolerances.
"""
import os

import numpy as np

import filtered_walk_ref as fw
import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po

BASE = "native_hnsw"
NQ = hw.NQ
PRECISIONS = [hr.F16, hr.BF16]
METRICS = [hr.COSINE, hr.EUCLIDEAN, hr.DOT]
PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
ROUTE_AUTO, ROUTE_WALK, ROUTE_EXACT = 0, 1, 2


def half_graph(src_dir, precision, metric, dim):
    """the dump in src_dir with its vectors rounded to `precision`, loaded: -> filtered_walk_ref.Graph (same links, rounded rows)"""
    d = f"{src_dir}_p{precision}"
    rounded = hw.patch_vectors(src_dir, d, BASE, precision)
    g_half = hw.load_graph(d, BASE, metric, dim)
    return fw.Graph(g_half, rounded, hw.PO_METRIC[metric])


class View:
    """one precision of a world: the reference graph over the rounded rows and the rounded queries"""

    def __init__(self, world, precision):
        self.precision, self.metric, self.n = precision, hw.PO_METRIC[world.metric], world.n
        self.G = half_graph(world.dir, precision, world.metric, world.dim)
        self.g_half = self.G.g
        self.qs = hr.round_half(world.qs, precision)


class World:
    """Gaussian rows and queries, the oracle graph on the f32 rows (canonical build ties), its dump, the five named filters and —
    made by the caller — the GPU handle that loaded the dump"""

    def __init__(self, root, metric, shape):
        n, dim, M, efc = shape
        self.metric, self.shape, self.n, self.dim = metric, shape, n, dim
        rng = np.random.default_rng(9000 + 100 * metric + n + dim)
        self.rows = rng.standard_normal((n, dim)).astype(np.float32)
        self.qs = rng.standard_normal((NQ, dim)).astype(np.float32)
        g = po.NativeHnsw(dim, hw.PO_METRIC[metric], M, efc, po.MODE_C)
        g.set_build_tie(po.TIE_CANONICAL)
        for v in self.rows:
            g.insert(v)
        self.dir = os.path.join(root, f"m{metric}_{n}_{dim}")
        os.makedirs(self.dir)
        g.file_dump(self.dir, BASE)
        frng = np.random.default_rng(n + dim + 1)
        self.filters = {"all": np.ones(n, dtype=bool), "half": fw.random_filter(frng, n, 0.5), "tenth": fw.random_filter(frng, n, 0.1),
                        "clustered": self.rows[:, 0] > 0.0, "few": fw.random_filter(frng, n, 40 / n)}
        self._views = {}

    def view(self, precision):
        if precision not in self._views:
            self._views[precision] = View(self, precision)
        return self._views[precision]


def protocol(G, q, k, ef_eff, allowed, first, cap_max):
    """one query on the walk / auto route: the walk at `first`, four times the room while it overflows, up to cap_max.
    -> (form (b) result of the last attempt, overflowed at cap_max)"""
    cap = first
    while True:
        r = fw.walk_single_list(G, q, k, ef_eff, allowed, cap)
        if not r[4] or cap >= cap_max:
            return r, r[4]
        cap = min(4 * cap, cap_max)


def expect_call(v, allowed, k, ef, route, max_list=0, matched=None, qs=None):
    """the whole call by the reference over view `v` (anything with G, n, metric, qs — qs ROUNDED) -> (ids, score bits, routes,
    (n_dist, n_expand)); asserts nothing.  allowed = filter AND live; matched = the rows in the filter (what sizes the list), when
    that differs.  Without max_list the largest list is taken as unbounded: the callers assert that no query overflows."""
    G, ef_eff = v.G, fw.ef_rule(k, ef)
    matched = int(allowed.sum()) if matched is None else matched
    ids, sbits, routes, nd, ne = [], [], [], 0, 0
    cap_max = max_list if max_list else 1 << 30
    sized = fw.sized_list(ef_eff, matched, v.n) if matched else None
    whole_exact = route == ROUTE_EXACT or (route == ROUTE_AUTO and (matched < ef_eff or sized > cap_max))
    for q in (v.qs if qs is None else qs):
        over = True
        if not whole_exact:
            r, over = protocol(G, q, k, ef_eff, allowed, min(sized, cap_max), cap_max)
            nd, ne = nd + r[2], ne + r[3]
        if over:
            e = fw.exact_pass(G, q, k, allowed)
            r, nd = (e[0], e[1]), nd + e[2]
        ids.append(list(r[0]))
        sbits.append(fw.score_bits(v.metric, r[1]))
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
