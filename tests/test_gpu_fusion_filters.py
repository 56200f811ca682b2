"""GPU tests of the multi-query search with one optional filter per group over the rows forms of the walk
(vdb_hip_index_multi_query_search_filters).

The reference is tests/fusion_ref.py, as in tests/test_gpu_fusion.py; everything is compared bit for bit.  The lists the rule is
applied to are the ones the underlying calls of the contract return for the group's vectors ALONE at the over-fetched k: the plain
call of the rows form for an unfiltered group, the call with one filter per query for a filtered one.  The refusals are decided on
the host before a launch.
"""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as fc
import fusion_ref as fr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
INVALID, UNSUPPORTED, STATE = -1, -7, -8
PAD_ID, PAD_SCORE = 0xFFFFFFFFFFFFFFFF, 0x7FC00000

DIM, M, EFC = 32, 16, 100
SIZES = [1, 3, 10, 3, 1, 10]       # groups of 1, 3 and 10 vectors, each size once unfiltered and once filtered below
TOP_KS = [1, 10]                   # over-fetch 20 and 200
STRATEGIES = [fc.STRATEGIES[2], fc.STRATEGIES[4]]   # ("rrf", 60) and ("weighted", 0.6, 0.3, 0.1)
assert STRATEGIES[0][0] == "rrf" and STRATEGIES[1][0] == "weighted"
ROWS = [va.WALK_ROWS_F32, va.WALK_ROWS_BF16, va.WALK_ROWS_INT8]
ROWS_NAME = {va.WALK_ROWS_F32: "f32", va.WALK_ROWS_BF16: "bf16", va.WALK_ROWS_INT8: "int8"}
WALKS = va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK
PLAIN = {va.WALK_ROWS_F32: va.KERNEL_HNSW, va.WALK_ROWS_BF16: va.KERNEL_HNSW_HALF, va.WALK_ROWS_INT8: va.KERNEL_HNSW_INT8}


def strategy_of(s):
    return va.FusionStrategy.RRF(s[1]) if s[0] == "rrf" else va.FusionStrategy.Weighted(*s[1:])


def assert_same(got, want, what):
    ids, sc, n = got
    assert np.array_equal(n, want[2]), (what, n, want[2])
    assert np.array_equal(ids, want[0]), (what, np.argwhere(ids != want[0])[:4])
    assert np.array_equal(sc.view(np.uint32), want[1]), (what, np.argwhere(sc.view(np.uint32) != want[1])[:4])


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


class World:
    def __init__(self, metric, rows):
        rng = np.random.default_rng(100 * int(metric) + rows)
        self.metric, self.n = metric, rows
        self.rows = rng.standard_normal((rows, DIM)).astype(np.float32)
        self.qs = rng.standard_normal((sum(SIZES), DIM)).astype(np.float32)
        self.ids = (np.arange(rows, dtype=np.uint64) * 7 + (1 << 33))
        self.ix = va.HnswIndex(DIM, metric, va.HnswParams(M, EFC, rows))
        assert self.ix.insert_batch_parallel(list(zip(self.ids.tolist(), self.rows))) == rows
        self.gone = self.ids[3::10].copy()
        for i in self.gone.tolist():
            assert self.ix.remove(i)
        self.live = set(self.ids.tolist()) - set(self.gone.tolist())
        self.ix.enable_half_precision(va.VectorPrecision.BF16)
        self.ix.train_quantizer()
        self.groups = np.split(self.qs, np.cumsum(SIZES)[:-1])
        pa = self.ids[np.random.default_rng(300).choice(rows, size=min(300, rows // 2), replace=False)]
        pb = self.ids[np.random.default_rng(20).choice(rows, size=20, replace=False)]
        self.fa, self.fb = self.ix.create_filter(pa), self.ix.create_filter(pb)
        self.fe = self.ix.create_filter(np.empty(0, dtype=np.uint64))
        self.allowed = {id(self.fa): set(pa.tolist()), id(self.fb): set(pb.tolist()), id(self.fe): set()}
        # per group: none, none, a wide filter, a narrow one, an empty one, the wide one again
        self.mixed = [None, None, self.fa, self.fb, self.fe, self.fa]
        self._lists = {}

    def group_lists(self, rows, g, kf, flt):
        """the lists the underlying call returns for the vectors of group g alone (cached: the reference, computed once)"""
        key = (rows, g, kf, id(flt) if flt is not None else None)
        if key not in self._lists:
            q, ix = self.groups[g], self.ix
            if flt is None:
                mode = {va.WALK_ROWS_F32: va.MODE_HNSW, va.WALK_ROWS_BF16: va.MODE_HNSW_BF16, va.WALK_ROWS_INT8: va.MODE_HNSW_INT8}[rows]
                ids, sc, cnt = ix._search_raw(q, kf, 0, mode)
            elif rows == va.WALK_ROWS_F32:
                ids, sc, cnt = ix.search_batch_with_filters(q, kf, [flt] * len(q))[0]
            elif rows == va.WALK_ROWS_INT8:
                ids, sc, cnt = ix.search_batch_with_filters_int8(q, kf, [flt] * len(q))[0]
            else:
                ids, sc, cnt = ix.search_batch_with_filters_half(q, kf, [flt] * len(q), va.MODE_HNSW_BF16)[0]
            self._lists[key] = [[(int(ids[v, j]), sc[v, j]) for j in range(int(cnt[v]))] for v in range(len(q))]
        return self._lists[key]

    def expect(self, rows, strategy, top_k, filters, order):
        kk, kf = max(top_k, 1), fr.overfetch(top_k)
        ids = np.empty((len(order), kk), dtype=np.uint64)
        sb = np.empty((len(order), kk), dtype=np.uint32)
        n = np.empty(len(order), dtype=np.uint32)
        for r, (g, flt) in enumerate(zip(order, filters)):
            ids[r], sb[r], n[r] = fr.fuse_top(strategy, self.group_lists(rows, g, kf, flt), top_k)
        return ids, sb, n

    def call(self, rows, strategy, top_k, filters, order):
        got = self.ix.multi_query_search_batch_filters([self.groups[g] for g in order], top_k, strategy_of(strategy), filters, rows)
        return got, self.ix.last_kernels()

    def close(self):
        for f in (self.fa, self.fb, self.fe):
            f.close()
        self.ix.close()


@pytest.fixture(scope="module")
def worlds():
    cache = {}

    def get(metric, rows):
        if (metric, rows) not in cache:
            cache[(metric, rows)] = World(metric, rows)
        return cache[(metric, rows)]
    yield get
    for w in cache.values():
        w.close()


WORLDS = [(DM.Cosine, 600), (DM.Euclidean, 600), (DM.Cosine, 150)]
world_id = lambda p: "%s-%d" % (p[0].name, p[1])  # noqa: E731
ALL = list(range(len(SIZES)))


@pytest.mark.parametrize("world", WORLDS, ids=world_id)
def test_f32_rows_with_no_or_one_shared_filter_is_the_one_filter_call(gpu_required, worlds, world):
    w = worlds(*world)
    for top_k in TOP_KS:
        for strategy in STRATEGIES:
            for flt in (None, w.fa, w.fb):
                old = w.ix.multi_query_search_batch(w.groups, top_k, strategy_of(strategy), flt)
                old_mask = w.ix.last_kernels()
                new = w.ix.multi_query_search_batch_filters(w.groups, top_k, strategy_of(strategy), [flt] * len(SIZES))
                assert same_bytes(old, new), (world, top_k, strategy, flt is not None)
                assert w.ix.last_kernels() == old_mask
    rrf = strategy_of(STRATEGIES[0])
    assert same_bytes(w.ix.multi_query_search_batch(w.groups, 10, rrf), w.ix.multi_query_search_batch_filters(w.groups, 10, rrf))
    ids, sc, n = w.ix.multi_query_search_batch_filters(w.groups, 0, rrf, w.mixed)
    assert ids.shape == (len(SIZES), 1) and (n == 0).all()
    assert w.ix.multi_query_search_batch_filters([], 5, rrf)[2].size == 0


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: ROWS_NAME[r])
@pytest.mark.parametrize("world", WORLDS, ids=world_id)
def test_mixed_table_is_the_rule_over_each_groups_own_lists(gpu_required, worlds, world, rows):
    w = worlds(*world)
    live_in = {id(f): len(w.allowed[id(f)] & w.live) for f in (w.fa, w.fb, w.fe)}
    for top_k in TOP_KS:
        for strategy in STRATEGIES:
            got, mask = w.call(rows, strategy, top_k, w.mixed, ALL)
            assert_same(got, w.expect(rows, strategy, top_k, w.mixed, ALL), (world, ROWS_NAME[rows], top_k, strategy))
            assert mask & va.KERNEL_FUSE and mask & WALKS and mask & PLAIN[rows], hex(mask)
            ids, sc, n = got
            for g, flt in enumerate(w.mixed):
                assert (ids[g, n[g]:] == PAD_ID).all() and (sc[g, n[g]:].view(np.uint32) == PAD_SCORE).all()
                out = set(ids[g, :n[g]].tolist())
                assert out <= w.live
                if flt is not None:
                    assert out <= w.allowed[id(flt)] and n[g] == min(top_k, live_in[id(flt)]), (g, n[g])
                alone, _ = w.call(rows, strategy, top_k, [flt], [g])
                assert same_bytes(alone, tuple(a[g:g + 1] for a in got)), (world, ROWS_NAME[rows], top_k, g)


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: ROWS_NAME[r])
def test_phases_in_any_order_and_alone(gpu_required, worlds, rows):
    w, top_k, strategy = worlds(DM.Cosine, 600), 10, STRATEGIES[0]
    tables = {
        "unfiltered behind filtered": ([w.fa, w.fb, w.fe, None, None], [2, 1, 4, 0, 5]),
        "interleaved": ([w.fb, None, w.fa, None], [5, 0, 1, 2]),
        "only unfiltered": ([None] * 3, [0, 1, 2]),
        "only filtered": ([w.fa, w.fb, w.fe], [0, 1, 2]),
        "only empty filters": ([w.fe, w.fe], [1, 2]),
    }
    for name, (filters, order) in tables.items():
        got, mask = w.call(rows, strategy, top_k, filters, order)
        assert_same(got, w.expect(rows, strategy, top_k, filters, order), (ROWS_NAME[rows], name))
        assert mask & va.KERNEL_FUSE
        any_fl = any(f is not None and f is not w.fe for f in filters)
        assert bool(mask & WALKS) == any_fl, (name, hex(mask))     # a phase without groups launches nothing
        if rows == va.WALK_ROWS_F32:
            assert bool(mask & va.KERNEL_HNSW) == any(f is None for f in filters), (name, hex(mask))


def test_documented_refusals(gpu_required, worlds):
    w = worlds(DM.Cosine, 600)
    out = [np.full((2, 5), 77, dtype=np.uint64), np.full((2, 5), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]

    def raw(ix, sizes=(2, 2), rows=0, ratio=0, table=(), fg=(0, 0), top_k=5, code=2, weights=None, null_entry=False):
        n_f = len(table)
        handles = (C.c_void_p * max(n_f, 1))(*[None if null_entry else f._h for f in table])
        gs, fga = np.array(sizes, dtype=np.uint32), np.array(fg, dtype=np.uint32)
        qs = np.ascontiguousarray(w.qs[:max(int(gs.sum()), 1)])
        rc = va.lib().vdb_hip_index_multi_query_search_filters(ix._h, rows, ratio, handles if n_f else None, n_f, fga.ctypes.data, qs.ctypes.data,
                                                               gs.ctypes.data, len(sizes), top_k, code, 60,
                                                               None if weights is None else weights.ctypes.data, out[0].ctypes.data,
                                                               out[1].ctypes.data, out[2].ctypes.data)
        assert all((o == 77).all() for o in out), "outputs touched on error"
        return rc, va._ffi.last_error()

    assert raw(w.ix, rows=-1)[0] == INVALID and raw(w.ix, rows=6)[0] == INVALID
    assert raw(w.ix, rows=va.WALK_ROWS_INT8, ratio=65)[0] == INVALID
    assert raw(w.ix, table=(w.fa,), null_entry=True)[0] == INVALID
    rc, msg = raw(w.ix, table=(w.fa,), fg=(0, 2))
    assert rc == INVALID and "entry 1" in msg
    rc, msg = raw(w.ix, sizes=(2, 0))
    assert rc == INVALID and "group 1" in msg
    rc, msg = raw(w.ix, sizes=(11, 1))
    assert rc == INVALID and "group 0" in msg
    assert raw(w.ix, code=4)[0] == INVALID
    assert raw(w.ix, code=3, weights=np.array([0.5, float("nan"), 0.5], np.float32))[0] == INVALID
    rc, msg = raw(w.ix, sizes=(2, 10), table=(w.fa,), fg=(1, 0), top_k=410)      # 10 lists of 820 records
    assert rc == UNSUPPORTED and "group 1" in msg
    for mode in (va.SHARD_RANGE, va.SHARD_REPLICA):
        grp = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64), devices=[0, 0], shard_mode=mode)
        try:
            assert raw(grp)[0] == UNSUPPORTED
        finally:
            grp.close()
    bits = va.HnswIndex(DIM, DM.Hamming, va.HnswParams(M, EFC, 64))
    try:
        bits.insert_batch_parallel(list(zip(range(40), (w.rows[:40] > 0).astype(np.float32))))
        for rows in range(1, 6):
            assert raw(bits, rows=rows)[0] == UNSUPPORTED
    finally:
        bits.close()
    plain = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 150))
    try:
        ids = np.arange(150, dtype=np.uint64)
        assert plain.insert_batch_parallel(list(zip(ids.tolist(), w.rows[:150]))) == 150
        for rows in range(1, 6):
            assert raw(plain, rows=rows)[0] == STATE, rows      # the image not enabled, the quantiser not trained
        with plain.create_filter(ids[:50]) as foreign:
            assert raw(w.ix, table=(foreign,), fg=(0, 1))[0] == INVALID
        with plain.create_filter(ids[:50]) as stale:
            assert plain.remove(0)
            plain.vacuum()
            assert raw(plain, table=(stale,), fg=(1, 0))[0] == STATE
    finally:
        plain.close()
    bare = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64))
    try:
        bare.upload(np.arange(40, dtype=np.uint64), w.rows[:40])
        assert raw(bare)[0] == STATE
    finally:
        bare.close()
