"""GPU tests of the hybrid search with one optional filter per query over every rows form of the walk
(vdb_hip_index_hybrid_search_filters, csrc/hybrid.hip hybrid_fuse_filters_kernel).

The reference is tests/hybrid_ref.py, as in tests/test_gpu_hybrid.py; everything is compared bit for bit — ids, fused score bits,
counts and padding; there are no tolerances.  The vector list the rule is applied to is the one the underlying call of the contract
returns for the query ALONE: the plain call of the rows form at 2k for an unfiltered query, the call with one filter per query of the
rows form at max(4k, k + 10) for a filtered one.  Nothing here provokes a fault: the limit cases are refusals the host decides before
a launch.
"""
import numpy as np
import pytest

import hybrid_cases as hc
import hybrid_ref as hr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
INVALID, UNSUPPORTED, STATE = -1, -7, -8
PAD_ID, PAD_SCORE = 0xFFFFFFFFFFFFFFFF, 0x7FC00000

DIM, M, EFC, NQ = 32, 16, 100, 6
KS = [1, 10, 11, 75]               # 2k = 2, 20, 22, 150; with a filter max(4k, k + 10) = 11, 40, 44, 300
WEIGHTS = np.array([0.5, 0.0, 1.0, 0.3, 0.8, 7.0], np.float32)
ROWS = [va.WALK_ROWS_F32, va.WALK_ROWS_F16, va.WALK_ROWS_BF16, va.WALK_ROWS_INT8, va.WALK_ROWS_F16_RESCORE, va.WALK_ROWS_BF16_RESCORE]
ROWS_NAME = {va.WALK_ROWS_F32: "f32", va.WALK_ROWS_F16: "f16", va.WALK_ROWS_BF16: "bf16", va.WALK_ROWS_INT8: "int8",
             va.WALK_ROWS_F16_RESCORE: "f16_rescore", va.WALK_ROWS_BF16_RESCORE: "bf16_rescore"}
HALF_MODE = {va.WALK_ROWS_F16: va.MODE_HNSW_F16, va.WALK_ROWS_BF16: va.MODE_HNSW_BF16, va.WALK_ROWS_F16_RESCORE: va.MODE_HNSW_F16,
             va.WALK_ROWS_BF16_RESCORE: va.MODE_HNSW_BF16}
H, F = va.KERNEL_HNSW_HALF, va.KERNEL_F16
WALKS = va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK


def list_len(k, filtered):
    return max(4 * k, k + 10) if filtered else 2 * k


def plain_bits(rows):
    """the bits the unfiltered phase of a rows form sets"""
    return {va.WALK_ROWS_F32: va.KERNEL_HNSW, va.WALK_ROWS_F16: H | F, va.WALK_ROWS_BF16: H, va.WALK_ROWS_INT8: va.KERNEL_HNSW_INT8,
            va.WALK_ROWS_F16_RESCORE: H | F | va.KERNEL_HALF_RESCORE, va.WALK_ROWS_BF16_RESCORE: H | va.KERNEL_HALF_RESCORE}[rows]


def filtered_bits(rows):
    """the bits every filtered phase of a rows form sets beside one of KERNEL_HNSW_FILTERED / KERNEL_FILTER_RANK"""
    return {va.WALK_ROWS_F32: 0, va.WALK_ROWS_F16: H | F, va.WALK_ROWS_BF16: H, va.WALK_ROWS_INT8: 0,
            va.WALK_ROWS_F16_RESCORE: 0, va.WALK_ROWS_BF16_RESCORE: 0}[rows]


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
        self.qs = rng.standard_normal((NQ, DIM)).astype(np.float32)
        self.ids = (np.arange(rows, dtype=np.uint64) * 7 + (1 << 33))      # external ids beyond 32 bits
        self.ix = va.HnswIndex(DIM, metric, va.HnswParams(M, EFC, rows))
        assert self.ix.insert_batch_parallel(list(zip(self.ids.tolist(), self.rows))) == rows
        self.gone = self.ids[3::10].copy()                                   # every tenth row removed
        for i in self.gone.tolist():
            assert self.ix.remove(i)
        self.live = set(self.ids.tolist()) - set(self.gone.tolist())
        self.ix.enable_half_precision(va.VectorPrecision.F16)
        self.ix.enable_half_precision(va.VectorPrecision.BF16)
        self.ix.train_quantizer()
        self.rng = rng
        # the mixed table: none, a wide filter, a narrow one, the wide one again, an empty one, none
        pa = self.ids[np.random.default_rng(300).choice(rows, size=min(300, rows // 2), replace=False)]
        pb = self.ids[np.random.default_rng(20).choice(rows, size=20, replace=False)]
        self.fa, self.fb = self.ix.create_filter(pa), self.ix.create_filter(pb)
        self.fe = self.ix.create_filter(np.empty(0, dtype=np.uint64))
        self.allowed = {id(self.fa): set(pa.tolist()), id(self.fb): set(pb.tolist()), id(self.fe): set()}
        self.mixed = [None, self.fa, self.fb, self.fa, self.fe, None]
        self._lists, self._texts = {}, {}

    def allowed_of(self, flt):
        return None if flt is None else self.allowed[id(flt)]

    def vector_list(self, rows, g, k, flt):
        """the list the underlying call of the contract returns for query g ALONE (cached: it is the reference, computed once)"""
        key = (rows, g, k, id(flt) if flt is not None else None)
        if key not in self._lists:
            q, kf, ix = self.qs[g:g + 1], list_len(k, flt is not None), self.ix
            if rows >= va.WALK_ROWS_F16_RESCORE:
                ids, _, cnt = ix.search_batch_with_filters_half_rescore(q, kf, [flt], HALF_MODE[rows])[0]
            elif flt is None:
                mode = {va.WALK_ROWS_F32: va.MODE_HNSW, va.WALK_ROWS_INT8: va.MODE_HNSW_INT8}.get(rows) or HALF_MODE[rows]
                ids, _, cnt = ix._search_raw(q, kf, 0, mode)
            elif rows == va.WALK_ROWS_F32:
                ids, _, cnt = ix.search_batch_with_filters(q, kf, [flt])[0]
            elif rows == va.WALK_ROWS_INT8:
                ids, _, cnt = ix.search_batch_with_filters_int8(q, kf, [flt])[0]
            else:
                ids, _, cnt = ix.search_batch_with_filters_half(q, kf, [flt], HALF_MODE[rows])[0]
            self._lists[key] = [int(ids[0, j]) for j in range(int(cnt[0]))]
        return self._lists[key]

    def text_hits(self, g, k, filtered):
        """the query's text hits, the same for every rows form: mixed from near rows, other live ids, removed rows and ids the handle
        never held"""
        key = (g, k, filtered)
        if key not in self._texts:
            n, rng = list_len(k, filtered), self.rng
            near = self.vector_list(va.WALK_ROWS_F32, g, k, None)
            pool = [rng.choice(near, size=min(len(near), (n + 1) // 2), replace=False).tolist() if near else [],
                    rng.choice(self.ids, size=min(n, self.n), replace=False).tolist(),
                    rng.choice(self.gone, size=min(len(self.gone), max(1, n // 5)), replace=False).tolist(),
                    [5, 6, (1 << 33) + 1, 0xFFFFFFFFFFFFFFFF][:max(1, n // 6)]]
            mix = [int(i) for p in pool for i in p]
            self._texts[key] = [mix[j] for j in rng.permutation(len(mix))[:n]]
        return self._texts[key]

    def expect(self, rows, k, filters, weights, order=None):
        """the reference rule over the underlying lists, query by query"""
        order = list(range(NQ)) if order is None else order
        kk = max(k, 1)
        ids = np.empty((len(order), kk), dtype=np.uint64)
        sb = np.empty((len(order), kk), dtype=np.uint32)
        n = np.empty(len(order), dtype=np.uint32)
        for r, (g, flt) in enumerate(zip(order, filters)):
            T = self.text_hits(g, k, flt is not None)
            c = hc.case(self.vector_list(rows, g, k, flt), T, float(weights[r]), dead=set(T) - self.live, allowed=self.allowed_of(flt))
            ids[r], sb[r], n[r] = hr.top(hc.reference(c, k, all_live=False), k)
        return ids, sb, n

    def call(self, rows, k, filters, weights, order=None, oversampling=0):
        order = list(range(NQ)) if order is None else order
        texts = [self.text_hits(g, k, flt is not None) for g, flt in zip(order, filters)]
        got = self.ix.hybrid_search_batch_filters(self.qs[order], texts, k, weights, filters, rows, oversampling)
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


WORLDS = [(DM.Cosine, 600), (DM.Euclidean, 600), (DM.Cosine, 150), (DM.Euclidean, 150)]
world_id = lambda p: "%s-%d" % (p[0].name, p[1])  # noqa: E731


# ---- 1. rows F32 without a filter, or with one shared filter, is the one-filter call byte for byte -----------------------------

@pytest.mark.parametrize("world", WORLDS, ids=world_id)
def test_f32_rows_with_no_or_one_shared_filter_is_the_one_filter_call(gpu_required, worlds, world):
    w = worlds(*world)
    for k in KS:
        for flt in (None, w.fa, w.fb):
            texts = [w.text_hits(g, k, flt is not None) for g in range(NQ)]
            old = w.ix.hybrid_search_batch(w.qs, texts, k, WEIGHTS, flt)
            old_mask = w.ix.last_kernels()
            new = w.ix.hybrid_search_batch_filters(w.qs, texts, k, WEIGHTS, [flt] * NQ)
            assert same_bytes(old, new), (world, k, flt is not None)
            assert w.ix.last_kernels() == old_mask
    # filters=None is "no query filtered"; the scalar and the default weight; k = 0; no queries
    texts = [w.text_hits(g, 10, False) for g in range(NQ)]
    assert same_bytes(w.ix.hybrid_search_batch(w.qs, texts, 10), w.ix.hybrid_search_batch_filters(w.qs, texts, 10))
    assert same_bytes(w.ix.hybrid_search_batch(w.qs, texts, 10, 0.3), w.ix.hybrid_search_batch_filters(w.qs, texts, 10, 0.3, [None] * NQ))
    ids, sc, n = w.ix.hybrid_search_batch_filters(w.qs, texts, 0, None, w.mixed)
    assert ids.shape == (NQ, 1) and (n == 0).all() and (ids == PAD_ID).all()
    assert w.ix.hybrid_search_batch_filters(np.zeros((0, DIM), np.float32), [], 5)[2].size == 0


# ---- 2. every rows form with the mixed table -----------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ROWS, ids=lambda r: ROWS_NAME[r])
@pytest.mark.parametrize("world", WORLDS, ids=world_id)
def test_mixed_table_is_the_rule_over_each_querys_own_list(gpu_required, worlds, world, rows):
    w = worlds(*world)
    live_in = {id(f): len(w.allowed[id(f)] & w.live) for f in (w.fa, w.fb, w.fe)}
    for k in KS:
        got, mask = w.call(rows, k, w.mixed, WEIGHTS)
        assert_same(got, w.expect(rows, k, w.mixed, WEIGHTS), (world, ROWS_NAME[rows], k))
        ids, sc, n = got
        # the walk bits of both phases of the rows form and the fuse bit
        assert mask & va.KERNEL_HYBRID_FUSE and mask & WALKS, hex(mask)
        assert mask & filtered_bits(rows) == filtered_bits(rows), (ROWS_NAME[rows], hex(mask))
        # (the re-score forms walk their unfiltered queries through the filters call too, which may answer a small index by its f32
        # exact pass alone: KERNEL_FILTER_RANK and none of the half bits)
        if rows < va.WALK_ROWS_F16_RESCORE or mask & va.KERNEL_HNSW_FILTERED:
            assert mask & plain_bits(rows) == plain_bits(rows), (ROWS_NAME[rows], hex(mask))
        for g, flt in enumerate(w.mixed):
            assert (ids[g, n[g]:] == PAD_ID).all() and (sc[g, n[g]:].view(np.uint32) == PAD_SCORE).all()
            out = set(ids[g, :n[g]].tolist())
            assert out <= w.live
            if flt is not None:
                assert out <= w.allowed[id(flt)] and n[g] == min(k, live_in[id(flt)]), (g, n[g])   # the empty filter: out_n = 0
            # the query sent alone through the new entry point
            alone = w.ix.hybrid_search_batch_filters(w.qs[g:g + 1], [w.text_hits(g, k, flt is not None)], k, WEIGHTS[g:g + 1], [flt], rows)
            assert same_bytes(alone, tuple(a[g:g + 1] for a in got)), (world, ROWS_NAME[rows], k, g)
    assert w.ix.last_search_stats()[0] > 0      # (distances were evaluated; a small index may be answered by exact passes, which expand nothing)


def test_search_stats_are_the_sum_over_both_phases(gpu_required, worlds):
    w, k = worlds(DM.Cosine, 600), 10
    for rows in (va.WALK_ROWS_F32, va.WALK_ROWS_BF16, va.WALK_ROWS_INT8):
        stats = []
        for filters, order in (([None, None], [0, 5]), ([w.fa, w.fb], [1, 2]), ([None, w.fa, w.fb, None], [0, 1, 2, 5])):
            w.call(rows, k, filters, WEIGHTS[order], order)
            stats.append(w.ix.last_search_stats())
        assert all(s[0] > 0 and s[1] > 0 for s in stats)
        assert stats[2] == (stats[0][0] + stats[1][0], stats[0][1] + stats[1][1]), (ROWS_NAME[rows], stats)


# ---- 3. rows is honoured -------------------------------------------------------------------------------------------------------

def test_bf16_rows_change_a_vector_list(gpu_required, worlds):
    differs = 0
    for world in WORLDS[:2]:
        w = worlds(*world)
        for k in (10, 11):
            for g in range(NQ):
                for flt in (None, w.fa):
                    differs += w.vector_list(va.WALK_ROWS_F32, g, k, flt) != w.vector_list(va.WALK_ROWS_BF16, g, k, flt)
    assert differs >= 1                         # (bf16 rounding reorders near neighbours on these Gaussian worlds)
    # ... and where the lists differ, the fused answers of the two rows forms are each its own list's
    w = worlds(DM.Cosine, 600)
    a, _ = w.call(va.WALK_ROWS_F32, 10, w.mixed, WEIGHTS)
    b, _ = w.call(va.WALK_ROWS_BF16, 10, w.mixed, WEIGHTS)
    assert_same(a, w.expect(va.WALK_ROWS_F32, 10, w.mixed, WEIGHTS), "f32")
    assert_same(b, w.expect(va.WALK_ROWS_BF16, 10, w.mixed, WEIGHTS), "bf16")


def test_oversampling_is_read_for_the_forms_that_have_one(gpu_required, worlds):
    w, k = worlds(DM.Cosine, 600), 10
    for rows in (va.WALK_ROWS_F32, va.WALK_ROWS_F16, va.WALK_ROWS_BF16):   # not read: any value, the same bytes
        assert same_bytes(w.call(rows, k, w.mixed, WEIGHTS)[0], w.call(rows, k, w.mixed, WEIGHTS, oversampling=1000)[0])
    # the re-score forms: 0 = 4; the int8 form: 0 = the handle's option
    for rows in (va.WALK_ROWS_F16_RESCORE, va.WALK_ROWS_BF16_RESCORE):
        assert same_bytes(w.call(rows, k, w.mixed, WEIGHTS)[0], w.call(rows, k, w.mixed, WEIGHTS, oversampling=4)[0])
    ratio = w.ix.get_option(va.OPT_INT8_OVERSAMPLING)
    assert same_bytes(w.call(va.WALK_ROWS_INT8, k, w.mixed, WEIGHTS)[0], w.call(va.WALK_ROWS_INT8, k, w.mixed, WEIGHTS, oversampling=ratio)[0])
    # a ratio of 1 is the underlying calls' lists at ratio 1
    for rows in (va.WALK_ROWS_INT8, va.WALK_ROWS_BF16_RESCORE):
        got, _ = w.call(rows, k, [None, w.fa], WEIGHTS[:2], [0, 1], oversampling=1)
        for r, (g, flt) in enumerate(((0, None), (1, w.fa))):
            q, kf = w.qs[g:g + 1], list_len(k, flt is not None)
            if rows == va.WALK_ROWS_INT8 and flt is None:   # the plain int8 call with a ratio of its own: search_with_config
                cfg = va.DualPrecisionConfig(oversampling_ratio=1, use_int8_traversal=True, min_index_size=0)
                V = [i for i, _ in w.ix.search_with_config(q[0], kf, 0, cfg)]
            elif rows == va.WALK_ROWS_INT8:
                ids, _, cnt = w.ix.search_batch_with_filters_int8(q, kf, [flt], oversampling=1)[0]
                V = [int(i) for i in ids[0, :cnt[0]]]
            else:
                ids, _, cnt = w.ix.search_batch_with_filters_half_rescore(q, kf, [flt], va.MODE_HNSW_BF16, oversampling=1)[0]
                V = [int(i) for i in ids[0, :cnt[0]]]
            T = w.text_hits(g, k, flt is not None)
            c = hc.case(V, T, float(WEIGHTS[r]), dead=set(T) - w.live, allowed=w.allowed_of(flt))
            wi, ws, wn = hr.top(hc.reference(c, k, all_live=False), k)
            assert_same(tuple(a[r:r + 1] for a in got), (wi.reshape(1, -1), ws.reshape(1, -1), np.array([wn], np.uint32)), (ROWS_NAME[rows], g))


# ---- 4. phases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [va.WALK_ROWS_F32, va.WALK_ROWS_F16, va.WALK_ROWS_INT8, va.WALK_ROWS_BF16_RESCORE], ids=lambda r: ROWS_NAME[r])
def test_phases_in_any_order_and_alone(gpu_required, worlds, rows):
    w, k = worlds(DM.Cosine, 600), 11
    tables = {
        "unfiltered behind filtered": ([w.fa, w.fb, w.fe, None, None, None], [1, 2, 4, 0, 5, 3]),
        "interleaved": ([w.fb, None, w.fa, None, w.fe, None], [2, 0, 1, 5, 4, 3]),
        "only unfiltered": ([None] * NQ, list(range(NQ))),
        "only filtered": ([w.fa, w.fb, w.fa, w.fb, w.fe, w.fa], list(range(NQ))),
        "only empty filters": ([w.fe] * 3, [0, 1, 2]),
        "one unfiltered": ([None], [3]),
        "one filtered": ([w.fb], [3]),
    }
    for name, (filters, order) in tables.items():
        got, mask = w.call(rows, k, filters, WEIGHTS[order], order)
        assert_same(got, w.expect(rows, k, filters, WEIGHTS[order], order), (ROWS_NAME[rows], name))
        assert mask & va.KERNEL_HYBRID_FUSE
        any_un, any_fl = any(f is None for f in filters), any(f is not None and f is not w.fe for f in filters)
        # a phase without queries launches nothing: its walk's bits stay out of the mask (f32: the plain walk's bit is its own)
        if rows < va.WALK_ROWS_F16_RESCORE:     # (the re-score forms walk their unfiltered queries with the filters kernels too)
            assert bool(mask & WALKS) == any_fl, (name, hex(mask))
        if rows == va.WALK_ROWS_F32:
            assert bool(mask & va.KERNEL_HNSW) == any_un, (name, hex(mask))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

def test_documented_refusals(gpu_required, worlds):
    w = worlds(DM.Cosine, 600)
    out = [np.full((2, 5), 77, dtype=np.uint64), np.full((2, 5), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]
    text = np.ascontiguousarray(np.stack([w.ids[:8], w.ids[8:16]]))
    import ctypes as C

    def raw(ix, rows=0, ratio=0, table=(), fq=(0, 0), k=5, text_n=(8, 8), weights=None, text=text, null_entry=False):
        n_f = len(table)
        handles = (C.c_void_p * max(n_f, 1))(*[None if null_entry else f._h for f in table])
        fqa, tn = np.array(fq, dtype=np.uint32), np.array(text_n, dtype=np.uint32)
        qs = np.ascontiguousarray(w.qs[:2])
        rc = va.lib().vdb_hip_index_hybrid_search_filters(ix._h, rows, ratio, handles if n_f else None, n_f, fqa.ctypes.data, qs.ctypes.data, 2, k,
                                                          text.ctypes.data, tn.ctypes.data, text.shape[1],
                                                          None if weights is None else weights.ctypes.data, out[0].ctypes.data,
                                                          out[1].ctypes.data, out[2].ctypes.data)
        assert all((o == 77).all() for o in out), "outputs touched on error"
        return rc, va._ffi.last_error()

    # INVALID_ARG
    assert raw(w.ix, rows=-1)[0] == INVALID and raw(w.ix, rows=6)[0] == INVALID
    assert raw(w.ix, table=(w.fa,), null_entry=True)[0] == INVALID
    rc, msg = raw(w.ix, table=(w.fa,), fq=(0, 2))                                   # a table value above n_filters
    assert rc == INVALID and "entry 1" in msg
    rc, msg = raw(w.ix, weights=np.array([0.5, float("nan")], np.float32))
    assert rc == INVALID and "query 1" in msg
    rc, msg = raw(w.ix, text_n=(8, 9))
    assert rc == INVALID and "query 1" in msg
    for rows in (va.WALK_ROWS_INT8, va.WALK_ROWS_F16_RESCORE, va.WALK_ROWS_BF16_RESCORE):
        assert raw(w.ix, rows=rows, ratio=65)[0] == INVALID
    # UNSUPPORTED: a query past the LDS with ITS OWN list length — 2k + text_n legal, max(4k, k + 10) + text_n not
    wide = np.zeros((2, 8183), dtype=np.uint64)
    rc, msg = raw(w.ix, table=(w.fa,), fq=(1, 0), text=wide, text_n=(8173, 8173))   # k = 5: 10 + 8173 <= 8192 < 20 + 8173
    assert rc == UNSUPPORTED and "query 1" in msg
    rc, msg = raw(w.ix, table=(w.fa,), fq=(1, 1), text=wide, text_n=(8, 8183))      # unfiltered: 10 + 8183
    assert rc == UNSUPPORTED and "query 1" in msg
    rc, msg = raw(w.ix, k=4097)                                                     # k' = 8194 alone is past it
    assert rc == UNSUPPORTED and "query 0" in msg
    # ... device groups, Hamming with other rows than f32
    for mode in (va.SHARD_RANGE, va.SHARD_REPLICA):
        grp = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64), devices=[0, 0], shard_mode=mode)
        try:
            assert raw(grp)[0] == UNSUPPORTED
        finally:
            grp.close()
    bits = va.HnswIndex(DIM, DM.Hamming, va.HnswParams(M, EFC, 64))
    try:
        bits.insert_batch_parallel(list(zip(range(40), (w.rows[:40] > 0).astype(np.float32))))
        for rows in ROWS[1:]:
            assert raw(bits, rows=rows)[0] == UNSUPPORTED
    finally:
        bits.close()
    # STATE: the image not enabled, the quantiser not trained, a stale filter, no graph; INVALID: a filter of another handle
    plain = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 150))
    try:
        ids = np.arange(150, dtype=np.uint64)
        assert plain.insert_batch_parallel(list(zip(ids.tolist(), w.rows[:150]))) == 150
        for rows in ROWS[1:]:
            assert raw(plain, rows=rows)[0] == STATE, ROWS_NAME[rows]
        with plain.create_filter(ids[:50]) as foreign:
            assert raw(w.ix, table=(foreign,), fq=(0, 1))[0] == INVALID
            assert raw(w.ix, table=(w.fa, foreign), fq=(0, 2))[0] == INVALID       # (named by no query: the table is checked whole)
        with plain.create_filter(ids[:50]) as stale:
            assert plain.remove(0)
            plain.vacuum()
            assert raw(plain, table=(stale,), fq=(1, 0))[0] == STATE
    finally:
        plain.close()
    bare = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64))
    try:
        bare.upload(np.arange(40, dtype=np.uint64), w.rows[:40])
        assert raw(bare)[0] == STATE
    finally:
        bare.close()
    # the same arrays in a legal call are written
    tn, fqa, qs = np.array([8, 8], np.uint32), np.array([0, 0], np.uint32), np.ascontiguousarray(w.qs[:2])
    rc = va.lib().vdb_hip_index_hybrid_search_filters(w.ix._h, 0, 0, None, 0, fqa.ctypes.data, qs.ctypes.data, 2, 5, text.ctypes.data, tn.ctypes.data, 8,
                                                      None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    assert rc == 0 and (out[2] == 5).all() and not (out[0] == 77).any()
