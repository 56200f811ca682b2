"""GPU tests of the hybrid search (csrc/hybrid.hip hybrid_fuse_kernel, vdb_hip_hybrid_fuse, vdb_hip_index_hybrid_search).

The reference is tests/hybrid_ref.py (held to the reference's own test cases and to the host model of csrc/vdb_hybrid.hpp by
tests/test_hybrid_cpu.py).  Everything is compared bit for bit — ids, fused score bits, counts and padding; there are no tolerances.
On an index the vector list the rule is applied to is the one the per-query call of the contract returns (search_batch in HNSW mode
at 2k, or search_batch_filtered_graph at max(4k, k + 10) with the filter), so the test pins the fusion and the plumbing, not the walk.
Nothing here provokes a fault: the limit cases are refusals the host decides before a launch.
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


def expect(cases, k, all_live=True):
    kk = max(k, 1)
    ids = np.empty((len(cases), kk), dtype=np.uint64)
    sb = np.empty((len(cases), kk), dtype=np.uint32)
    n = np.empty(len(cases), dtype=np.uint32)
    for g, c in enumerate(cases):
        ids[g], sb[g], n[g] = hr.top(hc.reference(c, k, all_live), k)
    return ids, sb, n


def assert_same(got, want, what):
    ids, sc, n = got
    assert np.array_equal(n, want[2]), (what, n, want[2])
    assert np.array_equal(ids, want[0]), (what, np.argwhere(ids != want[0])[:4])
    assert np.array_equal(sc.view(np.uint32), want[1]), (what, np.argwhere(sc.view(np.uint32) != want[1])[:4])


def fuse_call(cases, k):
    vi, vn, ti, tn, w = hc.pack(cases)
    return va.hybrid_fuse_arrays(vi, vn, ti, tn, k, w)


# ---- the kernel alone: vdb_hip_hybrid_fuse -----------------------------------------------------------------------------------

def test_adversarial_queries(gpu_required):
    adv = hc.adversarial_cases()
    names = sorted(adv)
    cases = [adv[n] for n in names]
    k = 40   # beyond every case's distinct ids
    assert_same(fuse_call(cases, k), expect(cases, k), names)
    # k around the number of distinct ids of every case: 0, 1, D - 1, D, D + 1, 4D
    for name in names:
        D = hc.distinct(adv[name])
        for kc in hc.cut_points(adv[name]):
            got = fuse_call([adv[name]], kc)
            assert_same(got, expect([adv[name]], kc), (name, kc))
            assert int(got[2][0]) == min(kc, D)
    # the default weight is 0.5
    vi, vn, ti, tn, _ = hc.pack([adv["weight_default"]])
    assert_same(va.hybrid_fuse_arrays(vi, vn, ti, tn, k), expect([adv["weight_0.5"]], k), "default")


@pytest.mark.parametrize("records", [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 8192])
def test_query_record_counts(gpu_required, records):
    rng = np.random.default_rng(records)
    small = hc.adversarial_cases()["lists_equal"]
    for w in (0.5, 0.3):
        c = hc.sized_case(records, rng, w)
        assert len(c["V"]) + len(c["T"]) == records
        want = expect([c], records)
        assert_same(fuse_call([c], records), want, w)
        # the same query behind a small one: the launch is sized by the larger, neither answer changes
        got = fuse_call([small, c], records)
        assert_same(tuple(a[1:] for a in got), want, w)
        assert_same(tuple(a[:1] for a in got), expect([small], records), w)
    # every record in one list
    for c in (hc.case(range(7, 7 + records), []), hc.case([], range(7, 7 + records), 0.25)):
        got = fuse_call([c], records)
        assert int(got[2][0]) == records
        assert_same(got, expect([c], records), "one list")


def test_query_past_the_lds_is_refused_untouched(gpu_required):
    rng = np.random.default_rng(8193)
    vi, vn, ti, tn, w = hc.pack([hc.adversarial_cases()["lists_equal"], hc.sized_case(8193, rng)])
    oi = np.full((2, 4), 77, dtype=np.uint64)
    os_ = np.full((2, 4), 77, dtype=np.float32)
    on = np.full(2, 77, dtype=np.uint32)
    rc = va.lib().vdb_hip_hybrid_fuse(0, vi.ctypes.data, vn.ctypes.data, vi.shape[1], ti.ctypes.data, tn.ctypes.data, ti.shape[1], w.ctypes.data, 2, 4,
                                      oi.ctypes.data, os_.ctypes.data, on.ctypes.data)
    assert rc == UNSUPPORTED and "query 1" in va._ffi.last_error()
    assert (oi == 77).all() and (os_ == 77).all() and (on == 77).all()


@pytest.mark.parametrize("nq", [1, 3, 130])
def test_queries_are_independent_of_their_companions(gpu_required, nq):
    rng = np.random.default_rng(nq)
    cases = [dict(hc.random_case(rng), dead=set(), allowed=None) for _ in range(nq)]
    if nq > 1:
        cases[1] = hc.case([], [])                         # a query of no ids
        cases[-1] = hc.sized_case(700, rng, 0.35)          # unequal sizes: the launch is sized by this one
    k = 12
    got = fuse_call(cases, k)
    assert_same(got, expect(cases, k), nq)
    for g in range(0, nq, max(1, nq // 16)):
        alone = fuse_call([cases[g]], k)
        for a, b in zip(alone, got):
            assert a[:1].tobytes() == b[g:g + 1].tobytes(), g


def test_invalid_calls(gpu_required):
    c = hc.adversarial_cases()["lists_equal"]
    vi, vn, ti, tn, w = hc.pack([c, c])
    out = [np.full((2, 3), 77, dtype=np.uint64), np.full((2, 3), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]

    def call(w=w, vi=vi, tn=tn, out_n=out[2]):
        rc = va.lib().vdb_hip_hybrid_fuse(0, None if vi is None else vi.ctypes.data, vn.ctypes.data, 4, ti.ctypes.data, tn.ctypes.data, 4,
                                          None if w is None else w.ctypes.data, 2, 3, out[0].ctypes.data, out[1].ctypes.data,
                                          None if out_n is None else out_n.ctypes.data)
        assert all((o == 77).all() for o in out)
        return rc

    assert call(vi=None) == INVALID and call(out_n=None) == INVALID
    assert call(tn=np.array([4, 5], np.uint32)) == INVALID
    assert call(w=np.array([0.5, float("nan")], np.float32)) == INVALID
    with pytest.raises(va.VelesHipError) as e:
        va.hybrid_fuse_arrays(vi, vn, ti, tn, 3, device=99)
    assert e.value.code == INVALID
    ids, sc, n = va.hybrid_fuse_arrays(vi, vn, ti, tn, 0)                  # k = 0: counts only
    assert ids.shape == (2, 1) and (n == 0).all() and (ids == PAD_ID).all()
    assert va.hybrid_fuse_arrays(np.zeros((0, 1), np.uint64), [], np.zeros((0, 1), np.uint64), [], 5)[2].size == 0


# ---- on an index: vdb_hip_index_hybrid_search --------------------------------------------------------------------------------

DIM, M, EFC, NQ = 32, 16, 100, 6
KS = [1, 10, 11, 75]               # 2k = 2, 20, 22, 150; with a filter max(4k, k + 10) = 11, 40, 44, 300
WEIGHTS = [0.5, 0.0, 1.0, 0.3, 0.8, 7.0]


class World:
    def __init__(self, metric, rows):
        rng = np.random.default_rng(100 * int(metric) + rows)
        self.metric, self.n = metric, rows
        self.rows = rng.standard_normal((rows, DIM)).astype(np.float32)
        self.qs = rng.standard_normal((NQ, DIM)).astype(np.float32)
        self.ids = (np.arange(rows, dtype=np.uint64) * 7 + (1 << 33))      # external ids beyond 32 bits
        self.ix = va.HnswIndex(DIM, metric, va.HnswParams(M, EFC, rows))
        assert self.ix.insert_batch_parallel(list(zip(self.ids.tolist(), self.rows))) == rows
        self.gone = self.ids[3::10].copy()                                   # removed rows
        for i in self.gone.tolist():
            assert self.ix.remove(i)
        self.live = set(self.ids.tolist()) - set(self.gone.tolist())
        self.rng = rng

    def lists(self, kf, flt=None):
        """the vector lists of the contract, one per query"""
        if flt is None:
            ids, _, cnt = self.ix._search_raw(self.qs, kf, 0, va.MODE_HNSW)
        else:
            (ids, _, cnt), _ = self.ix.search_batch_filtered_graph(self.qs, kf, flt)
        return [[int(ids[q, j]) for j in range(int(cnt[q]))] for q in range(NQ)]

    def text_hits(self, V, n):
        """n text ids mixed from the vector list, other live ids, removed rows and ids the handle never held"""
        rng = self.rng
        pool = [rng.choice(V, size=min(len(V), (n + 1) // 2), replace=False).tolist() if V else [],
                rng.choice(self.ids, size=n, replace=False).tolist(),
                rng.choice(self.gone, size=min(len(self.gone), max(1, n // 5)), replace=False).tolist(),
                [5, 6, (1 << 33) + 1, 0xFFFFFFFFFFFFFFFF][:max(1, n // 6)]]
        mix = [int(i) for p in pool for i in p]
        return [mix[j] for j in rng.permutation(len(mix))[:n]]

    def check(self, k, weights, allowed=None, flt=None):
        kf = 2 * k if flt is None else max(4 * k, k + 10)
        lists = self.lists(kf, flt)
        texts = [self.text_hits(V, kf) for V in lists]
        got = self.ix.hybrid_search_batch(self.qs, texts, k, weights, flt)
        mask = self.ix.last_kernels()
        w = [None] * NQ if weights is None else (list(weights) if np.ndim(weights) else [weights] * NQ)
        cases = [hc.case(V, T, wi, dead=set(T) - self.live, allowed=allowed) for V, T, wi in zip(lists, texts, w)]
        assert_same(got, expect(cases, k, all_live=False), (self.metric, self.n, k, weights, allowed is not None))
        assert mask & va.KERNEL_HYBRID_FUSE, mask
        ids, sc, n = got
        for g in range(NQ):
            assert (ids[g, n[g]:] == PAD_ID).all() and (sc[g, n[g]:].view(np.uint32) == PAD_SCORE).all()
            assert set(ids[g, :n[g]].tolist()) <= self.live
        return got, lists, texts, mask

    def close(self):
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


@pytest.mark.parametrize("rows", [600, 150])
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean], ids=lambda m: m.name)
def test_hybrid_search_is_the_rule_over_the_batch_lists(gpu_required, worlds, metric, rows):
    w = worlds(metric, rows)
    for k in KS:
        (ids, sc, n), lists, texts, mask = w.check(k, np.array(WEIGHTS, np.float32))
        assert mask & va.KERNEL_HNSW
        assert (n <= k).all()                                          # (a removed text id that leads the cut leaves it short)
        if rows == 150 and k == 75:
            assert all(len(V) <= len(w.live) < 2 * k for V in lists)    # lists shorter than 2k
    # the scalar form = the array form; the default = 0.5
    k = 10
    texts = [w.text_hits(V, 2 * k) for V in w.lists(2 * k)]
    a = w.ix.hybrid_search_batch(w.qs, texts, k, 0.3)
    b = w.ix.hybrid_search_batch(w.qs, texts, k, np.full(NQ, 0.3, np.float32))
    c = w.ix.hybrid_search_batch(w.qs, texts, k)
    d = w.ix.hybrid_search_batch(w.qs, texts, k, 0.5)
    for x, y in ((a, b), (c, d)):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    # one query alone = the query inside the call; the one-query front returns the same records
    for g in (0, 3, 5):
        ids, sc, n = w.ix.hybrid_search_batch(w.qs[g:g + 1], [texts[g]], k, 0.3)
        assert n[0] == a[2][g] and np.array_equal(ids[0], a[0][g]) and np.array_equal(sc[0].view(np.uint32), a[1][g].view(np.uint32))
        assert w.ix.hybrid_search(w.qs[g], texts[g], k, 0.3) == [(int(ids[0, j]), float(sc[0, j])) for j in range(int(n[0]))]
    # a text list of removed and unknown ids only, text-heavy: they fill the cut and leave, out_n < k
    dead = w.gone[:6].tolist() + [5, 6]
    ids, sc, n = w.ix.hybrid_search_batch(w.qs[:1], [dead], 6, 0.1)
    V = w.lists(12)[0]
    assert_same((ids, sc, n), expect([hc.case(V, dead, 0.1, dead=dead)], 6, all_live=False), "dead text")
    assert n[0] < 6
    # k = 0: out_n = 0; no queries: VDB_OK
    ids, sc, n = w.ix.hybrid_search_batch(w.qs, texts, 0)
    assert ids.shape == (NQ, 1) and (n == 0).all()
    assert w.ix.hybrid_search_batch(np.zeros((0, DIM), np.float32), [], 5)[2].size == 0


@pytest.mark.parametrize("allowed", [300, 20])
def test_with_a_filter_the_text_hits_are_compacted_before_ranks(gpu_required, worlds, allowed):
    w = worlds(DM.Cosine, 600)
    pick = w.ids[np.random.default_rng(allowed).choice(w.n, size=allowed, replace=False)]
    n_allowed_live = len(set(pick.tolist()) & w.live)
    with w.ix.create_filter(pick) as flt:
        assert flt.matched == n_allowed_live                               # (ids of removed rows are unknown to the handle)
        for k in KS:
            (ids, sc, n), lists, texts, mask = w.check(k, np.array(WEIGHTS, np.float32), allowed=set(pick.tolist()), flt=flt)
            assert mask & (va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK)
            for g in range(NQ):
                assert np.isin(ids[g, :n[g]], pick).all()
                assert n[g] == min(k, n_allowed_live)                  # never short while allowed candidates exist; 20 rows: out_n < 75
        one = w.ix.hybrid_search_with_filter(w.qs[2], texts[2], k, 0.3, flt)
        ids, sc, n = w.ix.hybrid_search_batch(w.qs[2:3], [texts[2]], k, 0.3, flt)
        assert one == [(int(ids[0, j]), float(sc[0, j])) for j in range(int(n[0]))]


def test_documented_refusals(gpu_required, worlds):
    w = worlds(DM.Cosine, 600)
    out = [np.full((2, 5), 77, dtype=np.uint64), np.full((2, 5), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]
    text = np.ascontiguousarray(np.stack([w.ids[:8], w.ids[8:16]]))

    def raw(ix, flt=None, k=5, text_n=(8, 8), weights=None, text=text):
        tn = np.array(text_n, dtype=np.uint32)
        qs = np.ascontiguousarray(w.qs[:2])
        rc = va.lib().vdb_hip_index_hybrid_search(ix._h, flt._h if flt is not None else None, qs.ctypes.data, 2, k, text.ctypes.data, tn.ctypes.data,
                                                  text.shape[1], None if weights is None else weights.ctypes.data, out[0].ctypes.data,
                                                  out[1].ctypes.data, out[2].ctypes.data)
        assert all((o == 77).all() for o in out), "outputs touched on error"
        return rc, va._ffi.last_error()

    rc, msg = raw(w.ix, weights=np.array([0.5, float("nan")], np.float32))
    assert rc == INVALID and "query 1" in msg
    rc, msg = raw(w.ix, text_n=(8, 9))
    assert rc == INVALID and "query 1" in msg
    wide = np.zeros((2, 8190), dtype=np.uint64)
    rc, msg = raw(w.ix, text=wide, text_n=(8, 8190))                 # 10 + 8190 records: past one block's LDS
    assert rc == UNSUPPORTED and "query 1" in msg
    rc, msg = raw(w.ix, k=4097)                                      # k' = 8194 alone is past it
    assert rc == UNSUPPORTED and "query 0" in msg
    # device groups
    for mode in (va.SHARD_RANGE, va.SHARD_REPLICA):
        grp = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64), devices=[0, 0], shard_mode=mode)
        try:
            assert raw(grp)[0] == UNSUPPORTED
        finally:
            grp.close()
    # a filter of another handle; a filter made stale by vacuum; no graph
    other = World(DM.Cosine, 150)
    try:
        with other.ix.create_filter(other.ids[:50]) as foreign:
            assert raw(w.ix, flt=foreign)[0] == INVALID
        with other.ix.create_filter(other.ids[:50]) as stale:
            other.ix.vacuum()
            assert raw(other.ix, flt=stale)[0] == STATE
    finally:
        other.close()
    bare = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64))
    try:
        bare.upload(np.arange(40, dtype=np.uint64), w.rows[:40])
        assert raw(bare)[0] == STATE
        with pytest.raises(va.VelesHipError) as e:
            bare.hybrid_search(w.qs[0], [1, 2], 5)
        assert e.value.code == STATE
    finally:
        bare.close()
