"""GPU tests of the multi-query search with result fusion (csrc/fusion.hip fuse_lists_kernel, vdb_hip_fuse_results,
vdb_hip_index_multi_query_search).

The reference is tests/fusion_ref.py (held to the reference's own test cases and to the host model of csrc/vdb_fusion.hpp by
tests/test_fusion_cpu.py).  Everything is compared bit for bit — ids, fused score bits, counts and padding; there are no tolerances.
On an index the lists the rule is applied to are the ones the per-query calls of the contract return (search_batch in HNSW mode at
the over-fetched k, or search_batch_filtered_graph with the filter), so the test pins the fusion and the plumbing, not the walk.
Nothing here provokes a fault: the limit cases are refusals the host decides before a launch.
"""
import numpy as np
import pytest

import fusion_cases as fc
import fusion_ref as fr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
INVALID, UNSUPPORTED, STATE = -1, -7, -8
PAD_ID, PAD_SCORE = 0xFFFFFFFFFFFFFFFF, 0x7FC00000


def strategy_of(s):
    kind = s[0]
    if kind == "average":
        return va.FusionStrategy.Average()
    if kind == "maximum":
        return va.FusionStrategy.Maximum()
    if kind == "rrf":
        return va.FusionStrategy.RRF(s[1])
    return va.FusionStrategy.Weighted(*s[1:])


def expect(strategy, groups, top_k):
    kk = max(top_k, 1)
    ids = np.empty((len(groups), kk), dtype=np.uint64)
    sb = np.empty((len(groups), kk), dtype=np.uint32)
    n = np.empty(len(groups), dtype=np.uint32)
    for g, group in enumerate(groups):
        ids[g], sb[g], n[g] = fr.fuse_top(strategy, group, top_k)
    return ids, sb, n


def assert_same(got, want, what):
    ids, sc, n = got
    assert np.array_equal(n, want[2]), (what, n, want[2])
    assert np.array_equal(ids, want[0]), (what, np.argwhere(ids != want[0])[:4])
    assert np.array_equal(sc.view(np.uint32), want[1]), (what, np.argwhere(sc.view(np.uint32) != want[1])[:4])


def fuse_call(strategy, groups, top_k):
    ids, sc, ln, gs = fc.pack(groups)
    return va.fuse_arrays(strategy_of(strategy), ids, sc, ln, gs, top_k)


# ---- the kernel alone: vdb_hip_fuse_results ----------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", fc.STRATEGIES, ids=str)
def test_adversarial_groups(gpu_required, strategy):
    adv = fc.adversarial_groups()
    names = sorted(adv)
    groups = [adv[k] for k in names]
    top_k = 330   # beyond every group's distinct ids (the largest: 300)
    assert_same(fuse_call(strategy, groups, top_k), expect(strategy, groups, top_k), names)
    # top_k around the number of distinct ids of one group: 0, 1, D - 1, D, D + 1, far beyond
    g = adv["ids_differ_in_one_half"]
    D = len(fr.fuse(strategy, g))
    for k in (0, 1, D - 1, D, D + 1, 4 * D):
        got = fuse_call(strategy, [g], k)
        assert_same(got, expect(strategy, [g], k), k)
        assert int(got[2][0]) == min(k, D)
    assert va.FusionStrategy.fuse(strategy_of(strategy), g) == [(i, float(s)) for i, s in fr.fuse(strategy, g)]


@pytest.mark.parametrize("records", [1, 63, 64, 65, 1023, 1024, 1025, 8192])
def test_group_record_counts(gpu_required, records):
    rng = np.random.default_rng(records)
    group = fc.sized_group(records, rng)
    assert sum(len(l) for l in group) == records
    for strategy in (("rrf", 60), ("weighted", 0.6, 0.3, 0.1)):
        want = expect(strategy, [group], records)
        assert_same(fuse_call(strategy, [group], records), want, strategy)
        # the same group behind a small one: the launch is sized by the larger, the small group's answer does not change
        small = fc.adversarial_groups()["one_list"]
        got = fuse_call(strategy, [small, group], records)
        assert_same(tuple(a[1:] for a in got), want, strategy)
        assert_same(tuple(a[:1] for a in got), expect(strategy, [small], records), strategy)
    # every id distinct: as many fused records as inputs
    uniq = [[(int(i), float(s)) for i, s in l] for l in fc.sized_group(records, rng, universe=1 << 40)]
    if len({i for l in uniq for i, _ in l}) == records:
        got = fuse_call(("average",), [uniq], records)
        assert int(got[2][0]) == records
        assert_same(got, expect(("average",), [uniq], records), "distinct")


def test_group_past_the_lds_is_refused_untouched(gpu_required):
    rng = np.random.default_rng(8193)
    ids, sc, ln, gs = fc.pack([fc.adversarial_groups()["one_list"], fc.sized_group(8193, rng)])
    oi = np.full((2, 4), 77, dtype=np.uint64)
    os_ = np.full((2, 4), 77, dtype=np.float32)
    on = np.full(2, 77, dtype=np.uint32)
    w = np.zeros(3, np.float32)
    rc = va.lib().vdb_hip_fuse_results(0, 2, 60, w.ctypes.data, ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, ids.shape[0], ids.shape[1],
                                       gs.ctypes.data, 2, 4, oi.ctypes.data, os_.ctypes.data, on.ctypes.data)
    assert rc == UNSUPPORTED and "group 1" in va._ffi.last_error()
    assert (oi == 77).all() and (os_ == 77).all() and (on == 77).all()


@pytest.mark.parametrize("n_groups", [1, 3, 130])
def test_groups_are_independent_of_their_companions(gpu_required, n_groups):
    rng = np.random.default_rng(n_groups)
    groups = [fc.random_group(rng) for _ in range(n_groups)]
    if n_groups > 1:
        groups[1] = []                                     # a group of no lists
        groups[-1] = fc.sized_group(700, rng)              # unequal sizes: the launch is sized by this one
    strategy, top_k = fc.STRATEGIES[n_groups % len(fc.STRATEGIES)], 12
    got = fuse_call(strategy, groups, top_k)
    assert_same(got, expect(strategy, groups, top_k), n_groups)
    for g in range(0, n_groups, max(1, n_groups // 16)):
        alone = fuse_call(strategy, [groups[g]], top_k)
        for a, b in zip(alone, got):
            assert a[:1].tobytes() == b[g:g + 1].tobytes(), g


def test_invalid_calls(gpu_required):
    g = fc.adversarial_groups()["one_list"]
    ids, sc, ln, gs = fc.pack([g, g])
    w = np.array([0.6, 0.3, 0.1], np.float32)
    out = [np.full((2, 3), 77, dtype=np.uint64), np.full((2, 3), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]

    def call(code=2, w=w, ids=ids, gs=gs, n_groups=2, out_n=out[2]):
        rc = va.lib().vdb_hip_fuse_results(0, code, 60, None if w is None else w.ctypes.data, None if ids is None else ids.ctypes.data,
                                           sc.ctypes.data, ln.ctypes.data, 2, ids.shape[1] if ids is not None else 3, gs.ctypes.data, n_groups, 3,
                                           out[0].ctypes.data, out[1].ctypes.data, None if out_n is None else out_n.ctypes.data)
        assert all((o == 77).all() for o in out)
        return rc

    assert call(gs=np.array([1, 2], np.uint32)) == INVALID
    assert call(ids=None) == INVALID and call(out_n=None) == INVALID
    assert call(code=4) == INVALID
    assert call(code=3, w=None) == INVALID
    for bad in ((0.5, 0.3, 0.1), (-0.1, 0.6, 0.5), (float("nan"), 0.5, 0.5)):
        assert call(code=3, w=np.array(bad, np.float32)) == INVALID, bad
    with pytest.raises(va.VelesHipError) as e:
        va.fuse_arrays(va.FusionStrategy.rrf_default(), ids, sc, ln, gs, 3, device=99)
    assert e.value.code == INVALID


# ---- on an index: vdb_hip_index_multi_query_search ---------------------------------------------------------------------------

DIM, M, EFC = 32, 8, 100
SIZES = [1, 3, 10, 2, 5]           # five groups of mixed sizes in one call: V = 1, 3 and 10 among them
TOP_KS = [10, 11, 51, 101]         # over-fetch 200, 110, 255, 202


class World:
    def __init__(self, metric, rows):
        rng = np.random.default_rng(100 * int(metric) + rows)
        self.metric, self.n = metric, rows
        self.rows = rng.standard_normal((rows, DIM)).astype(np.float32)
        self.qs = rng.standard_normal((sum(SIZES), DIM)).astype(np.float32)
        if metric == DM.Hamming:
            self.rows, self.qs = (self.rows > 0).astype(np.float32), (self.qs > 0).astype(np.float32)
        self.ids = (np.arange(rows, dtype=np.uint64) * 7 + (1 << 33))      # external ids beyond 32 bits
        self.ix = va.HnswIndex(DIM, metric, va.HnswParams(M, EFC, rows))
        assert self.ix.insert_batch_parallel(list(zip(self.ids.tolist(), self.rows))) == rows
        self.groups = np.split(self.qs, np.cumsum(SIZES)[:-1])

    def lists(self, kf, flt=None):
        """the lists of the contract, one per vector of the call"""
        if flt is None:
            ids, sc, cnt = self.ix._search_raw(self.qs, kf, 0, va.MODE_HNSW)
        else:
            (ids, sc, cnt), _ = self.ix.search_batch_filtered_graph(self.qs, kf, flt)
        per_vec = [[(int(ids[q, j]), sc[q, j]) for j in range(int(cnt[q]))] for q in range(self.qs.shape[0])]
        cuts = np.cumsum([0] + SIZES)
        return [per_vec[cuts[g]:cuts[g + 1]] for g in range(len(SIZES))], cnt

    def check(self, strategy, top_k, flt=None):
        lists, cnt = self.lists(fr.overfetch(top_k), flt)
        got = self.ix.multi_query_search_batch(self.groups, top_k, strategy_of(strategy), flt)
        mask = self.ix.last_kernels()
        assert_same(got, expect(strategy, lists, top_k), (self.metric, self.n, strategy, top_k))
        assert mask & va.KERNEL_FUSE, mask
        return got, cnt, mask

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
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct, DM.Hamming], ids=lambda m: m.name)
def test_multi_query_search_is_the_rule_over_the_batch_lists(gpu_required, worlds, metric, rows):
    w = worlds(metric, rows)
    for t, top_k in enumerate(TOP_KS):
        for strategy in (("rrf", 60), fc.STRATEGIES[(t + int(metric)) % 2], fc.STRATEGIES[4]):
            got, cnt, mask = w.check(strategy, top_k)
            assert mask & va.KERNEL_HNSW
            if rows == 150:
                assert int(cnt.max()) <= rows < fr.overfetch(top_k) or top_k == 11     # lists shorter than the over-fetch
            assert (got[2] > 0).all() and (got[2] <= top_k).all()
    # one group alone = the group inside the call; the one-query front returns the same records
    strategy, top_k = ("rrf", 60), 10
    all_ids, all_sc, all_n = w.ix.multi_query_search_batch(w.groups, top_k, strategy_of(strategy))
    for g in (0, 2, 4):
        ids, sc, n = w.ix.multi_query_search_batch([w.groups[g]], top_k, strategy_of(strategy))
        assert n[0] == all_n[g] and np.array_equal(ids[0], all_ids[g]) and np.array_equal(sc[0].view(np.uint32), all_sc[g].view(np.uint32))
        one = w.ix.multi_query_search_ids(w.groups[g], top_k, strategy_of(strategy))
        assert one == [(int(ids[0, j]), float(sc[0, j])) for j in range(int(n[0]))]
    # top_k = 0: nothing to fuse, out_n = 0
    ids, sc, n = w.ix.multi_query_search_batch(w.groups, 0, strategy_of(strategy))
    assert ids.shape == (len(SIZES), 1) and (n == 0).all()
    ids, sc, n = w.ix.multi_query_search_batch([], 5, strategy_of(strategy))
    assert n.size == 0


def test_removed_rows_never_come_back(gpu_required):
    w = World(DM.Cosine, 600)
    try:
        gone = w.ids[::10]
        for i in gone.tolist():
            assert w.ix.remove(i)
        for strategy, top_k in ((("rrf", 60), 10), (("average",), 51), (("weighted", 0.6, 0.3, 0.1), 101)):
            (ids, sc, n), _, _ = w.check(strategy, top_k)
            for g in range(len(SIZES)):
                assert not np.isin(ids[g, :n[g]], gone).any()
                assert (ids[g, n[g]:] == PAD_ID).all() and (sc[g, n[g]:].view(np.uint32) == PAD_SCORE).all()
    finally:
        w.close()


@pytest.mark.parametrize("allowed", [300, 20])
def test_with_a_filter_the_lists_are_the_filtered_walks(gpu_required, worlds, allowed):
    w = worlds(DM.Cosine, 600)
    pick = np.random.default_rng(allowed).choice(w.n, size=allowed, replace=False)
    with w.ix.create_filter(w.ids[pick]) as flt:
        assert flt.matched == allowed
        for strategy, top_k in ((("rrf", 60), 10), (("maximum",), 11), (("weighted", 0.7, 0.3, 0.0), 51)):
            (ids, sc, n), cnt, mask = w.check(strategy, top_k, flt)
            assert mask & (va.KERNEL_HNSW_FILTERED | va.KERNEL_FILTER_RANK)
            assert int(cnt.max()) <= allowed
            for g in range(len(SIZES)):
                assert np.isin(ids[g, :n[g]], w.ids[pick]).all() and n[g] == min(top_k, allowed)


def test_documented_refusals(gpu_required, worlds):
    w = worlds(DM.Cosine, 600)
    rrf = va.FusionStrategy.rrf_default()
    out = [np.full((2, 5), 77, dtype=np.uint64), np.full((2, 5), 77, dtype=np.float32), np.full(2, 77, dtype=np.uint32)]

    def raw(ix, sizes, flt=None, top_k=5, code=2, weights=None):
        gs = np.array(sizes, dtype=np.uint32)
        qs = np.ascontiguousarray(w.qs[:max(int(gs.sum()), 1)])
        rc = va.lib().vdb_hip_index_multi_query_search(ix._h, flt._h if flt is not None else None, qs.ctypes.data, gs.ctypes.data, len(sizes), top_k,
                                                       code, 60, None if weights is None else weights.ctypes.data, out[0].ctypes.data,
                                                       out[1].ctypes.data, out[2].ctypes.data)
        assert all((o == 77).all() for o in out), "outputs touched on error"
        return rc, va._ffi.last_error()

    rc, msg = raw(w.ix, [2, 0])
    assert rc == INVALID and "at least one vector" in msg and "group 1" in msg
    rc, msg = raw(w.ix, [11, 1])
    assert rc == INVALID and "at most 10 vectors, got 11" in msg and "group 0" in msg
    assert raw(w.ix, [2, 2], code=4)[0] == INVALID
    assert raw(w.ix, [2, 2], code=3, weights=np.array([0.5, 0.3, 0.1], np.float32))[0] == INVALID
    rc, msg = raw(w.ix, [2, 10], top_k=410)                      # 10 lists of 820 records: past one block's LDS
    assert rc == UNSUPPORTED and "group 1" in msg
    # device groups
    for mode in (va.SHARD_RANGE, va.SHARD_REPLICA):
        grp = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64), devices=[0, 0], shard_mode=mode)
        try:
            assert raw(grp, [2, 2])[0] == UNSUPPORTED
        finally:
            grp.close()
    # a filter of another handle; a filter made stale by vacuum; no graph
    other = World(DM.Cosine, 150)
    try:
        with other.ix.create_filter(other.ids[:50]) as foreign:
            assert raw(w.ix, [2, 2], flt=foreign)[0] == INVALID
        with other.ix.create_filter(other.ids[:50]) as stale:
            assert other.ix.remove(int(other.ids[0]))
            other.ix.vacuum()
            assert raw(other.ix, [2, 2], flt=stale)[0] == STATE
    finally:
        other.close()
    bare = va.HnswIndex(DIM, DM.Cosine, va.HnswParams(M, EFC, 64))
    try:
        bare.upload(np.arange(40, dtype=np.uint64), w.rows[:40])
        assert raw(bare, [2, 2])[0] == STATE
        with pytest.raises(va.VelesHipError) as e:
            bare.multi_query_search_ids(w.qs[:2], 5, rrf)
        assert e.value.code == STATE
    finally:
        bare.close()
