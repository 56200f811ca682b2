"""GPU parity of the multi-device handle (`devices=[...]`, csrc/shard_group.hip) for every search mode, k tier and shard shape it
serves — DESIGN 5: "ids, ranks, score bits, tie order are those of one index over all rows".

References (never the group handle's own output):
  * R-oracle: the oracle's scan over all live rows in global insertion order (`po.scan_topk`, `po.scan_topk_sq8`,
    `po.scan_topk_binary`, arithmetic mode from `sweep_arith_mode(k)`) — exact f32 on the five metrics, SQ8, Binary.  Where it
    applies the single-device handle over all rows must return the very same k-wide arrays, counts and filler included.
  * R-merge (tests/shard_merge_ref.py `merge_lists`, CPU-tested against the oracle's merge): the stable merge of the results of
    independent single-device indexes over exactly the rows each shard holds — the bf16 / f16 result modes (their bits may depend on
    the tier a shard's size selects) and everything with one graph per shard (HNSW, AUTO past 100 rows, rerank).
All groups are built as tests/test_gpu_sharded.py builds them (`shard_devices`): distinct devices when the box has them, else
co-located on device 0.  One process, one GPU is enough."""
import numpy as np
import pytest

from oracle import pyoracle as po

import shard_merge_ref as smr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
SQ = va.SearchQuality
VP = va.index.VectorPrecision
SM = va.StorageMode
PO_METRIC = {DM.Cosine: po.COSINE, DM.Euclidean: po.EUCLIDEAN, DM.DotProduct: po.DOT, DM.Hamming: po.HAMMING,
             DM.Jaccard: po.JACCARD}
UNSUPPORTED = -7
# enum vdb_kernel_bit: the selection stage on the matrix cores; every matrix-core family of the exact f32 sweep
SELECTION = va.index.KERNEL_SELECT_BF16 | va.index.KERNEL_SELECT_SPLIT
MATRIX_F32 = SELECTION | va.index.KERNEL_GEMM_F32 | va.index.KERNEL_SWEEP_MFMA_F32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shard_devices(n):
    """n shards over the visible GPUs: distinct devices when there are enough (RCCL), else co-located on device 0"""
    nd = va.device_count()
    return list(range(n)) if nd >= n else [0] * n


def group(dim, metric, max_elements, shards, mode=None, M=8, efc=50):
    return va.HnswIndex(dim, metric, va.HnswParams(M, efc, max_elements), devices=shard_devices(shards),
                        shard_mode=va.SHARD_RANGE if mode is None else mode)


def single(dim, metric, max_elements, M=8, efc=50):
    return va.HnswIndex(dim, metric, va.HnswParams(M, efc, max_elements))


def oracle_mode(ix, k):
    return po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C


def r_oracle(kind, metric, rows, ext_ids, qs, k, mode=po.MODE_C, live=None):
    """R-oracle as a k-wide single-device style block (ids, scores, counts): the scan over the live rows in insertion order"""
    qs = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, rows.shape[1])
    lv = np.arange(len(rows)) if live is None else np.flatnonzero(live)
    kk = min(k, len(lv))
    nq = len(qs)
    if kk == 0:
        return smr.pad_lists(np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32), k)
    sub = np.ascontiguousarray(rows[lv])
    if kind == "f32":
        eid, esc = po.scan_topk(PO_METRIC[metric], sub, qs, kk, mode, nthreads=po.host_threads())
    elif kind == "sq8":
        eid, esc = po.scan_topk_sq8(PO_METRIC[metric], sub, qs, kk, nthreads=po.host_threads())
    else:
        eid, esc = po.scan_topk_binary(sub, qs, kk)
    return smr.pad_lists(np.asarray(ext_ids, dtype=np.uint64)[lv[eid.astype(np.int64)]], esc, np.full(nq, kk, np.uint32), k)


def assert_same(got, exp, what):
    """whole k-wide arrays: counts, ids (ranks, tie order), score bits, the filler past the count"""
    gi, gs, gc = np.asarray(got[0], dtype=np.uint64), bits(got[1]), np.asarray(got[2], dtype=np.uint32)
    ei, es, ec = np.asarray(exp[0], dtype=np.uint64), bits(exp[1]), np.asarray(exp[2], dtype=np.uint32)
    assert gi.shape == ei.shape, (what, gi.shape, ei.shape)
    assert np.array_equal(gc, ec), (what, "counts", gc[:8], ec[:8])
    bad = np.flatnonzero(np.any(gi != ei, axis=1) | np.any(gs != es, axis=1))
    if len(bad):
        q = int(bad[0])
        p = int(np.flatnonzero((gi[q] != ei[q]) | (gs[q] != es[q]))[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(gi)} queries differ; first: query {q} rank {p}: got id {gi[q, p]} bits "
                             f"{gs[q, p]:#010x}, expected id {ei[q, p]} bits {es[q, p]:#010x}")


def tuples_block(res, k):
    """[(id, score), ...] of one query (or a list of them) -> a k-wide block"""
    if res and isinstance(res[0], tuple) or res == []:
        res = [res]
    return smr.pad_lists(*smr.lists_of_tuples(res, k), k)


# ---------------------------------------------------------------------------------------------------------------
# 1. k tiers through the merge
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
def test_k_tiers_through_the_merge(gpu_required, metric):
    rng = np.random.default_rng(100 + int(metric))
    n, dim, shards, nq = 3000, 96, 3, 70
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33)
    sh, one = group(dim, metric, n, shards), single(dim, metric, n)
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    for k in (1, 11, 48, 49, 100, 128):
        exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
        assert_same(sh.search_batch_brute_force(qs, k), exp, (metric, k, "group"))
        assert_same(one.search_batch_brute_force(qs, k), exp, (metric, k, "single device"))
    sh.close()
    one.close()


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
def test_short_shard_lists_full_merged_list_and_k_past_all_rows(gpu_required, metric):
    # 40 + 40 + 40 rows: at k = 100 every shard's list is short and the merged list is full; at k = 130 the counts are 120 and the
    # tail is the single-device filler
    rng = np.random.default_rng(200 + int(metric))
    n, dim, shards, nq = 120, 96, 3, 70
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(7)
    sh, one = group(dim, metric, n, shards), single(dim, metric, n)
    assert smr.shard_ranges(n, shards, n) == [(0, 40), (40, 80), (80, 120)]
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    for k, cnt in ((100, 100), (130, 120)):
        exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
        assert np.all(exp[2] == cnt)
        got = sh.search_batch_brute_force(qs, k)
        assert_same(got, exp, (metric, k, "group"))
        assert np.all(got[0][:, cnt:] == smr.FILL_ID) and np.all(bits(got[1])[:, cnt:] == smr.FILL_BITS)
        assert_same(one.search_batch_brute_force(qs, k), exp, (metric, k, "single device"))
    sh.close()
    one.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. ties and special scores straddling shards
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
def test_ties_and_special_scores_straddle_shards(gpu_required, metric):
    rng = np.random.default_rng(300 + int(metric))
    n, dim, shards, k = 3000, 64, 3, 25
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    v, w = rng.standard_normal(dim).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    # the same row in every shard (several times), a second family of duplicates: exact ties that must come out in global row order
    for r in (5, 6, 900, 1005, 1500, 1999, 2005, 2999):
        rows[r] = v
    for lo in (100, 1100, 2100):
        rows[lo:lo + 6] = w                      # 18 ties: all three shards inside the top 25, whatever else ranks first
    qs = rng.standard_normal((20, dim)).astype(np.float32)
    qs[0], qs[1], qs[2], qs[3] = v, w, v * np.float32(0.5), v + w
    if metric == DM.DotProduct:
        # products that are exactly zero, of either sign, in different shards: query = +-e0, every row's coordinate 0 negative
        # except the planted rows (+0.0 in shard 0, -0.0 in shard 2, an all-zero row in shard 1).  (Every sum starts from +0.0 in
        # the declared arithmetic, so the scores themselves come out +0.0: a 20-way tie over the three shards right behind the NaN
        # and the inf row.  The place of -0.0 against +0.0 in the merge rule is held on the CPU tier, tests/test_sharded_cpu.py.)
        rows[:, 0] = -np.abs(rows[:, 0]) - np.float32(0.1)
        rows[40:48] = np.abs(rows[40:48])
        rows[40:48, 0] = 0.0
        rows[2040:2048] = -np.abs(rows[2040:2048])
        rows[2040:2048, 0] = -0.0
        rows[1040:1044] = 0.0
        for qi, (s0, rest) in zip((4, 5, 6, 7), ((1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (-1.0, -0.0))):
            qs[qi] = rest
            qs[qi, 0] = s0
    # a NaN row and an inf row in different shards (as tests/test_gpu_sweep.py plants them on one device)
    rows[17, 3] = np.nan
    rows[1029, 0] = np.inf
    ids = np.arange(n, dtype=np.uint64)
    sh, one = group(dim, metric, n, shards), single(dim, metric, n)
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
    # the planted ties really are in the lists the comparison covers, from more than one shard
    assert {5, 6, 900, 1005, 1500, 1999, 2005, 2999} <= set(exp[0][0].tolist())
    assert len({int(i) // 1000 for i in exp[0][1].tolist()}) == 3
    if metric == DM.DotProduct:
        top = set(exp[0][4].tolist())
        assert top & set(range(40, 48)) and top & set(range(2040, 2048)) and top & set(range(1040, 1044))
    assert_same(sh.search_batch_brute_force(qs, k), exp, (metric, "group"))
    assert_same(one.search_batch_brute_force(qs, k), exp, (metric, "single device"))
    sh.close()
    one.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. shards that take different routes: shard 0 holds 66 048 rows (>= 65 536: the selection stage at 256 queries), shard 1 holds 300
ROUTE_C, ROUTE_TAIL, ROUTE_NQ = 66_048, 300, 256
_route_cache = {}


def route_corpus(dim, binary=False):
    key = (dim, binary)
    if key not in _route_cache:
        rng = np.random.default_rng(4000 + dim + int(binary))
        n = ROUTE_C + ROUTE_TAIL
        if binary:
            rows = (rng.random((n, dim)) > 0.6915).astype(np.float32)
            qs = (rng.random((ROUTE_NQ, dim)) > 0.6915).astype(np.float32)
        else:
            rows = rng.standard_normal((n, dim)).astype(np.float32)
            qs = rng.standard_normal((ROUTE_NQ, dim)).astype(np.float32)
        _route_cache[key] = (rows, qs, np.arange(n, dtype=np.uint64) + np.uint64(1 << 20))
    return _route_cache[key]


def route_handles(dim, metric, rows, ids, with_single=True, parts=False):
    out = [group(dim, metric, 2 * ROUTE_C, 2)]
    if with_single:
        out.append(single(dim, metric, len(rows)))
    for ix in out:
        assert ix.upload(ids, rows) == len(rows)
    if parts:
        for lo, hi in smr.shard_ranges(2 * ROUTE_C, 2, len(rows)):
            p = single(dim, metric, hi - lo)
            assert p.upload(ids[lo:hi], rows[lo:hi]) == hi - lo
            out.append(p)
    return out


# dim 128: the smallest dim at which Cosine, Euclidean and 10 < k <= 128 (the WIDE selection) all take the selection stage
# (select_stage.hip: dim % 64 == 0, dim >= 128).  dim 64: Cosine at k <= 10 takes it (split-bf16, dim % 32 == 0, dim >= 64); the
# dispatch has no selection kernel for Euclidean or for k > 10 there, so those cases hold the mix of a 66 048-row and a 300-row
# shard to the oracle and assert the route only where one exists.
@pytest.mark.parametrize("metric,dim,k,selection", [
    (DM.Cosine, 128, 10, True), (DM.Cosine, 128, 50, True), (DM.Euclidean, 128, 10, True), (DM.Euclidean, 128, 50, True),
    (DM.Cosine, 64, 10, True), (DM.Cosine, 64, 50, False), (DM.Euclidean, 64, 10, False), (DM.Euclidean, 64, 50, False)])
def test_shards_on_different_routes_exact_f32(gpu_required, metric, dim, k, selection):
    rows, qs, ids = route_corpus(dim)
    sh, one = route_handles(dim, metric, rows, ids)
    assert smr.shard_ranges(2 * ROUTE_C, 2, len(rows)) == [(0, ROUTE_C), (ROUTE_C, ROUTE_C + ROUTE_TAIL)]
    exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
    got = sh.search_batch_brute_force(qs, k)
    mask = sh.last_kernels()                      # the OR of what the shards ran
    assert_same(got, exp, (metric, dim, k, "group"))
    if selection:
        assert mask & SELECTION, f"no matrix-core selection kernel ran on the 66 048-row shard: kernels {mask:#x}"
    # results from both shards are in play (or the case says nothing about the merge)
    from_tail = np.isin(got[0], ids[ROUTE_C:]).sum()
    assert 0 < from_tail < got[0].size, from_tail
    assert_same(one.search_batch_brute_force(qs, k), exp, (metric, dim, k, "single device"))
    sh.close()
    one.close()


def test_shards_on_different_routes_hamming_four_bit_gemm(gpu_required):
    dim, k = 64, 10
    rows, qs, ids = route_corpus(dim, binary=True)
    sh, one = route_handles(dim, DM.Hamming, rows, ids)
    exp = r_oracle("f32", DM.Hamming, rows, ids, qs, k, po.MODE_C)
    got = sh.search_batch_brute_force(qs, k)
    mask = sh.last_kernels()
    assert_same(got, exp, "group")
    assert mask & va.index.KERNEL_BITS_GEMM, f"the four-bit GEMM did not run on the 66 048-row shard: kernels {mask:#x}"
    assert_same(one.search_batch_brute_force(qs, k), exp, "single device")
    sh.close()
    one.close()


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_shards_on_different_routes_sq8_and_binary(gpu_required, metric):
    dim, k = 128, 10
    rows, qs, ids = route_corpus(dim)
    sh, one = route_handles(dim, metric, rows, ids)
    for ix in (sh, one):
        ix.set_storage_mode(SM.SQ8)
    exp = r_oracle("sq8", metric, rows, ids, qs, k)
    assert_same(sh.search_batch_sq8(qs, k), exp, (metric, "sq8 group"))
    assert_same(one.search_batch_sq8(qs, k), exp, (metric, "sq8 single device"))
    last = int(ids[-1])                           # lives in the last shard
    assert sh.get_quantized_bytes(last) == po.QuantizedVector.from_f32(rows[-1]).to_bytes()
    if metric == DM.Euclidean:                    # the sign-bit codes do not depend on the metric: once
        for ix in (sh, one):
            ix.set_storage_mode(SM.Binary)
        exp = r_oracle("binary", metric, rows, ids, qs, k)
        assert_same(sh.search_batch_binary(qs, k), exp, "binary group")
        assert_same(one.search_batch_binary(qs, k), exp, "binary single device")
        assert sh.get_quantized_bytes(last) == po.BinaryQuantizedVector.from_f32(rows[-1]).to_bytes()
    sh.close()
    one.close()


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_shards_on_different_routes_half_result_modes(gpu_required, metric):
    # bf16 result mode (mode 3) and mode 7 (f16): the bits of a shard's list may depend on the tier its row count selects, so the
    # reference is R-merge over single-device indexes holding exactly the shards' rows
    dim, k = 128, 10
    rows, qs, ids = route_corpus(dim)
    sh, p0, p1 = route_handles(dim, metric, rows, ids, with_single=False, parts=True)
    hib = po.higher_is_better(PO_METRIC[metric])
    for prec in (VP.F16, VP.BF16):
        for ix in (sh, p0, p1):
            ix.enable_half_precision(prec)
        exp = smr.merge_lists([p.search_batch_brute_force_half(qs, k, prec) for p in (p0, p1)], k, hib)
        got = sh.search_batch_brute_force_half(qs, k, prec)
        assert_same(got, exp, (metric, prec))
        assert 0 < np.isin(got[0], ids[ROUTE_C:]).sum() < got[0].size
    if metric == DM.Cosine:                       # the bf16 result mode by its own entry points
        for ix in (sh, p0, p1):
            ix.enable_bf16()
        exp = smr.merge_lists([p.search_batch_brute_force_bf16(qs, k) for p in (p0, p1)], k, hib)
        assert_same(sh.search_batch_brute_force_bf16(qs, k), exp, (metric, "bf16 result mode"))
    for ix in (sh, p0, p1):
        ix.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. empty and dead shards
def dev_search(ix, qs, k, ef=0, mode=None):
    """vdb_hip_index_search_batch_dev with torch buffers; the outputs are poisoned first, so that what the call leaves unwritten shows"""
    torch = pytest.importorskip("torch")
    nq = len(qs)
    dq = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).cuda()
    d_ids = torch.full((nq, k), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    d_sc = torch.full((nq, k), -12345.0, dtype=torch.float32, device="cuda")
    d_n = torch.full((nq,), 0x7EADBEEF, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_batch_dev(dq.data_ptr(), nq, k, ef, va.MODE_BRUTE if mode is None else mode, d_ids.data_ptr(), d_sc.data_ptr(),
                        d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy().view(np.uint64), d_sc.cpu().numpy(), d_n.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_empty_and_dead_shards(gpu_required, metric):
    rng = np.random.default_rng(500 + int(metric))
    n, dim, shards, k = 1100, 32, 4, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((5, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(11)
    sh, one = group(dim, metric, 4000, shards), single(dim, metric, 4000)
    assert smr.shard_ranges(4000, shards, n) == [(0, 1000), (1000, 1100), (1100, 1100), (1100, 1100)]   # shards 2, 3: no row
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    live = np.ones(n, bool)

    def check(what):
        exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k), live)
        assert_same(sh.search_batch_brute_force(qs, k), exp, (metric, what, "group, host entry"))
        assert_same(dev_search(sh, qs, k), exp, (metric, what, "group, device entry"))
        assert_same(one.search_batch_brute_force(qs, k), exp, (metric, what, "single device"))
        return exp

    check("two empty shards")
    for r in range(1000):                         # every row of shard 0: it has rows, none of them live
        assert sh.remove(int(ids[r])) and one.remove(int(ids[r]))
    live[:1000] = False
    exp = check("shard 0 dead")
    assert np.all(exp[0] >= ids[1000])
    for r in range(1000, 1093):                   # 7 rows live anywhere: fewer than k
        assert sh.remove(int(ids[r])) and one.remove(int(ids[r]))
    live[1000:1093] = False
    exp = check("fewer than k live")
    assert np.all(exp[2] == 7) and sh.len() == 7
    sh.close()
    one.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. scratch reuse between calls of one handle
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_scratch_reuse_across_batch_shapes(gpu_required, metric):
    rng = np.random.default_rng(600 + int(metric))
    n, dim, shards = 900, 16, 3
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    allq = rng.standard_normal((1030, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    sh, one = group(dim, metric, n, shards), single(dim, metric, n)
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    # growing, shrinking, one query, and past the 1 024-query chunk of the single-device path
    for nq, k in ((70, 10), (3, 128), (300, 50), (1, 1), (1030, 10)):
        qs = allq[:nq] if nq != 3 else allq[500:503]
        exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
        assert_same(sh.search_batch_brute_force(qs, k), exp, (metric, nq, k, "group"))
        assert_same(one.search_batch_brute_force(qs, k), exp, (metric, nq, k, "single device"))
    sh.close()
    one.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. graph modes on range shards
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean, DM.DotProduct])
def test_per_shard_graphs_walk_and_rerank(gpu_required, metric):
    # the shape of test_gpu_sharded.py::test_range_handle_inserts_and_per_shard_graphs, on the metrics whose best score is the
    # largest as well: one graph per shard, merged == R-merge of independent single-device indexes over the same row ranges
    rng = np.random.default_rng(700 + int(metric))
    n, dim, k, ef = 1200, 64, 10, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((20, dim)).astype(np.float32)
    hib = po.higher_is_better(PO_METRIC[metric])
    sh = group(dim, metric, n, 2, efc=60)
    ranges = smr.shard_ranges(n, 2, n)
    parts = [single(dim, metric, hi - lo, efc=60) for lo, hi in ranges]
    for i in range(n):
        sh.insert(i, rows[i])
        parts[i // (n // 2)].insert(i, rows[i])
    assert [p.len() for p in parts] == [hi - lo for lo, hi in ranges] and sh.len() == n
    exp = smr.merge_lists([p._search_raw(qs, k, ef, va.MODE_HNSW) for p in parts], k, hib)
    got = sh._search_raw(qs, k, ef, va.MODE_HNSW)
    assert sh.last_kernels() & va.index.KERNEL_HNSW
    assert_same(got, exp, (metric, "graph walk"))
    assert len({int(i) // (n // 2) for i in got[0].ravel().tolist()}) == 2          # both shards contribute
    best = got[1][:, 0]                                                              # the lists are best first in the metric's order
    assert np.all(best >= got[1][:, k - 1]) if hib else np.all(best <= got[1][:, k - 1])
    if metric != DM.DotProduct:
        # rerank: raw scores in the metric's order, whatever order the walk's own scores have
        for qi in range(6):
            cand = [p.search_with_rerank(qs[qi], k, 40) for p in parts]
            exp1 = smr.merge_lists([tuples_block(c, k) for c in cand], k, hib)
            assert_same(tuples_block(sh.search_with_rerank(qs[qi], k, 40), k), exp1, (metric, "rerank", qi))
    # the exact scan over the same handle still equals the oracle
    assert_same(sh.search_batch_brute_force(qs, k), r_oracle("f32", metric, rows, np.arange(n), qs, k, oracle_mode(sh, k)), (metric, "exact"))
    sh.close()
    for p in parts:
        p.close()


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_auto_is_resolved_on_the_whole_index(gpu_required, metric):
    # search_with_quality's size switch (<= 100 live vectors: the exact scan) looks at the whole index: two shards of ~50 rows hold
    # 100 live rows -> the scan; one more insert -> one graph walk per shard, merged
    rng = np.random.default_rng(800 + int(metric))
    dim, k = 32, 10
    rows = rng.standard_normal((101, dim)).astype(np.float32)
    qs = rng.standard_normal((8, dim)).astype(np.float32)
    ef = SQ.Balanced.ef_search(k)
    hib = po.higher_is_better(PO_METRIC[metric])
    sh = group(dim, metric, 102, 2, efc=60)
    ranges = smr.shard_ranges(102, 2, 101)
    assert ranges == [(0, 51), (51, 101)]
    parts = [single(dim, metric, 51, efc=60) for _ in ranges]
    for i in range(100):
        sh.insert(i, rows[i])
        parts[0 if i < 51 else 1].insert(i, rows[i])
    assert sh.len() == 100 and [p.len() for p in parts] == [51, 49]
    exp = r_oracle("f32", metric, rows[:100], np.arange(100), qs, k, oracle_mode(sh, k))
    assert_same(sh._search_raw(qs, k, ef, va.MODE_AUTO), exp, (metric, "100 live rows: the exact scan"))
    assert not sh.last_kernels() & va.index.KERNEL_HNSW
    for qi in range(3):
        assert_same(tuples_block(sh.search_with_quality(qs[qi], k, SQ.Balanced), k), [a[qi:qi + 1] for a in exp], (metric, "search_with_quality", qi))
    sh.insert(100, rows[100])
    parts[1].insert(100, rows[100])
    # (the per-shard handles hold 51 / 50 rows: left to AUTO they would scan)
    exp = smr.merge_lists([p._search_raw(qs, k, ef, va.MODE_HNSW) for p in parts], k, hib)
    assert_same(sh._search_raw(qs, k, ef, va.MODE_AUTO), exp, (metric, "101 live rows: per-shard walks"))
    assert sh.last_kernels() & va.index.KERNEL_HNSW
    for qi in range(3):
        assert_same(tuples_block(sh.search_with_quality(qs[qi], k, SQ.Balanced), k), [a[qi:qi + 1] for a in exp], (metric, "search_with_quality", qi))
    sh.close()
    for p in parts:
        p.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the device-pointer entry
@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
@pytest.mark.parametrize("dim", [30, 17])
def test_device_pointer_entry_range_padded_rows(gpu_required, metric, dim):
    # dim % 4 != 0: the rows (and the query copy) are padded to row_stride > dim — the memset + 2-D copy branch of group_search_dev
    rng = np.random.default_rng(900 + dim + int(metric))
    n, k, nq = 2000, 50, 66
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(5)
    sh, one = group(dim, metric, n, 2), single(dim, metric, n)
    for ix in (sh, one):
        assert ix.upload(ids, rows) == n
    exp = r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(one, k))
    assert_same(dev_search(sh, qs, k), exp, (metric, dim, "group, device entry"))
    assert_same(dev_search(sh, qs[:3], k), r_oracle("f32", metric, rows, ids, qs[:3], k, oracle_mode(one, k)), (metric, dim, "smaller batch after a larger one"))
    assert_same(sh.search_batch_brute_force(qs, k), exp, (metric, dim, "group, host entry"))
    assert_same(one.search_batch_brute_force(qs, k), exp, (metric, dim, "single device"))
    sh.close()
    one.close()


def test_replica_group_device_and_host_entries_and_quantizer(gpu_required):
    rng = np.random.default_rng(21)
    n, dim, k, ef = 800, 30, 10, 64
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((37, dim)).astype(np.float32)
    rep, one = group(dim, DM.Cosine, n, 2, mode=va.SHARD_REPLICA, efc=60), single(dim, DM.Cosine, n, efc=60)
    items = [(i, rows[i]) for i in range(n)]
    assert rep.insert_batch_parallel(items, 256) == n and one.insert_batch_parallel(items, 256) == n
    info = rep.shard_info()
    assert info["n_shards"] == 2 and info["shard_mode"] == va.SHARD_REPLICA and info["transport"] == "none"
    # nq = 1 on two replicas: the second replica's slice is empty
    for nq in (37, 1):
        q = qs[:nq]
        for mode, e in ((va.MODE_BRUTE, 0), (va.MODE_HNSW, ef)):
            ref = one._search_raw(q, k, e, mode)
            assert np.all(ref[2] == k)
            assert_same(dev_search(rep, q, k, e, mode), ref, ("device entry", nq, mode))
            assert_same(rep._search_raw(q, k, e, mode), ref, ("host entry", nq, mode))
    assert rep.search_batch_parallel(qs[:1], k, SQ.Custom(ef)) == one.search_batch_parallel(qs[:1], k, SQ.Custom(ef))
    assert rep.search(qs[0], k) == one.search(qs[0], k)
    # 8. the int8 quantiser on replicas: trained on every replica, the flag on the handle the caller holds
    assert not rep.is_quantizer_trained()
    rep.train_quantizer()
    one.train_quantizer()
    assert rep.is_quantizer_trained() and one.is_quantizer_trained()
    for nq in (37, 1):
        assert rep.search_batch_int8(qs[:nq], k, ef) == one.search_batch_int8(qs[:nq], k, ef), nq
        assert_same(rep._search_raw(qs[:nq], k, ef, va.MODE_HNSW_INT8), one._search_raw(qs[:nq], k, ef, va.MODE_HNSW_INT8), ("int8 walk", nq))
    assert rep.last_kernels() & va.index.KERNEL_HNSW_INT8
    for cfg in (va.DualPrecisionConfig(min_index_size=100), va.DualPrecisionConfig(oversampling_ratio=2, min_index_size=100),
                va.DualPrecisionConfig(), va.DualPrecisionConfig(use_int8_traversal=False, min_index_size=100)):
        for qi in range(4):
            a, b = rep.search_with_config(qs[qi], k, ef, cfg), one.search_with_config(qs[qi], k, ef, cfg)
            assert len(b) == k and [i for i, _ in a] == [i for i, _ in b], (cfg, qi)
            assert np.array_equal(bits([s for _, s in a]), bits([s for _, s in b])), (cfg, qi)
    rep.close()
    one.close()


def test_range_group_refuses_the_quantizer(gpu_required):
    rng = np.random.default_rng(22)
    sh = group(16, DM.Cosine, 200, 2)
    sh.upload(np.arange(200), rng.standard_normal((200, 16)).astype(np.float32))
    with pytest.raises(va.VelesHipError) as e:
        sh.train_quantizer()
    assert e.value.code == UNSUPPORTED
    assert not sh.is_quantizer_trained()
    with pytest.raises(va.VelesHipError) as e:
        sh.search_batch_int8(np.ones((2, 16), np.float32), 5, 64)
    assert e.value.code == UNSUPPORTED
    sh.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. riders on the same kind of handle
@pytest.mark.parametrize("metric", [DM.Euclidean, DM.Cosine])
def test_sweep_engine_option_reaches_every_shard(gpu_required, metric):
    rng = np.random.default_rng(1000 + int(metric))
    n, dim, shards, nq, k = 3000, 96, 3, 70, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    sh = group(dim, metric, n, shards)
    assert sh.upload(ids, rows) == n
    info = sh.shard_info()
    assert info["n_shards"] == shards and info["shard_mode"] == va.SHARD_RANGE and info["rank"] == 0 and info["world"] == 1
    assert info["transport"] == ("rccl" if va.device_count() >= shards else "d2d-copy")
    before = sh.search_batch_brute_force(qs, k)
    assert sh.last_kernels() & MATRIX_F32, f"{sh.last_kernels():#x}"
    assert_same(before, r_oracle("f32", metric, rows, ids, qs, k, oracle_mode(sh, k)), (metric, "engine 1"))
    sh.set_option(va.OPT_SWEEP_ENGINE, 0)
    assert sh.get_option(va.OPT_SWEEP_ENGINE) == 0 and sh.sweep_arith_mode(k) == "C"
    after = sh.search_batch_brute_force(qs, k)
    mask = sh.last_kernels()
    assert not mask & MATRIX_F32 and mask & va.index.KERNEL_SWEEP_VALU, f"{mask:#x}"
    # every shard switched: the vector-ALU kernels' summation order (oracle mode C) on all rows — a shard left on the matrix cores
    # would keep mode M bits for Cosine
    assert_same(after, r_oracle("f32", metric, rows, ids, qs, k, po.MODE_C), (metric, "engine 0"))
    if metric == DM.Euclidean:                    # one summation order on both engines: the same bits
        assert_same(after, before, "engine 0 against engine 1")
    sh.set_option(va.OPT_SWEEP_ENGINE, -1)
    assert_same(sh.search_batch_brute_force(qs, k), before, (metric, "back to the default"))
    assert sh.last_kernels() & MATRIX_F32
    sh.close()
