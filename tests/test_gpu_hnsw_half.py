"""GPU tests of the graph search over the half-precision rows (VDB_SEARCH_HNSW_F16 / VDB_SEARCH_HNSW_BF16, csrc/hnsw_half.hip).

The walk's declared summation order is the f32 walk's (mode C), so over an image H it must equal, bit for bit, the oracle's mode-C
NativeHnsw::search over the vectors dequant(H) with the rounded query (tests/half_walk_ref.py makes that oracle graph by patching a
dump; tests/test_half_walk_ref_cpu.py checks the patching).  DotProduct / Euclidean: ids, ranks, score bits and the walk's counters on
N(0,1) data; Cosine: the same on data where every sum is exact (the reference's rule for tiny norms differs from the f32 walk's, and
its order of summation does not matter there), and by the tolerance of tests/test_gpu_half_precision.py on N(0,1) data.
Shapes are those of tests/test_gpu_int8.py: the smallest that reach every instance (CPL 0 / CPL 3 / dim % 4 != 0, register and LDS
list).  One oracle graph and one GPU handle per (metric, shape), shared by the tests of this file.
"""
import ctypes as C
import os

import numpy as np
import pytest

import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po
from test_gpu_half_precision import TOL

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP, SQ = va.DistanceMetric, va.VectorPrecision, va.SearchQuality
METRIC = {hr.COSINE: DM.Cosine, hr.EUCLIDEAN: DM.Euclidean, hr.DOT: DM.DotProduct}
VPREC = {hr.F16: VP.F16, hr.BF16: VP.BF16}
MODE = {hr.F16: va.MODE_HNSW_F16, hr.BF16: va.MODE_HNSW_BF16}
BASE = "native_hnsw"
PRECISIONS = [hr.F16, hr.BF16]


class World:
    """N(0,1) rows and queries, the oracle graph on the f32 rows, its dump, one GPU handle with both images, and — per precision —
    the patched dump, the oracle graph over the rounded vectors and the half walk's answers."""

    def __init__(self, root, metric, shape, rows=None, qs=None, tag="n01"):
        n, dim, M, efc = shape
        self.metric, self.shape, self.dim = metric, shape, dim
        rng = np.random.default_rng(1000 * metric + n + dim)
        self.rows = rng.standard_normal((n, dim)).astype(np.float32) if rows is None else rows
        self.qs = rng.standard_normal((hw.NQ, dim)).astype(np.float32) if qs is None else qs
        self.g = hw.build_graph(self.rows, metric, M, efc)
        self.dir = os.path.join(root, f"{tag}_m{metric}_{n}_{dim}")
        os.makedirs(self.dir)
        self.g.file_dump(self.dir, BASE)
        self.ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
        self.ix.load_reference_files(self.dir, BASE)
        self._patched, self._answers, self.enabled = {}, {}, set()

    def enable(self, precision):
        if precision not in self.enabled:
            self.ix.enable_half_precision(VPREC[precision])
            self.enabled.add(precision)

    def patched(self, precision):
        if precision not in self._patched:
            d = f"{self.dir}_p{precision}"
            hw.patch_vectors(self.dir, d, BASE, precision)
            self._patched[precision] = (d, hw.load_graph(d, BASE, self.metric, self.dim))
        return self._patched[precision]

    def answers(self, precision, k, ef):
        """(results, counters, kernel bits) of the half walk for the UNROUNDED queries"""
        key = (precision, k, ef)
        if key not in self._answers:
            self.enable(precision)
            res = self.ix.search_batch_half_graph(self.qs, k, ef, VPREC[precision])
            self._answers[key] = (res, self.ix.last_search_stats(), self.ix.last_kernels())
        return self._answers[key]


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root, cache = str(tmp_path_factory.mktemp("half_walk")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = World(root, metric, shape)
        return cache[(metric, shape)]
    get.root = root
    yield get
    for w in cache.values():
        w.ix.close()


def ids_of(res):
    return [[r[0] for r in one] for one in res]


def bits_of(res):
    return [hw.bits([r[1] for r in one]) for one in res]


def assert_same(res, want_ids, want_bits, ctx):
    assert len(res) == len(want_ids)
    for qi, (gi, gb) in enumerate(zip(ids_of(res), bits_of(res))):
        assert gi == want_ids[qi], (ctx, qi)
        assert np.array_equal(gb, want_bits[qi]), (ctx, qi)


# ---- 1. the image is what the walk reads; bits equal the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", [hr.DOT, hr.EUCLIDEAN])
def test_half_walk_bits_equal_the_oracle_over_the_rounded_vectors(worlds, metric, shape, precision):
    w = worlds(metric, shape)
    _, g_half = w.patched(precision)
    qr = hr.round_half(w.qs, precision)
    assert not np.array_equal(hw.bits(qr), hw.bits(w.qs))
    differs = False
    for k, ef in hw.KEF:
        res, stats, kern = w.answers(precision, k, ef)
        oid, obits, ostats = hw.oracle_walk(g_half, metric, qr, k, ef)
        print(f"metric {metric} shape {shape} precision {precision} k {k} ef {ef}: counters gpu {stats} oracle {ostats}")
        assert_same(res, oid, obits, (k, ef))
        assert stats == ostats, (k, ef)
        assert kern & va.KERNEL_HNSW_HALF and not kern & (va.KERNEL_HNSW | va.KERNEL_HNSW_INT8), hex(kern)
        assert bool(kern & va.KERNEL_F16) == (precision == hr.F16), hex(kern)
        f32 = w.ix.search_batch_parallel(w.qs, k, SQ.Custom(ef))             # the same handle's f32 rows: another answer
        assert w.ix.last_kernels() & va.KERNEL_HNSW
        differs |= any(a.size != b.size or not np.array_equal(a, b) for a, b in zip(bits_of(res), bits_of(f32)))
    assert differs, "the half walk answered with the f32 walk's score bits: the f32 rows were read"


# ---- 2. Cosine ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
def test_cosine_bit_exact_on_exact_data(worlds, shape, precision):
    n, dim, M, efc = shape
    rng = np.random.default_rng(50 + n + precision)
    rows, qs = hw.grid(rng, (n, dim), precision), hw.grid(rng, (hw.NQ, dim), precision)
    w = World(worlds.root, hr.COSINE, shape, rows, qs, tag=f"grid{precision}")      # (tie-rich on purpose; its own handle)
    try:
        for k, ef in hw.KEF:
            res, stats, kern = w.answers(precision, k, ef)
            oid, obits, ostats = hw.oracle_walk(w.g, hr.COSINE, qs, k, ef)           # g_half = g: the grid is representable
            print(f"cosine grid shape {shape} precision {precision} k {k} ef {ef}: counters gpu {stats} oracle {ostats}")
            assert_same(res, oid, obits, (k, ef))
            assert stats == ostats, (k, ef)
            assert kern & va.KERNEL_HNSW_HALF and bool(kern & va.KERNEL_F16) == (precision == hr.F16)
    finally:
        w.ix.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
def test_cosine_scores_within_tolerance_on_gaussian_data(worlds, shape, precision):
    w = worlds(hr.COSINE, shape)
    full, _ = hr.truth64(hr.COSINE, precision, w.rows, w.qs)          # f64 cosine of the ROUNDED values
    for k, ef in hw.KEF:
        res, _, kern = w.answers(precision, k, ef)
        assert kern & va.KERNEL_HNSW_HALF
        worst = 0.0
        for qi, one in enumerate(res):
            assert len(one) == k and len({i for i, _ in one}) == k
            for i, s in one:
                worst = max(worst, abs(s - min(max(full[qi, i], 0.0), 1.0)))     # transform_score clamps 1 - d to [0, 1]
        print(f"cosine n01 shape {shape} precision {precision} k {k} ef {ef}: worst |score - f64| {worst:.3g}")
        assert worst <= TOL, (k, ef, worst)


# ---- 3. GPU-to-GPU identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", hw.SHAPES)
@pytest.mark.parametrize("metric", [hr.DOT, hr.EUCLIDEAN])
def test_half_walk_equals_the_f32_walk_over_the_dequantised_rows(worlds, metric, shape, precision):
    n, dim, M, efc = shape
    w = worlds(metric, shape)
    d, _ = w.patched(precision)
    ix2 = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
    try:
        ix2.load_reference_files(d, BASE)                                 # its f32 rows are dequant(H)
        qr = hr.round_half(w.qs, precision)
        for k, ef in hw.KEF:
            res, stats, _ = w.answers(precision, k, ef)
            f32 = ix2.search_batch_parallel(qr, k, SQ.Custom(ef))
            assert ix2.last_kernels() & va.KERNEL_HNSW
            assert_same(res, ids_of(f32), bits_of(f32), (k, ef))
            assert ix2.last_search_stats() == stats, (k, ef)
    finally:
        ix2.close()


# ---- 4. life cycle ------------------------------------------------------------------------------------------------------------------------
def latent_rows(rng, n, dim, latent=12):
    proj = rng.standard_normal((latent, dim)).astype(np.float32)
    return (rng.standard_normal((n, latent)).astype(np.float32) @ proj + 0.1 * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)


def test_life_cycle_inserts_removes_both_images_and_entry_points(tmp_path):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(4)
    n, dim, k = 1500, 96, 10
    rows = latent_rows(rng, n, dim)
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(8, 60, n))
    ix.insert_batch_parallel([(i, rows[i]) for i in range(1000)], 64)
    ix.enable_half_precision(VP.F16)
    ix.enable_half_precision(VP.BF16)
    ix.insert_batch_parallel([(i, rows[i]) for i in range(1000, n)], 128)           # rows that arrive AFTER the images were enabled
    # The late rows as queries: the walk ends next to them, so it reads their image rows.  Reference: the handle's own graph, dumped,
    # with the vectors rounded — the oracle's walk over it gives the ids, score bits and counters; where it finds the row itself, the
    # distance is exactly 0 (rounded query == rounded row), which only a converted image row gives.
    late = np.arange(1000, n, 25)
    saved = str(tmp_path / "saved")
    ix.save(saved, BASE)
    for prec in PRECISIONS:
        d = f"{saved}_p{prec}"
        hw.patch_vectors(saved, d, BASE, prec)
        g_half = hw.load_graph(d, BASE, hr.EUCLIDEAN, dim)
        oid, obits, ostats = hw.oracle_walk(g_half, hr.EUCLIDEAN, hr.round_half(rows[late], prec), 1, 128)
        res = ix.search_batch_half_graph(rows[late], 1, 128, VPREC[prec])
        assert_same(res, oid, obits, prec)
        assert ix.last_search_stats() == ostats
        found = [i for i, r in enumerate(res) if r[0][0] == late[i]]
        assert found and all(res[i][0][1] == 0.0 for i in found), prec
    qs = latent_rows(rng, 20, dim)
    a16 = ix.search_batch_half_graph(qs, k, 64, VP.F16)
    k16 = ix.last_kernels()
    ab = ix.search_batch_half_graph(qs, k, 64, VP.BF16)
    kb = ix.last_kernels()
    assert k16 & va.KERNEL_HNSW_HALF and k16 & va.KERNEL_F16 and kb & va.KERNEL_HNSW_HALF and not kb & va.KERNEL_F16
    assert any(not np.array_equal(x, y) for x, y in zip(bits_of(a16), bits_of(ab))), "each image gives its own answers"
    assert ix.search_batch_half_graph(qs, k, 64, VP.F16) == a16                      # (and the bf16 call did not disturb the f16 one)

    # nq = 1 through vdb_hip_index_search, 7 queries through the device-pointer entry point: the batch call's answers
    ids, sc, cnt = np.zeros(k, np.uint64), np.zeros(k, np.float32), C.c_uint32(0)
    va._ffi.check(va.lib().vdb_hip_index_search(ix._h, qs[3].ctypes.data_as(C.c_void_p), dim, k, 64, va.MODE_HNSW_F16,
                                                ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(cnt)))
    assert cnt.value == k and ids.tolist() == [r[0] for r in a16[3]] and np.array_equal(hw.bits(sc), bits_of(a16)[3])
    dq = torch.from_numpy(qs[:7].copy()).cuda()
    d_ids = torch.zeros((7, k), dtype=torch.int64, device="cuda")
    d_sc = torch.zeros((7, k), dtype=torch.float32, device="cuda")
    d_n = torch.zeros(7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_batch_dev(dq.data_ptr(), 7, k, 64, va.MODE_HNSW_BF16, d_ids.data_ptr(), d_sc.data_ptr(), d_n.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.all(d_n.cpu().numpy() == k)
    assert d_ids.cpu().numpy().astype(np.uint64).tolist() == ids_of(ab[:7])
    assert np.array_equal(d_sc.cpu().numpy().view(np.uint32), np.stack(bits_of(ab[:7])))

    # batches beyond one pass of the resident blocks (600 as the smallest; 1 100 is more than four blocks on each of 256 CUs):
    # a sample of 20 equals 20 single calls
    big = latent_rows(rng, 1100, dim)
    for nq in (600, 1100):
        res = ix.search_batch_half_graph(big[:nq], k, 64, VP.F16)
        for qi in np.linspace(0, nq - 1, 20).astype(int):
            assert ix.search_batch_half_graph(big[qi:qi + 1], k, 64, VP.F16)[0] == res[qi], (nq, qi)

    # a removed id never appears; the walk is unchanged (the node stays in the graph), the result shortens as in mode 2
    gone = a16[0][0][0]
    assert ix.remove(gone)
    after = ix.search_batch_half_graph(qs, k, 64, VP.F16)
    for qi in range(len(qs)):
        assert after[qi] == [r for r in a16[qi] if r[0] != gone], qi
    assert len(after[0]) == k - 1
    ix.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(va.VelesHipError) as e:
        fn()
    return e.value.code


def test_refusals_leave_the_handle_usable():
    rng = np.random.default_rng(5)
    n, dim, k = 600, 64, 5
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    items = [(i, rows[i]) for i in range(n)]
    ix = va.HnswIndex(dim, DM.DotProduct, va.HnswParams(8, 60, n))
    ix.insert_batch_parallel(items, 64)
    assert code_of(lambda: ix.search_batch_half_graph(qs, k, 64, VP.F16)) == -8          # mode 8 without the f16 image
    assert code_of(lambda: ix._search_raw(qs, k, 64, 10)) == -1                          # (and no mode 10)
    ix.enable_half_precision(VP.F16)
    assert code_of(lambda: ix.search_batch_half_graph(qs, k, 64, VP.BF16)) == -8         # mode 9 with only f16 enabled
    with pytest.raises(ValueError):
        ix.search_batch_half_graph(qs, k, 64, VP.F32)
    ok = ix.search_batch_half_graph(qs, k, 64, VP.F16)                                   # a later valid call works
    assert all(len(r) == k for r in ok) and ix.last_kernels() & va.KERNEL_HNSW_HALF
    # the entry points that carry no mode keep the f32 walk on a handle with an image: rerank, AUTO, multi-entry, with_config
    ix.search_with_rerank(qs[0], k, 20)
    assert not ix.last_kernels() & va.KERNEL_HNSW_HALF
    ix.search_with_quality(qs[0], k, SQ.Balanced)
    assert ix.last_kernels() & va.KERNEL_HNSW and not ix.last_kernels() & va.KERNEL_HNSW_HALF
    ix.search_multi_entry(qs, k, 64, 3)
    assert not ix.last_kernels() & va.KERNEL_HNSW_HALF
    ix.search_with_config(qs[0], k, 64)
    assert not ix.last_kernels() & va.KERNEL_HNSW_HALF
    assert ix.search_batch_half_graph(qs, k, 64, VP.F16) == ok

    nograph = va.HnswIndex(dim, DM.DotProduct, va.HnswParams(8, 60, n))                  # rows uploaded, graph not built
    nograph.upload(np.arange(n), rows)
    nograph.enable_half_precision(VP.F16)
    assert code_of(lambda: nograph.search_batch_half_graph(qs, k, 64, VP.F16)) == -8
    assert code_of(lambda: nograph.search_batch_parallel(qs, k, SQ.Custom(64))) == -8    # as VDB_SEARCH_HNSW
    assert np.all(nograph.search_batch_brute_force_half(qs, k, VP.F16)[2] == k)
    nograph.close()

    ham = va.HnswIndex(64, DM.Hamming, va.HnswParams(8, 60, 300))                        # cannot have an image
    ham.insert_batch_parallel([(i, (rows[i] > 0).astype(np.float32)) for i in range(300)], 64)
    hq = (qs > 0).astype(np.float32)
    assert code_of(lambda: ham.search_batch_half_graph(hq, k, 64, VP.F16)) == -8
    assert code_of(lambda: ham.search_batch_half_graph(hq, k, 64, VP.BF16)) == -8
    assert all(len(r) == k for r in ham.search_batch_parallel(hq, k, SQ.Custom(64)))
    ham.close()

    rng_group = va.HnswIndex(dim, DM.DotProduct, va.HnswParams(8, 60, n), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    rng_group.insert_batch_parallel(items, 64)
    rng_group.enable_half_precision(VP.F16)
    assert code_of(lambda: rng_group.search_batch_half_graph(qs, k, 64, VP.F16)) == -7
    assert np.all(rng_group.search_batch_brute_force(qs, k)[2] == k)
    rng_group.close()

    rep = va.HnswIndex(dim, DM.DotProduct, va.HnswParams(8, 60, n), devices=[0, 0], shard_mode=va.SHARD_REPLICA)
    rep.insert_batch_parallel(items, 64)
    rep.enable_half_precision(VP.F16)
    assert rep.search_batch_half_graph(qs, k, 64, VP.F16) == ok                          # the single handle's bits
    assert code_of(lambda: rep.search_batch_half_graph(qs, k, 64, VP.BF16)) == -8
    rep.close()
    ix.close()
