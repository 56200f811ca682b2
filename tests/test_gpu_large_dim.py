"""GPU parity tests of exact search at the embedding sizes the reference is configured for: up to `max_dimensions: 4096` by default
(velesdb-core config.rs), 1 536 / 3 072 / 4 096 in common use.  Every LDS budget of the batch path depends on dim, and above ~2 K
the dispatch changes route with it:
- Cosine / DotProduct take the WIDE selection only while the gathered exact pass (the streaming matrix-core kernel, one 16-query
  tile: 8 KiB of LDS per 128 elements) fits 160 KiB — every k up to dim 2 048, k <= 62 at dim 2 432, never from dim 2 560;
- Euclidean takes it over the augmented form whenever dim % 64 == 0; its unproven queries go through the vector-ALU sweep with an
  8-query tile in LDS (32 B per element): above the default 64 KiB from dim 2 048 (dim 1 792 at k = 128), and above the 160 KiB a
  block may have from dim ~4 860 at k = 128 — there the batch takes the exact kernels;
- the exact vector-ALU kernels keep the query tile in LDS and shrink it to fit.

Bar, as for every exact path: ids, ranks, counts and score BITS of the oracle's restatement (mode M where the matrix-core kernel is
the exact path, C otherwise: `sweep_arith_mode`), and `last_select_level()` equal to the table below — written out here, not read
back from the library, so that a shape cannot take the exact kernels unnoticed and pass for coverage of the selection stage.

The corpora are embedding-like: a 64-dimensional latent spread over all dims, plus a little isotropic noise.  (On i.i.d. Gaussian
rows the distances of a 3 072- or 4 096-dim corpus concentrate so tightly that the Euclidean WIDE bound proves only about half of
the queries: the results stay exact through the gathered pass, but the handle then parks at levels 2 / 0 and the level a batch
takes depends on the batches before it.)

The oracle's order is total (score, then row id: vo_scan_topk's comparator), so the top-128 list of a query starts with its top-k
list for every k: one oracle call per (metric, dim, mode, query set) at k = 128 serves every k of that set."""
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
PO = {DM.Cosine: po.COSINE, DM.DotProduct: po.DOT, DM.Euclidean: po.EUCLIDEAN, DM.Hamming: po.HAMMING, DM.Jaccard: po.JACCARD}
N = 65_536 + 37          # just above the selection stage's smallest corpus (kGemmBf16MinRows), a ragged last tile
KMAX = 128
NQ = 300
CD = (DM.Cosine, DM.DotProduct)
EU = (DM.Euclidean,)
ALL_K = (1, 128)

# (metrics, dim, k range, level) — the level that serves a batch of >= 16 queries at selector level 3 (the default)
LEVELS = [
    (CD, 1536, ALL_K, 4),      # 12 k-units x 8 KiB + 16 k keys: the gathered matrix-core pass fits 160 KiB at every k -> WIDE (k <= 10 too)
    (CD, 1792, ALL_K, 4),      # 14 k-units = 112 KiB + 16 KiB of keys at k = 128: fits -> WIDE
    (CD, 2048, ALL_K, 4),      # 16 k-units = 128 KiB + 16 KiB of keys at k = 128: fits -> WIDE
    (CD, 2432, (1, 62), 4),    # 19 k-units = 152 KiB + 128 k + 192 B: fits up to k = 62 -> WIDE
    (CD, 2432, (63, 128), 0),  # ... and not from k = 63: no matrix-core exact kernel either -> the exact vector-ALU kernels
    (CD, 3072, ALL_K, 0),      # 24 k-units = 192 KiB: never fits -> the exact vector-ALU kernels
    (CD, 4096, ALL_K, 0),      # 32 k-units = 256 KiB: never fits -> the exact vector-ALU kernels
    (CD, 2500, ALL_K, 0),      # not a multiple of 64: no bf16 image (and 20 k-units: no matrix-core kernel) -> exact vector-ALU kernels
    (CD, 4095, ALL_K, 0),      # not a multiple of 64 -> the exact vector-ALU kernels
    (EU, 1536, ALL_K, 4),      # augmented form; gathered vector-ALU pass 64 k + 64 + 32 dim B = 56 KiB at k = 128 -> WIDE
    (EU, 1792, ALL_K, 4),      # 64 KiB + 64 B at k = 128: above the default LDS window, inside 160 KiB -> WIDE
    (EU, 2048, ALL_K, 4),      # 64 KiB + 64 k + 64 B: above the default window at every k, inside 160 KiB -> WIDE
    (EU, 2432, ALL_K, 4),      # 76 KiB + 64 k + 64 B -> WIDE
    (EU, 3072, ALL_K, 4),      # 96 KiB + 64 k + 64 B -> WIDE
    (EU, 4096, ALL_K, 4),      # 128 KiB + 64 k + 64 B: 136 KiB at k = 128 -> WIDE
    (EU, 4928, (1, 10), 4),    # 154 KiB + 64 k + 64 B: 155 KiB at k = 10 -> WIDE
    (EU, 4928, (11, 128), 0),  # ... 162 KiB at k = 128: the gathered pass cannot launch -> the exact kernels, not an error
    (EU, 2500, ALL_K, 0),      # not a multiple of 64: no augmented image -> the exact vector-ALU kernels
    (EU, 4095, ALL_K, 0),      # not a multiple of 64 -> the exact vector-ALU kernels
]


def expected_level(metric, dim, k):
    rows = [lv for ms, d, (lo, hi), lv in LEVELS if metric in ms and d == dim and lo <= k <= hi]
    assert len(rows) == 1, f"no single row of the level table for {metric} dim {dim} k {k}"
    return rows[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mode_of(ix, metric, k):
    if metric == DM.Euclidean:
        return po.MODE_C
    return po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C


def embedding_like(rng, n, dim, out=None, latent=64):
    """rows z W + 0.05 e: z ~ N(0, I_latent), W ~ N(0, 1 / latent) (unit variance per element), e ~ N(0, I_dim); in chunks"""
    w = (rng.standard_normal((latent, dim), dtype=np.float32) / np.float32(np.sqrt(latent)))
    out = np.empty((n, dim), dtype=np.float32) if out is None else out
    for r0 in range(0, n, 16_384):
        r1 = min(n, r0 + 16_384)
        out[r0:r1] = rng.standard_normal((r1 - r0, latent), dtype=np.float32) @ w
        out[r0:r1] += np.float32(0.05) * rng.standard_normal((r1 - r0, dim), dtype=np.float32)
    return out


@functools.lru_cache(maxsize=2)
def dense(dim, n=N, seed=0):
    """(rows, queries) of one dim, built once and shared by the tests of that dim"""
    rng = np.random.default_rng(seed * 100_003 + dim)
    rows = embedding_like(rng, n + NQ, dim)
    return rows[:n], rows[n:]


_oracle = {}


def oracle(metric, rows, qs, mode, tag):
    """top-KMAX of every query in qs, once per (metric, corpus tag, mode, query count); prefixes serve smaller k and batches"""
    key = (int(metric), tag, mode, qs.shape[0])
    if key not in _oracle:
        _oracle[key] = po.scan_topk(PO[metric], rows, qs, KMAX, mode, nthreads=po.host_threads())
    return _oracle[key]


@pytest.fixture(autouse=True)
def _drop_oracle_results_of_other_dims():
    yield
    if len(_oracle) > 64:
        _oracle.clear()


def check(ix, metric, rows, qs, k, tag, level, nq=None):
    q = qs if nq is None else qs[:nq]
    ids, sc, cnt = ix.search_batch_brute_force(q, k)
    got = ix.last_select_level()
    assert got == level, (f"{metric} dim {rows.shape[1]} k {k} nq {q.shape[0]}: select level {got}, the table says {level} "
                          f"(last selection batch: {ix.last_split_stats()} queries / unproven)")
    eid, esc = oracle(metric, rows, qs, mode_of(ix, metric, k), tag)
    eid, esc = eid[:q.shape[0], :k], esc[:q.shape[0], :k]
    assert np.all(cnt == k)
    assert np.array_equal(ids, eid), f"{metric} dim {rows.shape[1]} k {k} nq {q.shape[0]}: ids / ranks differ from the oracle"
    assert np.array_equal(bits(sc), bits(esc)), f"{metric} dim {rows.shape[1]} k {k} nq {q.shape[0]}: score bits differ from the oracle"
    return ids, sc


def new_index(dim, metric, rows):
    ix = va.HnswIndex(dim, metric)
    ix.upload(np.arange(rows.shape[0], dtype=np.uint64), rows)
    return ix


# ------------------------------------------------------------------------------------------------ (a) dense f32 batches
DENSE_K = {2432: (1, 10, 11, 62, 63, 100, 128)}
BIG_BATCH_DIMS = (2048, 2432, 4095, 4096)   # nq = 300 (two query tiles) here; 17 (just above the selection chunk minimum) everywhere


@pytest.mark.parametrize("dim", [1536, 1792, 2048, 2432, 3072, 4096, 2500, 4095])
def test_dense_batches_vs_oracle(gpu_required, dim):
    rows, qs = dense(dim)
    for metric in (DM.Cosine, DM.DotProduct, DM.Euclidean):
        ix = new_index(dim, metric, rows)
        try:
            for k in DENSE_K.get(dim, (1, 10, 11, 100, 128)):
                for nq in ((17, NQ) if dim in BIG_BATCH_DIMS else (17,)):
                    check(ix, metric, rows, qs, k, ("dense", dim), expected_level(metric, dim, k), nq)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ (b) selector levels
@pytest.mark.parametrize("dim", [2048, 4096])
def test_selector_levels_agree(gpu_required, dim):
    """selector level 2 (block-local lists for k <= 10) and 0 (no selection stage) give the bits of the default level and the oracle's"""
    rows, qs = dense(dim)
    for metric in (DM.Cosine, DM.DotProduct, DM.Euclidean):
        ix = new_index(dim, metric, rows)
        try:
            for k in (10, 50):
                ref = check(ix, metric, rows, qs, k, ("dense", dim), expected_level(metric, dim, k))
                # level 2 at k <= 10: the block-local lists where a matrix-core exact kernel exists (Cosine / DotProduct up to dim
                # 2 432), the augmented form's for Euclidean; k > 10 keeps the WIDE selection
                lv2 = expected_level(metric, dim, k) if k > 10 else (2 if (metric == DM.Euclidean or dim <= 2048) else 0)
                try:
                    va.set_split_selector(2)
                    got = check(ix, metric, rows, qs, k, ("dense", dim), lv2)
                    assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1]))
                    va.set_split_selector(0)
                    got = check(ix, metric, rows, qs, k, ("dense", dim), 0)
                    assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1]))
                finally:
                    va.set_split_selector(3)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ (c) the gathered exact pass runs
@pytest.mark.parametrize("dim", [2048, 4096])
def test_gathered_exact_pass_with_listed_queries(gpu_required, dim):
    """near-copies of query 5 (distances far below the augmented form's error bound) and a cluster around query 6 tighter than the
    bf16 bound and larger than a query's list: both queries stay unproven, and the gathered exact pass answers them — as few of the
    64 as leave the handle on the selection stage (<= 1/16)"""
    base, qs0 = dense(dim)
    qs = qs0[:64]
    rng = np.random.default_rng(dim + 5)
    rows = base.copy()
    rows[500:540] = qs[5] + 1e-3 * rng.standard_normal((40, dim), dtype=np.float32)
    rows[20_000:24_500] = qs[6] + 1e-3 * rng.standard_normal((4500, dim), dtype=np.float32)
    cases = [(DM.Euclidean, (10, 128))] + ([(DM.Cosine, (128,))] if dim == 2048 else [])   # (Cosine at k = 128: one 16-query tile per pass)
    try:
        for metric, ks in cases:
            ix = new_index(dim, metric, rows)
            try:
                for k in ks:
                    check(ix, metric, rows, qs, k, ("planted", dim), expected_level(metric, dim, k))
                    nq_l, unproven = ix.last_split_stats()
                    assert nq_l == 64 and 0 < unproven <= 4, f"{metric} dim {dim} k {k}: {unproven} of {nq_l} queries unproven"
            finally:
                ix.close()
    finally:
        for key in [key for key in _oracle if key[1] == ("planted", dim)]:
            del _oracle[key]


# ------------------------------------------------------------------------------------------------ (d) other result modes
@pytest.mark.parametrize("dim", [2048, 4096])
def test_sq8_storage_mode(gpu_required, dim):
    """StorageMode::SQ8: the reference's asymmetric chain over the codes, bit for bit.  Cosine / DotProduct batches take the WIDE
    selection over the dequantised image at k = 10 and 100; Euclidean has the block-local lists (level 3) at k <= 10 and the exact SQ8
    sweep above"""
    rows, qs0 = dense(dim)
    qs = qs0[:32]
    for metric in (DM.Cosine, DM.DotProduct, DM.Euclidean):
        ix = va.HnswIndex(dim, metric)
        ix.set_storage_mode(va.StorageMode.SQ8)
        ix.upload(np.arange(rows.shape[0], dtype=np.uint64), rows)
        try:
            eid, esc = po.scan_topk_sq8(PO[metric], rows, qs, 100, nthreads=po.host_threads())
            for k in (10, 100):
                ids, sc, cnt = ix.search_batch_sq8(qs, k)
                level = 4 if metric != DM.Euclidean else (3 if k <= 10 else 0)
                assert ix.last_select_level() == level, (metric, dim, k, ix.last_select_level())
                assert np.all(cnt == k)
                assert np.array_equal(ids, eid[:, :k].astype(np.uint64)), f"SQ8 {metric} dim {dim} k {k}: ids / ranks differ"
                assert np.array_equal(bits(sc), bits(esc[:, :k])), f"SQ8 {metric} dim {dim} k {k}: score bits differ"
        finally:
            ix.close()


@pytest.mark.parametrize("dim", [4096, 4095])
@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct])
def test_bf16_result_mode(gpu_required, dim, metric):
    """search_batch_brute_force_bf16 (half_precision.rs semantics: bf16-rounded rows and queries, f32 sums in an order the matrix
    core decides): every score within 1e-5 of the f64 score of the bf16 values, best first, nothing better missed, ranks equal to
    the oracle's wherever its neighbouring scores are further apart than that — the streaming kernel (3 queries) and the
    GEMM-structured one (>= 64 queries, dim % 64 == 0)"""
    n = 5000
    rng = np.random.default_rng(dim + int(metric))
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    ix = va.HnswIndex(dim, metric)
    ix.upload(np.arange(n, dtype=np.uint64), rows)
    ix.enable_bf16()
    rr = po.round_bf16(rows).astype(np.float64)
    try:
        for nq, k in ((3, 10), (3, 100), (100, 10), (100, 100)):
            qs = rng.standard_normal((nq, dim), dtype=np.float32)
            gi, gs, gc = ix.search_batch_brute_force_bf16(qs, k)
            eid, esc = po.scan_topk_bf16(PO[metric], rows, qs, k, nthreads=po.host_threads())
            qq = po.round_bf16(qs).astype(np.float64)
            full = qq @ rr.T
            if metric == DM.Cosine:
                full /= np.linalg.norm(qq, axis=1)[:, None] * np.linalg.norm(rr, axis=1)[None, :]
                scale = np.ones_like(full)
            else:
                scale = np.linalg.norm(qq, axis=1)[:, None] * np.linalg.norm(rr, axis=1)[None, :]
            tol = 1e-5
            assert np.all(gc == k)
            for qi in range(nq):
                g_i, g_s = gi[qi].astype(np.int64), gs[qi].astype(np.float64)
                assert np.all(np.abs(g_s - full[qi, g_i]) <= tol * scale[qi, g_i]), (dim, metric, nq, k, qi)
                assert np.all(np.diff(g_s) <= 1e-12)
                assert g_s[-1] >= np.sort(full[qi])[::-1][k - 1] - tol * scale[qi].max()
                e_i = eid[qi].astype(np.int64)
                for r in range(k):
                    if g_i[r] != e_i[r]:
                        assert abs(float(esc[qi, r]) - full[qi, g_i[r]]) <= 2 * tol * scale[qi, g_i[r]], (dim, metric, nq, k, qi, r)
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [DM.Hamming, DM.Jaccard])
def test_bit_metrics_at_dim_4096(gpu_required, metric):
    """Hamming / Jaccard over 128-word rows: 40 queries at k = 1 over >= 65 536 rows on the four-bit GEMM, the rest on the vector-ALU kernels —
    integer scores, ids and ranks (ties by row) equal to the oracle's"""
    dim = 4096
    rng = np.random.default_rng(4096 + int(metric))
    rows = (rng.random((N, dim)) > 0.6915).astype(np.float32)
    rows[1000:1040] = rows[999]                       # exact ties across one tile
    qs = (rng.random((40, dim)) > 0.6915).astype(np.float32)
    qs[1] = rows[999]
    ix = new_index(dim, metric, rows)
    try:
        eid, esc = po.scan_topk(PO[metric], rows, qs, KMAX, po.MODE_C, nthreads=po.host_threads())
        for nq in (40, 4):
            for k in ALL_K:
                ids, sc, cnt = ix.search_batch_brute_force(qs[:nq], k)
                if nq >= 32 and k <= 10:       # (the four-bit GEMM keeps k <= 10; k = 128 and small batches: the vector-ALU kernels)
                    assert ix.last_kernels() & va.KERNEL_BITS_GEMM, "the matrix-core path did not serve the batch"
                assert np.all(cnt == k)
                assert np.array_equal(ids, eid[:nq, :k]), f"{metric} nq {nq} k {k}: ids / ranks differ"
                assert np.array_equal(bits(sc), bits(esc[:nq, :k])), f"{metric} nq {nq} k {k}: score bits differ"
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ (e) batches below the selection chunk
@pytest.mark.parametrize("dim", [4096, 4095])
def test_small_batches_shrink_the_tile(gpu_required, dim):
    """1 / 2 / 15 queries: the exact vector-ALU kernel with its query tile shrunk to the LDS window; a query alone gives the bits it
    gets inside a batch of 300"""
    rows, qs = dense(dim)
    for metric in (DM.Cosine, DM.DotProduct, DM.Euclidean):
        ix = new_index(dim, metric, rows)
        try:
            for k in ALL_K:
                for nq in (1, 2, 15):
                    check(ix, metric, rows, qs, k, ("dense", dim), 0, nq)
                big, sbig = check(ix, metric, rows, qs, k, ("dense", dim), expected_level(metric, dim, k))
                for qi in (0, 7, 299):
                    one, s1, _ = ix.search_batch_brute_force(qs[qi:qi + 1], k)
                    assert np.array_equal(one[0], big[qi]) and np.array_equal(bits(s1[0]), bits(sbig[qi])), (metric, dim, k, qi)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ the 160 KiB guard
def test_euclidean_beyond_the_gathered_pass_lds(gpu_required):
    """dim 4 928 (a multiple of 64; the reference allows up to 65 536): at k = 128 the gathered vector-ALU pass of the WIDE selection
    would need 162 KiB of LDS — the batch comes back exact from the exact kernels; at k = 10 (155 KiB) the WIDE selection serves"""
    dim = 4928
    rng = np.random.default_rng(dim)
    rows = embedding_like(rng, N + 32, dim)
    rows, qs = rows[:N], rows[N:]
    ix = new_index(dim, DM.Euclidean, rows)
    try:
        for k in (128, 10):
            check(ix, DM.Euclidean, rows, qs, k, ("dense", dim), expected_level(DM.Euclidean, dim, k))
    finally:
        ix.close()
        _oracle.clear()


# ------------------------------------------------------------------------------------------------ (f) HNSW at dim 3072
def test_hnsw_at_dim_3072(gpu_required, tmp_path):
    """graph search on an oracle-built graph (ids, distance bits, counters) and a sequential GPU build link for link, at a dim whose
    query no longer fits the kernels' register layout.  The dual-precision (int8) walk keeps its query codes in registers up to dim
    1 024: above, training the quantiser is refused with an error, never answered approximately."""
    dim, n, M, efc = 3072, 3000, 8, 40
    rng = np.random.default_rng(3072)
    rows = embedding_like(rng, n + 12, dim)
    rows, qs = rows[:n], rows[n:]
    for metric in (DM.Cosine, DM.Euclidean, DM.DotProduct):
        g = po.NativeHnsw(dim, PO[metric], M, efc, po.MODE_C)
        for v in rows:
            g.insert(v)
        d = tmp_path / f"m{int(metric)}"
        d.mkdir()
        g.file_dump(str(d), "native_hnsw")
        ix = va.HnswIndex(dim, metric, va.HnswParams(M, efc, n))
        ix.load_reference_files(str(d), "native_hnsw")
        try:
            for k, ef in ((10, 64), (1, 16), (50, 200)):
                res = ix.search_batch_parallel(qs, k, va.SearchQuality.Custom(ef))
                nd_gpu, ne_gpu = ix.last_search_stats()
                nd = ne = 0
                for qi, q in enumerate(qs):
                    oid, od = g.search(q, k, ef, po.TIE_CANONICAL)
                    a, b = po.NativeHnsw.last_stats()
                    nd, ne = nd + a, ne + b
                    osc = np.array([po.transform_score(PO[metric], float(x)) for x in od], dtype=np.float32)
                    assert [r[0] for r in res[qi]] == oid.tolist(), (metric, k, ef, qi)
                    assert np.array_equal(bits([r[1] for r in res[qi]]), bits(osc)), (metric, k, ef, qi)
                assert (nd_gpu, ne_gpu) == (nd, ne), "distance-evaluation / expansion counters differ from the oracle"
            if metric == DM.Euclidean:
                with pytest.raises(va.VelesHipError, match="dim > 1024"):
                    ix.train_quantizer()
        finally:
            ix.close()
    # sequential insert on the GPU: the oracle's graph link for link (canonical tie order)
    m = 600
    for metric in (DM.Cosine, DM.Euclidean):
        g = po.NativeHnsw(dim, PO[metric], M, efc, po.MODE_C)
        g.set_build_tie(po.TIE_CANONICAL)
        ix = va.HnswIndex(dim, metric, va.HnswParams(M, efc, m))
        try:
            for i in range(m):
                g.insert(rows[i])
                ix.insert(i, rows[i])
            nl, ml, ep = ix.graph_info()
            assert (nl, ml, ep) == (g.num_layers, g.max_layer, g.entry_point)
            for layer in range(g.num_layers):
                for node in range(m):
                    assert ix.neighbors(layer, node) == g.neighbors(layer, node), (metric, layer, node)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ (g) rows beyond 4 GiB
def _mem_available():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_rows_beyond_4_gib(gpu_required, metric):
    """270 000 x 4 096 f32 rows = 4.1 GiB: byte offsets of the last rows exceed 2^32 in the exact kernels and, for Euclidean, in the
    WIDE selection's re-scoring and gathered exact pass (near-copies of query 5 placed beyond the 4-GiB line: its best rows lie there)"""
    n, dim, nq = 270_000, 4096, 64
    need = n * dim * 4 + (1 << 30)
    avail = _mem_available()
    if avail is not None and avail < need + (4 << 30):
        pytest.skip(f"host memory: {avail >> 20} MiB available, this case needs about {(need + (4 << 30)) >> 20} MiB")
    rng = np.random.default_rng(270_000 + int(metric))
    try:
        both = np.empty((n + nq, dim), dtype=np.float32)
    except MemoryError:
        pytest.skip("host memory: the 4.1 GiB corpus could not be allocated")
    embedding_like(rng, n + nq, dim, out=both)
    rows, qs = both[:n], both[n:].copy()
    rows[n - 40:] = qs[5] + 1e-3 * rng.standard_normal((40, dim), dtype=np.float32)
    ix = new_index(dim, metric, rows)
    try:
        eid, esc = po.scan_topk(PO[metric], rows, qs, 100, mode_of(ix, metric, 100), nthreads=po.host_threads())
        for k in (100, 10):
            ids, sc, cnt = ix.search_batch_brute_force(qs, k)
            assert ix.last_select_level() == expected_level(metric, dim, k), (metric, k, ix.last_select_level())
            assert np.all(cnt == k)
            assert np.array_equal(ids, eid[:, :k]), f"{metric} k {k}: ids / ranks differ from the oracle"
            assert np.array_equal(bits(sc), bits(esc[:, :k])), f"{metric} k {k}: score bits differ from the oracle"
        assert eid[5, 0] >= n - 40
    finally:
        ix.close()
        del rows, both
