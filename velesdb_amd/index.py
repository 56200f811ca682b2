"""Host-side mirror of the reference's operator interface for the hot path, over the C ABI.

`HnswIndex` has the surface of crates/velesdb-core/src/index/hnsw/index/*.rs (the concrete
type `Collection` holds, core/collection/types.rs:146) and implements `VectorIndex`
(index/mod.rs:30-83): same method names, argument meaning, result conventions and panics
(as AssertionError with the reference's message).  `HipDistance` mirrors `DistanceEngine`
(native/distance.rs:14-28) and `GpuAccelerator` mirrors gpu/gpu_backend.rs:33-415.

All compute happens in libvelesdb_hip.so; this file only marshals numpy buffers.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import check, lib
from .params import DistanceMetric, DualPrecisionConfig, HnswParams, SearchQuality

MODE_AUTO, MODE_BRUTE, MODE_HNSW, MODE_BRUTE_BF16, MODE_HNSW_INT8, MODE_BRUTE_SQ8, MODE_BRUTE_BINARY, MODE_BRUTE_F16 = 0, 1, 2, 3, 4, 5, 6, 7
OPT_MAX_QUERY_TILE, OPT_SWEEP_ENGINE, OPT_SELECTOR_LEVEL, OPT_INT8_OVERSAMPLING, OPT_KERNEL_TIMING = 0, 1, 2, 3, 4
# the combining front of the host-pointer search entry points (include/velesdb_hip.h): queries per combined launch (0 = off),
# waiting window of a leader in microseconds, combined batches in flight
OPT_COMBINE_MAX_BATCH, OPT_COMBINE_WINDOW_US, OPT_COMBINE_INFLIGHT = 5, 6, 7
KIND_ENGINE, KIND_RAW = 0, 1
# enum vdb_kernel_bit (HnswIndex.last_kernels)
(KERNEL_SWEEP_VALU, KERNEL_SWEEP_MFMA_F32, KERNEL_GEMM_F32, KERNEL_SWEEP_MFMA_BF16, KERNEL_GEMM_BF16, KERNEL_GEMM_BF16_GLDS,
 KERNEL_SELECT_BF16, KERNEL_SELECT_SPLIT, KERNEL_BITS, KERNEL_SQ8, KERNEL_HNSW, KERNEL_HNSW_INT8, KERNEL_BITS_GEMM) = (1 << i for i in range(13))
# an f16 instance of a matrix-core family ran (set next to the family's bit); the half-row Euclidean sweep
KERNEL_F16, KERNEL_SWEEP_HALF_L2 = 1 << 13, 1 << 14
# graph search over the f16 / bf16 copy of the rows (VDB_SEARCH_HNSW_F16 / _BF16) and its kernel family
MODE_HNSW_F16, MODE_HNSW_BF16 = 8, 9
KERNEL_HNSW_HALF = 1 << 15
# filtered exact search (HnswIndex.create_filter / search_batch_brute_force_filtered): the route option (0 auto, 1 listed sweep,
# 2 mask substitution) and the listed sweep's kernel bit
OPT_FILTER_ROUTE = _ffi.VDB_OPT_FILTER_ROUTE
FILTER_ROUTE_AUTO, FILTER_ROUTE_LISTED, FILTER_ROUTE_MASK = 0, 1, 2
KERNEL_SWEEP_LISTED = _ffi.VDB_KERNEL_SWEEP_LISTED
# filtered graph search (HnswIndex.search_batch_filtered_graph): the route of a call / of a query, and the two kernel families
ROUTE_AUTO, ROUTE_WALK, ROUTE_EXACT = 0, 1, 2
KERNEL_HNSW_FILTERED = _ffi.VDB_KERNEL_HNSW_FILTERED
KERNEL_FILTER_RANK = _ffi.VDB_KERNEL_FILTER_RANK
# ... and the half walk whose candidates are re-scored over the f32 rows (HnswIndex.search_batch_with_filters_half_rescore)
KERNEL_HALF_RESCORE = _ffi.VDB_KERNEL_HALF_RESCORE
KERNEL_SWEEP_LISTED_GROUPS = _ffi.VDB_KERNEL_SWEEP_LISTED_GROUPS
# multi-query search with result fusion (HnswIndex.multi_query_search_ids / FusionStrategy.fuse): the fusion kernel's bit, the limits
KERNEL_FUSE = _ffi.VDB_KERNEL_FUSE
MAX_FUSED_VECTORS = 10      # MAX_VECTORS of multi_query_search (collection/search/batch.rs:238)
FUSE_MAX_RECORDS = 8192     # records of one group the fusion kernel takes (VDB_FUSE_MAX_RECORDS)
# hybrid search (HnswIndex.hybrid_search / hybrid_fuse_arrays): the kernel's bit, |V| + |T| of one query (VDB_HYBRID_MAX_RECORDS)
KERNEL_HYBRID_FUSE = _ffi.VDB_KERNEL_HYBRID_FUSE
HYBRID_MAX_RECORDS = 8192
# the rows the walks of hybrid_search_batch_filters / multi_query_search_batch_filters take their distances over (enum vdb_walk_rows)
WALK_ROWS_F32, WALK_ROWS_F16, WALK_ROWS_BF16, WALK_ROWS_INT8 = _ffi.VDB_WALK_ROWS_F32, _ffi.VDB_WALK_ROWS_F16, _ffi.VDB_WALK_ROWS_BF16, _ffi.VDB_WALK_ROWS_INT8
WALK_ROWS_F16_RESCORE, WALK_ROWS_BF16_RESCORE = _ffi.VDB_WALK_ROWS_F16_RESCORE, _ffi.VDB_WALK_ROWS_BF16_RESCORE
_PAD_ID = 0xFFFFFFFFFFFFFFFF  # what the library pads result ids with (the score beside it: NaN 0x7FC00000)
SHARD_REPLICA, SHARD_RANGE = 0, 1
COMM_ID_BYTES = 128


class VectorPrecision(enum.IntEnum):
    """VectorPrecision (half_precision.rs:36-44), the discriminants of enum vdb_vector_precision."""
    F32 = 0
    F16 = 1
    BF16 = 2


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    n = C.c_int32(0)
    check(lib().vdb_hip_device_count(C.byref(n)))
    return int(n.value)


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    check(lib().vdb_hip_device_name(device, buf, 256))
    return buf.value.decode()


def comm_unique_id() -> bytes:
    """The 128-byte id of a new one-process-per-GPU shard group (rank 0 makes it, every rank passes it to join_group)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib().vdb_hip_comm_unique_id(buf))
    return bytes(buf)


def set_kernel_timing(on: bool) -> None:
    check(lib().vdb_hip_set_kernel_timing(1 if on else 0))


def set_max_query_tile(b: int) -> None:
    """Tuning knob of the exact sweep: queries served per corpus pass (1..32).  Results do not depend on it."""
    check(lib().vdb_hip_set_max_query_tile(b))


def set_sweep_engine(engine: int) -> None:
    """0 = vector-ALU sweep kernels (oracle mode C), 1 = matrix-core kernel for Cosine/Dot (oracle mode M)."""
    check(lib().vdb_hip_set_sweep_engine(engine))


def set_split_selector(level) -> None:
    """Large exact cosine / dot batches: 0 / False = the exact f32 matrix-core kernel for the whole batch; 1 / True =
    split-bf16 selection + exact re-scoring + proof; 2 = plain bf16 selection first (block-local candidate lists for k <= 10, the WIDE
    selection for 10 < k <= 128), level 1 as the fallback level; 3 (the library's default) = level 2 with the WIDE selection at every
    k <= 128.  Results are identical at every level."""
    check(lib().vdb_hip_set_split_selector(int(level)))


class FusionError(ValueError):
    """FusionError (fusion/strategy.rs:10-34): the reference's messages."""


class FusionStrategy:
    """FusionStrategy (fusion/strategy.rs:46-79) with `fuse` on the device (vdb_hip_fuse_results).  Build one with Average(), Maximum(),
    RRF(k=60), rrf_default() or Weighted(avg, max, hit).  Fused lists come back descending by the total order of the fused score, equal
    scores by id ascending (the reference leaves ties to HashMap iteration); NaN weights are refused (the reference lets them through)."""

    def __init__(self, code: int, rrf_k: int = 0, weights=(0.0, 0.0, 0.0), name: str = ""):
        self.code, self.rrf_k, self.weights, self.name = code, rrf_k, tuple(np.float32(w) for w in weights), name

    def __repr__(self):
        return self.name

    def __eq__(self, other):
        return isinstance(other, FusionStrategy) and (self.code, self.rrf_k, self.weights) == (other.code, other.rrf_k, other.weights)

    def __hash__(self):
        return hash((self.code, self.rrf_k, self.weights))

    @classmethod
    def Average(cls) -> "FusionStrategy":
        return cls(_ffi.VDB_FUSION_AVERAGE, name="Average")

    @classmethod
    def Maximum(cls) -> "FusionStrategy":
        return cls(_ffi.VDB_FUSION_MAXIMUM, name="Maximum")

    @classmethod
    def RRF(cls, k: int = 60) -> "FusionStrategy":
        return cls(_ffi.VDB_FUSION_RRF, rrf_k=int(k), name=f"RRF(k={int(k)})")

    @classmethod
    def rrf_default(cls) -> "FusionStrategy":
        return cls.RRF(60)

    @classmethod
    def Weighted(cls, avg_weight: float, max_weight: float, hit_weight: float) -> "FusionStrategy":
        """FusionStrategy::weighted (strategy.rs:95-122): f32 arithmetic, the reference's messages; NaN is refused too."""
        a, m, h = np.float32(avg_weight), np.float32(max_weight), np.float32(hit_weight)
        for w in (a, m, h):
            if w < 0:
                raise FusionError(f"Weights must be non-negative, got {float(w):.4f}")
        total = np.float32(np.float32(a + m) + h)
        if np.isnan(total) or np.abs(np.float32(total - np.float32(1.0))) > np.float32(0.001):
            raise FusionError(f"Weights must sum to 1.0, got {float(total):.4f}")
        return cls(_ffi.VDB_FUSION_WEIGHTED, weights=(a, m, h), name=f"Weighted({float(a)}, {float(m)}, {float(h)})")

    def _weights_ptr(self):
        w = np.array(self.weights, dtype=np.float32)
        return w, _ptr(w)

    def fuse(self, results, device: int = 0) -> List[Tuple[int, float]]:
        """FusionStrategy::fuse (strategy.rs:138-167): `results` = one list of (id, score) per query, best first."""
        ids, sc, cnt = fuse_groups(self, [results], None, device)
        return [(int(ids[0, i]), float(sc[0, i])) for i in range(int(cnt[0]))]


def fuse_groups(fusion: FusionStrategy, groups, top_k: Optional[int] = None, device: int = 0):
    """vdb_hip_fuse_results: `groups` = a sequence of groups, each a sequence of lists of (id, score); every group is fused on its own,
    all in one launch.  top_k None = everything (the largest group's record count).  Returns (ids, scores, counts): numpy arrays
    [n_groups][max(top_k, 1)] padded with id 2^64 - 1 / NaN, and [n_groups]."""
    lists = [list(l) for g in groups for l in g]
    sizes = np.array([len(g) for g in groups], dtype=np.uint32)
    stride = max([len(l) for l in lists], default=0)
    ids = np.zeros((len(lists), max(stride, 1)), dtype=np.uint64)
    sc = np.zeros((len(lists), max(stride, 1)), dtype=np.float32)
    ln = np.array([len(l) for l in lists], dtype=np.uint32)
    for j, l in enumerate(lists):
        if l:
            ids[j, :len(l)] = np.array([r[0] for r in l], dtype=np.uint64)
            sc[j, :len(l)] = np.array([r[1] for r in l], dtype=np.float32)
    if top_k is None:
        top_k = max([sum(len(l) for l in g) for g in groups], default=0)
    return fuse_arrays(fusion, ids, sc, ln, sizes, top_k, device)


def fuse_arrays(fusion: FusionStrategy, ids, scores, list_n, group_sizes, top_k: int, device: int = 0):
    """vdb_hip_fuse_results over numpy arrays: ids / scores [n_lists][list_stride], list_n [n_lists], group_sizes [n_groups]."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    list_n = np.ascontiguousarray(list_n, dtype=np.uint32)
    group_sizes = np.ascontiguousarray(group_sizes, dtype=np.uint32)
    n_lists, stride = (ids.shape if ids.ndim == 2 else (0, 0))
    ng, kk = group_sizes.size, max(top_k, 1)
    out_ids = np.full((ng, kk), _PAD_ID, dtype=np.uint64)      # (top_k = 0: the library writes counts only; the one slot stays padding)
    out_sc = np.full((ng, kk), np.nan, dtype=np.float32)
    out_n = np.zeros(ng, dtype=np.uint32)
    w, wp = fusion._weights_ptr()
    check(lib().vdb_hip_fuse_results(device, fusion.code, fusion.rrf_k, wp, _ptr(ids) if ids.size else None, _ptr(scores) if scores.size else None,
                                     _ptr(list_n) if n_lists else None, n_lists, stride, _ptr(group_sizes) if ng else None, ng, top_k,
                                     _ptr(out_ids), _ptr(out_sc), _ptr(out_n)))
    return out_ids, out_sc, out_n


def _id_lists(lists, nq: Optional[int] = None):
    """a sequence of id sequences -> (ids [n][max(stride, 1)] u64, counts [n] u32, stride)"""
    lists = [np.asarray(l, dtype=np.uint64).reshape(-1) for l in lists]
    if nq is not None and len(lists) != nq:
        raise ValueError(f"Queries count ({nq}) does not match id lists count ({len(lists)})")
    stride = max([l.size for l in lists], default=0)
    ids = np.zeros((len(lists), max(stride, 1)), dtype=np.uint64)
    for j, l in enumerate(lists):
        ids[j, :l.size] = l
    return ids, np.array([l.size for l in lists], dtype=np.uint32), stride


def _hybrid_weights(vector_weight, nq: int):
    """None (0.5 for all), a scalar or a per-query array -> the [nq] f32 array the library takes, or None"""
    if vector_weight is None:
        return None
    w = np.asarray(vector_weight, dtype=np.float32)
    if w.ndim == 0:
        return np.full(nq, w, dtype=np.float32)
    if w.shape != (nq,):
        raise ValueError(f"Queries count ({nq}) does not match vector_weight count ({w.size})")
    return np.ascontiguousarray(w)


def hybrid_fuse_arrays(vec_ids, vec_n, text_ids, text_n, k: int, vector_weights=None, device: int = 0):
    """vdb_hip_hybrid_fuse over numpy arrays: the hybrid_search rule alone (collection/search/text.rs:113-203) for nq list pairs in
    one launch, every id live, no filter.  vec_ids [nq][vec_stride] / text_ids [nq][text_stride] u64, best first; vec_n / text_n [nq];
    vector_weights None (0.5), a scalar or [nq].  Returns (ids, fused scores, counts): [nq][max(k, 1)] padded with id 2^64 - 1 / NaN,
    and [nq]; equal fused scores come back by id DESCENDING."""
    vec_ids = np.ascontiguousarray(vec_ids, dtype=np.uint64)
    text_ids = np.ascontiguousarray(text_ids, dtype=np.uint64)
    vec_n = np.ascontiguousarray(vec_n, dtype=np.uint32)
    text_n = np.ascontiguousarray(text_n, dtype=np.uint32)
    nq, kk = vec_n.size, max(k, 1)
    if text_n.size != nq:
        raise ValueError(f"Queries count ({nq}) does not match id lists count ({text_n.size})")
    vs = vec_ids.shape[1] if vec_ids.ndim == 2 else 0
    ts = text_ids.shape[1] if text_ids.ndim == 2 else 0
    w = _hybrid_weights(vector_weights, nq)
    out_ids = np.full((nq, kk), _PAD_ID, dtype=np.uint64)      # (k = 0: the library writes counts only; the one slot stays padding)
    out_sc = np.full((nq, kk), np.nan, dtype=np.float32)
    out_n = np.zeros(nq, dtype=np.uint32)
    check(lib().vdb_hip_hybrid_fuse(device, _ptr(vec_ids) if vec_ids.size else None, _ptr(vec_n) if nq else None, vs,
                                    _ptr(text_ids) if text_ids.size else None, _ptr(text_n) if nq else None, ts,
                                    _ptr(w) if w is not None and nq else None, nq, k, _ptr(out_ids), _ptr(out_sc), _ptr(out_n)))
    return out_ids, out_sc, out_n


class Filter:
    """An id allow-list of one index (vdb_hip_filter): an immutable snapshot of the rows the given ids had when it was created.
    `matched` = rows in the set.  Close it (or leave its `with` block) before the index is closed."""

    def __init__(self, handle, matched: int):
        self._h = handle
        self.matched = matched

    def close(self) -> None:
        if self._h:
            lib().vdb_hip_filter_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HnswIndex:
    """HNSW index whose vectors, graph and search run on one MI355X."""

    def __init__(self, dimension: int, metric: DistanceMetric, params: Optional[HnswParams] = None,
                 device: int = 0, devices: Optional[Sequence[int]] = None, shard_mode: int = SHARD_REPLICA):
        # HnswIndex::new / with_params — constructors.rs:28-32,117-160.  `devices` (more than one) = one handle over
        # several GPUs: SHARD_RANGE (contiguous row ranges, exact searches merged) or SHARD_REPLICA (query stream split)
        self._h = C.c_void_p()
        self._dimension = int(dimension)
        self._metric = DistanceMetric(metric)
        self.params = params or HnswParams.auto(dimension)
        devs = list(devices) if devices is not None else [int(device)]
        arr = (C.c_int32 * len(devs))(*devs)
        check(lib().vdb_hip_index_create(dimension, int(self._metric), self.params.max_connections,
                                         self.params.ef_construction, self.params.max_elements, arr, len(devs),
                                         int(shard_mode), C.byref(self._h)))
        # HnswParams::storage_mode (params.rs:24-27; with_sq8 / with_binary): SQ8 / Binary collections quantise every stored
        # vector — applied at construction, as the Rust shim does (velesdb-hip/src/lib.rs `with_params`)
        if int(getattr(self.params, "storage_mode", 0)) != 0:
            self.set_storage_mode(self.params.storage_mode)

    def join_group(self, unique_id: bytes, rank: int, world: int) -> None:
        """One process per GPU: this index becomes shard `rank` of `world` (rank order = row order); exact searches
        then return the global top-k on every rank (one RCCL all-gather per batch)."""
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().vdb_hip_index_join_group(self._h, buf, rank, world))

    def shard_info(self) -> dict:
        v = [C.c_int32(0) for _ in range(5)]
        check(lib().vdb_hip_index_shard_info(self._h, *[C.byref(x) for x in v]))
        return {"n_shards": v[0].value, "shard_mode": v[1].value, "rank": v[2].value, "world": v[3].value,
                "transport": {0: "none", 1: "rccl", 2: "d2d-copy"}[v[4].value]}

    @classmethod
    def with_params(cls, dimension, metric, params, device=0):
        return cls(dimension, metric, params, device)

    @classmethod
    def new_turbo(cls, dimension, metric, device=0):  # constructors.rs:86-91
        p = HnswParams.auto(dimension)
        return cls(dimension, metric, HnswParams(p.max_connections, p.ef_construction * 3 // 2, p.max_elements), device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().vdb_hip_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- VectorIndex ------------------------------------------------------------------
    def insert(self, id: int, vector) -> None:
        """VectorIndex::insert (index/mod.rs:46).  Duplicate ids are skipped silently."""
        v = _f32(vector).reshape(-1)
        assert v.size == self._dimension, \
            f"Vector dimension mismatch: expected {self._dimension}, got {v.size}"  # trait_impl.rs:12-18
        check(lib().vdb_hip_index_insert(self._h, int(id), _ptr(v), v.size))

    def search(self, query, k: int) -> List[Tuple[int, float]]:
        """VectorIndex::search (index/mod.rs:58) = search_with_quality(Balanced) (trait_impl.rs:38-42)."""
        return self.search_with_quality(query, k, SearchQuality.Balanced)

    def remove(self, id: int) -> bool:
        r = C.c_int32(0)
        check(lib().vdb_hip_index_remove(self._h, int(id), C.byref(r)))
        return bool(r.value)

    def len(self) -> int:
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_len(self._h, C.byref(n)))
        return int(n.value)

    __len__ = len

    def is_empty(self) -> bool:
        return self.len() == 0

    def dimension(self) -> int:
        return self._dimension

    def metric(self) -> DistanceMetric:
        return self._metric

    # ---- HnswIndex inherent methods ----------------------------------------------------
    def _validate(self, q: np.ndarray, what="Query"):
        assert q.shape[-1] == self._dimension, \
            f"{what} dimension mismatch: expected {self._dimension}, got {q.shape[-1]}"  # search.rs:16-23

    def _search_raw(self, queries: np.ndarray, k: int, ef: int, mode: int):
        assert queries.ndim == 2 and queries.shape[1] == self._dimension and queries.flags.c_contiguous
        nq = queries.shape[0]
        kk = max(k, 1)
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_search_batch(self._h, _ptr(queries), nq, k, ef, mode, _ptr(ids), _ptr(sc),
                                               _ptr(cnt)))
        return ids, sc, cnt

    @staticmethod
    def _tuples(ids, sc, n) -> List[Tuple[int, float]]:
        return [(int(ids[i]), float(sc[i])) for i in range(int(n))]

    def search_with_quality(self, query, k: int, quality: SearchQuality) -> List[Tuple[int, float]]:
        """search.rs:59-94."""
        q = _f32(query).reshape(1, -1)
        self._validate(q)
        if quality.kind == "perfect":  # search.rs:68-70
            ids, sc, cnt = self._search_raw(q, k, 0, MODE_BRUTE)
        else:
            ids, sc, cnt = self._search_raw(q, k, quality.ef_search(k), MODE_AUTO)
        return self._tuples(ids[0], sc[0], cnt[0])

    def search_filtered(self, query, k: int, keep) -> List[Tuple[int, float]]:
        """The index side of Collection::search_with_filter (collection/search/vector.rs:164-235): post-filtering over an
        over-fetched candidate list — candidates_k = max(4 k, k + 10) through VectorIndex::search, the ids `keep(id)`
        rejects dropped, the first k survivors kept, then ordered by the metric's rule (a stable sort, as the reference's
        sort_by over partial_cmp).  Payload storage and the Filter type stay the caller's: `keep` stands for
        `filter.matches(payload(id))`."""
        candidates_k = max(k * 4, k + 10)  # vector.rs:182
        out = [(i, s) for i, s in self.search(query, candidates_k) if keep(i)][:k]
        hib = self._metric in (DistanceMetric.Cosine, DistanceMetric.DotProduct, DistanceMetric.Jaccard)  # higher_is_better
        # vector.rs:219-233: stable sort by score (partial_cmp; incomparable pairs compare Equal and keep their order)
        import functools

        def cmp(a, b):
            x, y = (b[1], a[1]) if hib else (a[1], b[1])
            return -1 if x < y else (1 if x > y else 0)
        return sorted(out, key=functools.cmp_to_key(cmp))

    def search_brute_force(self, query, k: int) -> List[Tuple[int, float]]:
        """search.rs:176-219: exact scan, raw scores, metric.sort_results order."""
        q = _f32(query).reshape(1, -1)
        self._validate(q)
        ids, sc, cnt = self._search_raw(q, k, 0, MODE_BRUTE)
        return self._tuples(ids[0], sc[0], cnt[0])

    search_brute_force_buffered = search_brute_force  # search.rs:367-370
    brute_force_search_parallel = search_brute_force  # batch.rs:223-244 (same result contract)

    def search_brute_force_gpu(self, query, k: int) -> Optional[List[Tuple[int, float]]]:
        """search.rs:229-279: None when no GPU is available."""
        if device_count() == 0:
            return None
        return self.search_brute_force(query, k)

    def search_batch_parallel(self, queries, k: int, quality: SearchQuality) -> List[List[Tuple[int, float]]]:
        """batch.rs:159-197: always the graph, one launch for the whole batch."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        if qs.shape[0] == 0:
            return []
        for i in range(qs.shape[0]):
            assert qs.shape[1] == self._dimension, \
                f"Query {i} dimension mismatch: expected {self._dimension}, got {qs.shape[1]}"
        ids, sc, cnt = self._search_raw(qs, k, quality.ef_search(k), MODE_HNSW)
        return [self._tuples(ids[i], sc[i], cnt[i]) for i in range(qs.shape[0])]

    def search_with_rerank(self, query, k: int, rerank_k: int) -> List[Tuple[int, float]]:
        """search.rs:118-160: HNSW candidates (Accurate) re-scored exactly; raw scores, metric order."""
        return self.search_with_rerank_quality(query, k, rerank_k, SearchQuality.Accurate)

    def search_with_rerank_quality(self, query, k: int, rerank_k: int, initial_quality: SearchQuality):
        """search.rs:297-350 (Perfect is replaced by Accurate to avoid recursion, :305-310)."""
        q = _f32(query).reshape(1, -1)
        self._validate(q)
        if initial_quality.kind == "perfect":
            initial_quality = SearchQuality.Accurate
        ef = initial_quality.ef_search(rerank_k)
        kk = max(k, 1)
        ids = np.empty((1, kk), dtype=np.uint64)
        sc = np.empty((1, kk), dtype=np.float32)
        cnt = np.zeros(1, dtype=np.uint32)
        check(lib().vdb_hip_index_search_rerank(self._h, _ptr(q), 1, k, rerank_k, ef, _ptr(ids), _ptr(sc), _ptr(cnt)))
        return self._tuples(ids[0], sc[0], cnt[0])

    def search_multi_entry(self, queries, k: int, ef_search: int, num_probes: int):
        """NativeHnsw::search_multi_entry (native/graph.rs:288-348) for a batch: the descent's result plus up to
        min(num_probes, 4) - 1 nodes drawn from the graph's own xorshift stream as entry points of one layer-0 search.  Like the
        reference it advances that stream (query i takes the draws nq sequential calls would give it).  numpy outputs."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        nq, kk = qs.shape[0], max(k, 1)
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_search_multi_entry(self._h, _ptr(qs), nq, k, ef_search, num_probes, _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def train_quantizer(self, sample_rows: int = 0) -> None:
        """ScalarQuantizer::train on the first sample_rows rows (0 = min(1000, rows)) + u8 codes of every row."""
        check(lib().vdb_hip_index_train_quantizer(self._h, sample_rows))

    def is_quantizer_trained(self) -> bool:
        """DualPrecisionHnsw::is_quantizer_trained (native/dual_precision.rs:117-120), read from the handle."""
        t = C.c_int32(0)
        check(lib().vdb_hip_index_quantizer_trained(self._h, C.byref(t)))
        return bool(t.value)

    def search_with_config(self, query, k: int, ef_search: int, config: Optional[DualPrecisionConfig] = None) -> List[Tuple[int, float]]:
        """DualPrecisionHnsw::search_with_config (native/dual_precision.rs:259-278): the int8 traversal only with a trained
        quantiser, `use_int8_traversal` and at least `min_index_size` (default 10 000) vectors; otherwise the plain f32 graph
        search.  The config travels with the call (vdb_hip_index_search_with_config): the rule is applied inside the library from
        the handle's own state, `oversampling_ratio` (k * ratio of the int8 walk's best are re-scored exactly) is this call's own —
        no handle option is touched, concurrent callers may use different ratios."""
        cfg = config or DualPrecisionConfig()
        q = _f32(query).reshape(1, -1)
        self._validate(q)
        kk = max(k, 1)
        ids = np.empty((1, kk), dtype=np.uint64)
        sc = np.empty((1, kk), dtype=np.float32)
        cnt = np.zeros(1, dtype=np.uint32)
        check(lib().vdb_hip_index_search_with_config(self._h, _ptr(q), 1, k, ef_search, max(int(cfg.oversampling_ratio), 1),
                                                     1 if cfg.use_int8_traversal else 0, int(cfg.min_index_size), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return self._tuples(ids[0], sc[0], cnt[0])

    def search_batch_int8(self, queries, k: int, ef_search: int):
        """DualPrecisionHnsw::search_with_config(use_int8_traversal): int8 graph walk + exact f32 re-rank."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        ids, sc, cnt = self._search_raw(qs, k, ef_search, MODE_HNSW_INT8)
        return [self._tuples(ids[i], sc[i], cnt[i]) for i in range(qs.shape[0])]

    def enable_bf16(self) -> None:
        """Keeps a bf16 (round-to-nearest-even) copy of the rows for search_batch_brute_force_bf16."""
        check(lib().vdb_hip_index_enable_bf16(self._h))

    def search_batch_brute_force_bf16(self, queries, k: int):
        """Exact scan with bf16 rows and queries, f32 accumulation on the matrix cores
        (half_precision.rs:199-255 semantics); numpy outputs like search_batch_brute_force."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        return self._search_raw(qs, k, 0, MODE_BRUTE_BF16)

    def enable_half_precision(self, precision) -> None:
        """Keeps a half-precision copy of the rows (VectorData::from_f32_slice(.., precision), half_precision.rs:94-101) for
        search_batch_brute_force_half: Cosine, DotProduct and Euclidean indexes; F16 and BF16 may both be enabled."""
        check(lib().vdb_hip_index_enable_half_precision(self._h, int(precision)))

    def set_graph_precision(self, precision) -> None:
        """The row format every distance of graph construction is taken over from now on (insert, insert_batch*, build_graph,
        the rebuild inside vacuum): F32 (default) or — after enable_half_precision(precision) — F16 / BF16, the image the half
        walks read.  The graph is then the reference's over the dequantised rows, link for link.  Allowed on a graph that has
        nodes (the cached neighbour distances are recomputed in the new precision before the next insert).  Not persisted: a
        loaded index starts at F32."""
        check(lib().vdb_hip_index_set_graph_precision(self._h, int(precision)))

    def graph_precision(self) -> VectorPrecision:
        p = C.c_int32(0)
        check(lib().vdb_hip_index_graph_precision(self._h, C.byref(p)))
        return VectorPrecision(p.value)

    def search_batch_brute_force_half(self, queries, k: int, precision):
        """Exact scan over the half-precision copy of the rows with queries rounded the same way: half_precision::dot_product /
        cosine_similarity / euclidean_distance on VectorData::{F16, BF16} (half_precision.rs:199-287); numpy outputs like
        search_batch_brute_force.  Needs enable_half_precision(precision)."""
        precision = VectorPrecision(int(precision))
        if precision == VectorPrecision.F32:
            raise ValueError("half-precision search: F16 or BF16")
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        return self._search_raw(qs, k, 0, MODE_BRUTE_F16 if precision == VectorPrecision.F16 else MODE_BRUTE_BF16)

    def search_batch_half_graph(self, queries, k: int, ef_search: int, precision):
        """Graph search over the half-precision copy of the rows: NativeHnsw::search on the index's graph exactly as
        search_batch_parallel (ef_search = 0 -> Balanced, max(ef_search, k), scores through transform_score), every distance taken
        between the query rounded to `precision` and the row's half image (half_precision.rs:199-287) — half the bytes of the f32
        walk per visited node.  Needs enable_half_precision(precision) and a graph.  Returns what search_batch_int8 returns."""
        precision = VectorPrecision(int(precision))
        if precision == VectorPrecision.F32:
            raise ValueError("half-precision graph search: F16 or BF16")
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        ids, sc, cnt = self._search_raw(qs, k, ef_search, MODE_HNSW_F16 if precision == VectorPrecision.F16 else MODE_HNSW_BF16)
        return [self._tuples(ids[i], sc[i], cnt[i]) for i in range(qs.shape[0])]

    # ---- storage modes (core/quantization.rs) -----------------------------------------------
    def set_storage_mode(self, mode) -> None:
        """StorageMode of the owning collection (quantization.rs:17-29): the index keeps the SQ8 / binary code of every
        vector, as collection/core/crud.rs:66-82 does on upsert."""
        check(lib().vdb_hip_index_set_storage_mode(self._h, int(mode)))

    def get_quantized_bytes(self, id: int) -> bytes:
        """QuantizedVector::to_bytes / BinaryQuantizedVector::to_bytes of the stored code of `id`."""
        n = C.c_size_t(0)
        buf = (C.c_uint8 * (self._dimension + 16))()
        check(lib().vdb_hip_index_get_quantized(self._h, id, buf, len(buf), C.byref(n)))
        return bytes(buf[:n.value])

    def search_batch_sq8(self, queries, k: int):
        """Exact scan over the SQ8 codes with the reference's asymmetric `_simd` distances (quantization.rs:410-554):
        cosine / dot similarity (best = largest) or SQUARED Euclidean distance (best = smallest)."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        return self._search_raw(qs, k, 0, MODE_BRUTE_SQ8)

    def search_batch_binary(self, queries, k: int):
        """Exact scan by Hamming distance between sign-bit codes (BinaryQuantizedVector::hamming_distance)."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        return self._search_raw(qs, k, 0, MODE_BRUTE_BINARY)

    def search_batch_brute_force(self, queries, k: int):
        """Batched exact search (one corpus pass per tile of queries); numpy outputs."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        return self._search_raw(qs, k, 0, MODE_BRUTE)

    def create_filter(self, ids, negate: bool = False) -> Filter:
        """The ids a caller's predicate matched, as a device-side allow-list (negate: every row present now except them).  Unknown
        and duplicate ids are ignored; rows inserted later are not in it, rows removed later drop out of its results; vacuum() and
        load make it stale (searches then raise with VDB_ERR_STATE)."""
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        h, m = C.c_void_p(), C.c_uint64(0)
        check(lib().vdb_hip_index_filter_create(self._h, _ptr(a) if a.size else None, a.size, 1 if negate else 0, C.byref(m), C.byref(h)))
        return Filter(h, int(m.value))

    def search_batch_brute_force_filtered(self, queries, k: int, flt: Filter, mode: int = MODE_BRUTE):
        """search_batch_brute_force among the filter's rows only: the exact top-k of the allowed live rows — ids, ranks and score
        bits of an index that holds just those rows (what the reference's `_with_filter` searches approximate by over-fetching,
        collection/search/vector.rs:164-239).  numpy outputs."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        nq, kk = qs.shape[0], max(k, 1)
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_search_batch_filtered(self._h, flt._h if flt is not None else None, _ptr(qs), nq, k, mode, _ptr(ids),
                                                        _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def _search_filtered_mode(self, queries, k: int, flt: Filter, mode: int):
        """vdb_hip_index_search_batch_filtered_mode: the exact scan of `mode` (SQ8 codes, sign bits, a half image) among the filter's
        rows only — what the plain call in that mode returns on an index that holds just the allowed live rows.  numpy outputs."""
        if not isinstance(flt, Filter):
            raise TypeError("filtered search: flt must be a Filter (create_filter)")
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        if qs.ndim != 2:
            raise ValueError(f"filtered search: queries must be one vector or a (nq, dim) array, got {qs.ndim} dimensions")
        if int(k) < 0:
            raise ValueError("filtered search: k must not be negative")
        self._validate(qs)
        nq, kk = qs.shape[0], max(int(k), 1)
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_search_batch_filtered_mode(self._h, flt._h, mode, _ptr(qs), nq, int(k), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def search_batch_filtered_sq8(self, queries, k: int, flt: Filter):
        """search_batch_sq8 among the filter's rows only (storage mode SQ8): ids, ranks and score bits of an SQ8 index that holds
        just the allowed live rows.  OPT_FILTER_ROUTE picks the listed sweep over the codes or mask substitution (same bits)."""
        return self._search_filtered_mode(queries, k, flt, MODE_BRUTE_SQ8)

    def search_batch_filtered_binary(self, queries, k: int, flt: Filter):
        """search_batch_binary among the filter's rows only (storage mode Binary): Hamming distances between sign-bit codes, ties by
        row, of an index that holds just the allowed live rows."""
        return self._search_filtered_mode(queries, k, flt, MODE_BRUTE_BINARY)

    def search_batch_filtered_half(self, queries, k: int, flt: Filter, precision):
        """search_batch_brute_force_half among the filter's rows only (enable_half_precision(precision) first).  Euclidean: bit
        for bit on both routes; Cosine / DotProduct: mask substitution over the matrix-core tiers, within that mode's tolerance."""
        precision = VectorPrecision(int(precision))
        if precision == VectorPrecision.F32:
            raise ValueError("half-precision search: F16 or BF16")
        return self._search_filtered_mode(queries, k, flt, MODE_BRUTE_F16 if precision == VectorPrecision.F16 else MODE_BRUTE_BF16)

    def search_batch_filtered_graph(self, queries, k: int, flt: Filter, ef: int = 0, route: int = ROUTE_AUTO, max_list: int = 0,
                                    mode: int = MODE_HNSW):
        """Graph search with the filter consulted inside the walk (vdb_hip_index_search_graph_filtered): layer 0 keeps allowed live
        rows only in its result set, every node still navigates.  route: ROUTE_AUTO (walk, or the exact pass where the walk's
        candidate list could not hold the query), ROUTE_WALK, ROUTE_EXACT; max_list lowers the largest candidate list (0 = what
        the LDS holds).  Returns ((ids, scores, counts), routes): numpy outputs, routes[q] = 1 walk / 2 exact pass / 0 nothing ran."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        nq, kk = qs.shape[0], max(k, 1)
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        routes = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_search_graph_filtered(self._h, flt._h if flt is not None else None, _ptr(qs), nq, k, ef, mode, route,
                                                        max_list, _ptr(ids), _ptr(sc), _ptr(cnt), _ptr(routes)))
        return (ids, sc, cnt), routes

    def _filters_call_buffers(self, queries, k: int, filters):
        """what the calls with one optional filter per query share: the validated queries, the table of distinct filters (by object
        identity; index len(table) = no filter), every query's index into it and the output arrays"""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        filters = list(filters)
        nq, kk = qs.shape[0], max(k, 1)
        if len(filters) != nq:
            raise ValueError(f"Queries count ({nq}) does not match filters count ({len(filters)})")
        table, slot_of = [], {}  # distinct filters by object identity; index len(table) = no filter
        for f in filters:
            if f is not None and id(f) not in slot_of:
                slot_of[id(f)] = len(table)
                table.append(f)
        fq = np.array([len(table) if f is None else slot_of[id(f)] for f in filters], dtype=np.uint32)
        handles = (C.c_void_p * max(len(table), 1))(*[f._h for f in table])
        ids = np.empty((nq, kk), dtype=np.uint64)
        sc = np.empty((nq, kk), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        routes = np.zeros(nq, dtype=np.uint32)
        return qs, nq, table, handles, fq, ids, sc, cnt, routes

    def search_batch_with_filters(self, queries, k: int, filters, ef: int = 0, route: int = ROUTE_AUTO, max_list: int = 0):
        """search_batch_filtered_graph with one optional filter PER QUERY in one call (vdb_hip_index_search_graph_filters; the
        collection layer's search_batch_with_filters).  filters: a sequence of Optional[Filter], one per query; None = no filter
        (every row present now).  Query i gets bit for bit what search_batch_filtered_graph returns for it alone with its filter,
        whatever its companions are.  Returns ((ids, scores, counts), routes)."""
        qs, nq, table, handles, fq, ids, sc, cnt, routes = self._filters_call_buffers(queries, k, filters)
        check(lib().vdb_hip_index_search_graph_filters(self._h, handles if table else None, len(table), _ptr(fq), _ptr(qs), nq, k, ef,
                                                       MODE_HNSW, route, max_list, _ptr(ids), _ptr(sc), _ptr(cnt), _ptr(routes)))
        return (ids, sc, cnt), routes

    def search_batch_brute_force_with_filters(self, queries, k: int, filters):
        """search_batch_brute_force_filtered with one optional filter PER QUERY in one call (vdb_hip_index_search_batch_filters; the
        collection layer's search_batch_with_filters on the exact sweep).  filters: a sequence of Optional[Filter], one per query;
        None = no filter.  Query i gets bit for bit what search_batch_brute_force_filtered returns for it alone with its filter
        (without one: what search_batch_brute_force returns for it alone), whatever its companions are.  numpy outputs."""
        qs, nq, table, handles, fq, ids, sc, cnt, _ = self._filters_call_buffers(queries, k, filters)
        check(lib().vdb_hip_index_search_batch_filters(self._h, handles if table else None, len(table), _ptr(fq), _ptr(qs), nq, k,
                                                       MODE_BRUTE, _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def search_batch_with_filters_mode(self, queries, k: int, filters, mode: int):
        """search_batch_brute_force_with_filters over the SQ8 codes, the sign bits or a half image of the rows
        (vdb_hip_index_search_batch_filters_mode): mode is MODE_BRUTE_SQ8, MODE_BRUTE_BINARY, MODE_BRUTE_F16 or MODE_BRUTE_BF16.
        filters: a sequence of Optional[Filter], one per query; None = no filter.  SQ8, Binary and Euclidean over a half image: query
        i gets bit for bit what the one-filter call of that mode returns for it alone (without a filter: the plain call of that
        mode).  Cosine / DotProduct over a half image: bit for bit what the one-filter call returns for the query's group — the
        queries that name the same filter, in call order.  numpy outputs."""
        if int(k) < 0:
            raise ValueError("filtered search: k must not be negative")
        qs, nq, table, handles, fq, ids, sc, cnt, _ = self._filters_call_buffers(queries, int(k), filters)
        check(lib().vdb_hip_index_search_batch_filters_mode(self._h, handles if table else None, len(table), _ptr(fq), int(mode), _ptr(qs),
                                                            nq, int(k), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def search_batch_with_filters_sq8(self, queries, k: int, filters):
        """search_batch_filtered_sq8 with one optional filter PER QUERY in one call (storage mode SQ8)."""
        return self.search_batch_with_filters_mode(queries, k, filters, MODE_BRUTE_SQ8)

    def search_batch_with_filters_binary(self, queries, k: int, filters):
        """search_batch_filtered_binary with one optional filter PER QUERY in one call (storage mode Binary)."""
        return self.search_batch_with_filters_mode(queries, k, filters, MODE_BRUTE_BINARY)

    def search_batch_brute_force_with_filters_half(self, queries, k: int, filters, precision):
        """search_batch_filtered_half with one optional filter PER QUERY in one call (enable_half_precision(precision) first).
        (search_batch_with_filters_half is the GRAPH walk over the half image; this is the exact sweep over it.)"""
        precision = VectorPrecision(int(precision))
        if precision == VectorPrecision.F32:
            raise ValueError("half-precision search: F16 or BF16")
        return self.search_batch_with_filters_mode(queries, k, filters, MODE_BRUTE_F16 if precision == VectorPrecision.F16 else MODE_BRUTE_BF16)

    def last_filters_exact_plan(self):
        """the plan of this thread's last search_batch_brute_force_with_filters / search_batch_with_filters_mode call: (filter groups,
        groups on the listed route, groups on mask substitution, unfiltered queries, grouped sweep launches, merge launches behind them)"""
        out = (C.c_uint32 * 6)()
        check(lib().vdb_hip_index_last_filters_exact_plan(self._h, out))
        return tuple(int(v) for v in out)

    def search_batch_with_filters_half(self, queries, k: int, filters, mode: int, ef: int = 0, route: int = ROUTE_AUTO,
                                       max_list: int = 0):
        """search_batch_with_filters over the half-precision image of the rows (vdb_hip_index_search_graph_filters_half): mode is
        MODE_HNSW_F16 or MODE_HNSW_BF16 (enable_half_precision first).  Same filters, routes, lists and outputs; every distance of
        the walk and of the exact pass is the one search_batch(mode) takes — the query rounded to the precision against the row's
        image.  With no query filtered the call is search_batch(mode).  Returns ((ids, scores, counts), routes)."""
        qs, nq, table, handles, fq, ids, sc, cnt, routes = self._filters_call_buffers(queries, k, filters)
        check(lib().vdb_hip_index_search_graph_filters_half(self._h, mode, handles if table else None, len(table), _ptr(fq), _ptr(qs), nq,
                                                            k, ef, route, max_list, _ptr(ids), _ptr(sc), _ptr(cnt), _ptr(routes)))
        return (ids, sc, cnt), routes

    def search_batch_with_filters_int8(self, queries, k: int, filters, ef: int = 0, oversampling: int = 0, route: int = ROUTE_AUTO,
                                       max_list: int = 0):
        """search_batch_with_filters over the u8 codes of the trained quantiser (vdb_hip_index_search_graph_filters_int8;
        train_quantizer first): the int8 walk of search_batch(MODE_HNSW_INT8) with the filter consulted inside it at
        ef = max(ef, k * oversampling), the k * oversampling best allowed candidates re-scored in f32 and cut to k; the exact pass is
        the f32 one, so a row has the same score on either route.  oversampling 0 = the handle's option.  With no query filtered
        the call is search_batch(MODE_HNSW_INT8) at the same ef and ratio.  Returns ((ids, scores, counts), routes)."""
        qs, nq, table, handles, fq, ids, sc, cnt, routes = self._filters_call_buffers(queries, k, filters)
        check(lib().vdb_hip_index_search_graph_filters_int8(self._h, handles if table else None, len(table), _ptr(fq), _ptr(qs), nq, k, ef,
                                                            oversampling, route, max_list, _ptr(ids), _ptr(sc), _ptr(cnt), _ptr(routes)))
        return (ids, sc, cnt), routes

    def search_batch_filtered_graph_int8(self, queries, k: int, flt: Filter, ef: int = 0, oversampling: int = 0, route: int = ROUTE_AUTO,
                                         max_list: int = 0):
        """search_batch_filtered_graph over the u8 codes: search_batch_with_filters_int8 with `flt` for every query (a table of
        one)."""
        qs = _f32(queries)
        nq = 1 if qs.ndim == 1 else qs.shape[0]
        return self.search_batch_with_filters_int8(qs, k, [flt] * nq, ef=ef, oversampling=oversampling, route=route, max_list=max_list)

    def search_batch_with_filters_half_rescore(self, queries, k: int, filters, mode: int, ef: int = 0, oversampling: int = 0,
                                               route: int = ROUTE_AUTO, max_list: int = 0):
        """search_batch_with_filters_half with exact f32 answers (vdb_hip_index_search_graph_filters_half_rescore; mode is
        MODE_HNSW_F16 or MODE_HNSW_BF16, enable_half_precision first): the half walk with the filter consulted inside it at
        ef = max(ef, k * oversampling), the k * oversampling best allowed candidates re-scored with the exact f32 distance between
        the unrounded query and the f32 row, stable-sorted and cut to k; the exact pass is the f32 one, so a row has the same score
        on either route.  oversampling 0 = 4; more than 64 is refused.  Returns ((ids, scores, counts), routes)."""
        qs, nq, table, handles, fq, ids, sc, cnt, routes = self._filters_call_buffers(queries, k, filters)
        check(lib().vdb_hip_index_search_graph_filters_half_rescore(self._h, mode, handles if table else None, len(table), _ptr(fq),
                                                                    _ptr(qs), nq, k, ef, oversampling, route, max_list, _ptr(ids),
                                                                    _ptr(sc), _ptr(cnt), _ptr(routes)))
        return (ids, sc, cnt), routes

    def search_batch_filtered_graph_half_rescore(self, queries, k: int, flt: Filter, mode: int, ef: int = 0, oversampling: int = 0,
                                                 route: int = ROUTE_AUTO, max_list: int = 0):
        """search_batch_filtered_graph over the half-precision image with exact f32 answers:
        search_batch_with_filters_half_rescore with `flt` for every query (a table of one)."""
        qs = _f32(queries)
        nq = 1 if qs.ndim == 1 else qs.shape[0]
        return self.search_batch_with_filters_half_rescore(qs, k, [flt] * nq, mode, ef=ef, oversampling=oversampling, route=route,
                                                           max_list=max_list)

    def search_batch_half_rescore(self, queries, k: int, mode: int, ef: int = 0, oversampling: int = 0):
        """the plain dual-precision half search: search_batch_with_filters_half_rescore with no filter for any query (n_filters = 0).
        Returns (ids, scores, counts)."""
        qs = _f32(queries)
        nq = 1 if qs.ndim == 1 else qs.shape[0]
        return self.search_batch_with_filters_half_rescore(qs, k, [None] * nq, mode, ef=ef, oversampling=oversampling)[0]

    def search_batch_filtered_graph_half(self, queries, k: int, flt: Filter, mode: int, ef: int = 0, route: int = ROUTE_AUTO,
                                         max_list: int = 0):
        """search_batch_filtered_graph over the half-precision image: search_batch_with_filters_half with `flt` for every query (a
        table of one)."""
        qs = _f32(queries)
        nq = 1 if qs.ndim == 1 else qs.shape[0]
        return self.search_batch_with_filters_half(qs, k, [flt] * nq, mode, ef=ef, route=route, max_list=max_list)

    def multi_query_search_batch(self, groups, top_k: int, fusion: FusionStrategy, flt: Optional[Filter] = None):
        """Collection::multi_query_search_ids (collection/search/batch.rs:352-402) for MANY user queries in one call
        (vdb_hip_index_multi_query_search): `groups` = a sequence of groups of 1..10 vectors (the reformulations of one user query).
        Every vector is searched at the over-fetched k (SearchQuality::Balanced; with `flt` by the filtered graph search), every group's
        lists are fused by `fusion` on the device, the first top_k fused records per group come back.  Returns (ids, scores, counts):
        numpy arrays [n_groups][max(top_k, 1)] padded with id 2^64 - 1 / NaN, and [n_groups]."""
        mats = []
        for g in groups:
            vs = [_f32(v).reshape(-1) for v in g]
            if not vs:
                raise ValueError("multi_query_search requires at least one vector")
            if len(vs) > MAX_FUSED_VECTORS:
                raise ValueError(f"multi_query_search supports at most {MAX_FUSED_VECTORS} vectors, got {len(vs)}")
            for v in vs:
                if v.shape[0] != self._dimension:
                    raise ValueError(f"Vector dimension mismatch: expected {self._dimension}, got {v.shape[0]}")
            mats.append(np.stack(vs))
        sizes = np.array([m.shape[0] for m in mats], dtype=np.uint32)
        qs = np.ascontiguousarray(np.concatenate(mats)) if mats else np.zeros((0, self._dimension), np.float32)
        ng, kk = len(mats), max(top_k, 1)
        ids = np.full((ng, kk), _PAD_ID, dtype=np.uint64)          # (top_k = 0: the library writes counts only)
        sc = np.full((ng, kk), np.nan, dtype=np.float32)
        cnt = np.zeros(ng, dtype=np.uint32)
        w, wp = fusion._weights_ptr()
        check(lib().vdb_hip_index_multi_query_search(self._h, flt._h if flt is not None else None, _ptr(qs) if ng else None,
                                                     _ptr(sizes) if ng else None, ng, top_k, fusion.code, fusion.rrf_k, wp, _ptr(ids),
                                                     _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def multi_query_search_ids(self, vectors, top_k: int, fusion: FusionStrategy, flt: Optional[Filter] = None) -> List[Tuple[int, float]]:
        """Collection::multi_query_search_ids for one user query: `vectors` = its 1..10 reformulations.  (id, fused score), best first."""
        ids, sc, cnt = self.multi_query_search_batch([list(vectors)], top_k, fusion, flt)
        return self._tuples(ids[0], sc[0], cnt[0])

    def hybrid_search_batch(self, queries, text_hits, k: int, vector_weight=None, flt: Optional[Filter] = None):
        """Collection::hybrid_search / hybrid_search_with_filter (collection/search/text.rs:113-299) for MANY user queries in one call
        (vdb_hip_index_hybrid_search).  `text_hits` = one id sequence per query: what the caller's BM25 index returned for the
        query's text at 2k (with `flt`: max(4k, k + 10)), best first.  Every query is walked at that k (SearchQuality::Balanced; with
        `flt` by the filtered graph search) and its list fused with its text hits on the device: w = clamp(vector_weight, 0, 1),
        score = sum w / (rank + 60) over the vector list + sum (1 - w) / (rank + 60) over the text hits, the first k by (score
        descending, id descending).  Without `flt`, text ids the index does not hold take their place in the cut and are then
        dropped; with it, text hits outside (filter AND live) are dropped before ranks are assigned.  vector_weight: None (0.5), a
        scalar or one per query; NaN is refused.  Returns (ids, fused scores, counts): [nq][max(k, 1)] padded with id 2^64 - 1 /
        NaN, and [nq]."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        nq, kk = qs.shape[0], max(k, 1)
        tids, tn, ts = _id_lists(text_hits, nq)
        w = _hybrid_weights(vector_weight, nq)
        ids = np.full((nq, kk), _PAD_ID, dtype=np.uint64)          # (k = 0: the library writes counts only)
        sc = np.full((nq, kk), np.nan, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_hybrid_search(self._h, flt._h if flt is not None else None, _ptr(qs) if nq else None, nq, k,
                                                _ptr(tids) if ts else None, _ptr(tn) if nq else None, ts,
                                                _ptr(w) if w is not None and nq else None, _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def hybrid_search(self, query, text_hits, k: int, vector_weight=None) -> List[Tuple[int, float]]:
        """Collection::hybrid_search (text.rs:113-203) for one query: `text_hits` = the ids text_index.search(text, 2k) returned.
        (id, fused score), best first."""
        ids, sc, cnt = self.hybrid_search_batch(_f32(query).reshape(1, -1), [text_hits], k, vector_weight)
        return self._tuples(ids[0], sc[0], cnt[0])

    def hybrid_search_with_filter(self, query, text_hits, k: int, vector_weight, flt: Filter) -> List[Tuple[int, float]]:
        """Collection::hybrid_search_with_filter (text.rs:221-299) for one query, `flt` consulted inside the walk and in front of
        the text ranks: `text_hits` = the ids text_index.search(text, max(4k, k + 10)) returned."""
        ids, sc, cnt = self.hybrid_search_batch(_f32(query).reshape(1, -1), [text_hits], k, vector_weight, flt)
        return self._tuples(ids[0], sc[0], cnt[0])

    @staticmethod
    def _filter_table(filters, n: int, what: str):
        """the table of distinct filters (by object identity) of a call with one optional filter per unit, and every unit's index
        into it (len(table) = no filter)"""
        filters = list(filters)
        if len(filters) != n:
            raise ValueError(f"{what} count ({n}) does not match filters count ({len(filters)})")
        table, slot_of = [], {}
        for f in filters:
            if f is not None and id(f) not in slot_of:
                slot_of[id(f)] = len(table)
                table.append(f)
        of = np.array([len(table) if f is None else slot_of[id(f)] for f in filters], dtype=np.uint32)
        handles = (C.c_void_p * max(len(table), 1))(*[f._h for f in table])
        return table, handles, of

    def hybrid_search_batch_filters(self, queries, text_hits, k: int, vector_weight=None, filters=None, rows: int = WALK_ROWS_F32,
                                    oversampling: int = 0):
        """hybrid_search_batch with one optional filter PER QUERY over any form of the walk (vdb_hip_index_hybrid_search_filters).
        filters: a sequence of Optional[Filter], one per query (None: no query is filtered).  rows: WALK_ROWS_F32, _F16 / _BF16
        (enable_half_precision first), _INT8 (train_quantizer first) or _F16_RESCORE / _BF16_RESCORE; oversampling is read for the
        last three (0 = the handle's option for _INT8, 4 for the re-score forms).  An unfiltered query is walked at 2k by the plain
        call of that rows form, a filtered one at max(4k, k + 10) by the call with one filter per query, and its text hits outside
        ITS filter are dropped before ranks exist; `text_hits[i]` is what the text index returned at that length.  Query i gets bit
        for bit what it gets alone.  Returns (ids, fused scores, counts) as hybrid_search_batch."""
        qs = _f32(queries)
        if qs.ndim == 1:
            qs = qs.reshape(1, -1)
        self._validate(qs)
        nq, kk = qs.shape[0], max(k, 1)
        table, handles, fq = self._filter_table([None] * nq if filters is None else filters, nq, "Queries")
        tids, tn, ts = _id_lists(text_hits, nq)
        w = _hybrid_weights(vector_weight, nq)
        ids = np.full((nq, kk), _PAD_ID, dtype=np.uint64)          # (k = 0: the library writes counts only)
        sc = np.full((nq, kk), np.nan, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        check(lib().vdb_hip_index_hybrid_search_filters(self._h, int(rows), int(oversampling), handles if table else None, len(table),
                                                        _ptr(fq) if nq else None, _ptr(qs) if nq else None, nq, k,
                                                        _ptr(tids) if ts else None, _ptr(tn) if nq else None, ts,
                                                        _ptr(w) if w is not None and nq else None, _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def multi_query_search_batch_filters(self, groups, top_k: int, fusion: FusionStrategy, filters=None, rows: int = WALK_ROWS_F32,
                                         oversampling: int = 0):
        """multi_query_search_batch with one optional filter PER GROUP over any form of the walk
        (vdb_hip_index_multi_query_search_filters).  filters: a sequence of Optional[Filter], one per group; rows / oversampling as
        in hybrid_search_batch_filters.  Every vector is searched at the over-fetched k — an unfiltered group's by the plain call of
        the rows form, a filtered group's by the call with one filter per query, all of them on the group's filter.  Group g gets bit
        for bit what it gets alone.  Returns (ids, scores, counts) as multi_query_search_batch."""
        mats = []
        for g in groups:
            vs = [_f32(v).reshape(-1) for v in g]
            if not vs:
                raise ValueError("multi_query_search requires at least one vector")
            if len(vs) > MAX_FUSED_VECTORS:
                raise ValueError(f"multi_query_search supports at most {MAX_FUSED_VECTORS} vectors, got {len(vs)}")
            for v in vs:
                if v.shape[0] != self._dimension:
                    raise ValueError(f"Vector dimension mismatch: expected {self._dimension}, got {v.shape[0]}")
            mats.append(np.stack(vs))
        sizes = np.array([m.shape[0] for m in mats], dtype=np.uint32)
        qs = np.ascontiguousarray(np.concatenate(mats)) if mats else np.zeros((0, self._dimension), np.float32)
        ng, kk = len(mats), max(top_k, 1)
        table, handles, fg = self._filter_table([None] * ng if filters is None else filters, ng, "Groups")
        ids = np.full((ng, kk), _PAD_ID, dtype=np.uint64)          # (top_k = 0: the library writes counts only)
        sc = np.full((ng, kk), np.nan, dtype=np.float32)
        cnt = np.zeros(ng, dtype=np.uint32)
        w, wp = fusion._weights_ptr()
        check(lib().vdb_hip_index_multi_query_search_filters(self._h, int(rows), int(oversampling), handles if table else None, len(table),
                                                             _ptr(fg) if ng else None, _ptr(qs) if ng else None,
                                                             _ptr(sizes) if ng else None, ng, top_k, fusion.code, fusion.rrf_k, wp,
                                                             _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def search_brute_force_filtered(self, query, k: int, flt: Filter) -> List[Tuple[int, float]]:
        """search_brute_force among the filter's rows only (one query)."""
        ids, sc, cnt = self.search_batch_brute_force_filtered(_f32(query).reshape(1, -1), k, flt)
        return self._tuples(ids[0], sc[0], cnt[0])

    def insert_batch_sequential(self, vectors: Iterable[Tuple[int, Sequence[float]]]) -> int:
        """batch.rs:128-149."""
        items = list(vectors)
        if not items:
            return 0
        ids = np.ascontiguousarray([i for i, _ in items], dtype=np.uint64)
        for _, v in items:
            assert len(v) == self._dimension, \
                f"Vector dimension mismatch: expected {self._dimension}, got {len(v)}"
        vecs = _f32([v for _, v in items])
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_insert_batch(self._h, _ptr(ids), _ptr(vecs), len(items), C.byref(n)))
        return int(n.value)

    def insert_batch_parallel(self, vectors: Iterable[Tuple[int, Sequence[float]]], max_batch: int = 0) -> int:
        """batch.rs:83-108.  Batch-synchronous and deterministic here (rayon, non-deterministic, there)."""
        items = list(vectors)
        if not items:
            return 0
        ids = np.ascontiguousarray([i for i, _ in items], dtype=np.uint64)
        for _, v in items:
            assert len(v) == self._dimension, \
                f"Vector dimension mismatch: expected {self._dimension}, got {len(v)}"
        vecs = _f32([v for _, v in items])
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_insert_batch_parallel(self._h, _ptr(ids), _ptr(vecs), len(items), max_batch,
                                                        C.byref(n)))
        return int(n.value)

    def build_graph(self, max_batch: int = 0) -> None:
        """Links every uploaded row that is not in the graph yet (batched GPU construction)."""
        check(lib().vdb_hip_index_build_graph(self._h, max_batch))

    def upload(self, ids, vectors) -> int:
        """Bulk upload without graph construction (exact search only until a graph exists)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        vecs = _f32(vectors)
        assert vecs.ndim == 2 and vecs.shape[1] == self._dimension, \
            f"Vector dimension mismatch: expected {self._dimension}, got {vecs.shape[-1]}"
        assert ids.shape[0] == vecs.shape[0], f"{ids.shape[0]} ids for {vecs.shape[0]} vectors"
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_upload(self._h, _ptr(ids), _ptr(vecs), vecs.shape[0], C.byref(n)))
        return int(n.value)

    def upload_vector_store(self, directory: str) -> int:
        """Upload every vector of a flushed MmapStorage directory (core/storage/mmap.rs: vectors.idx + vectors.dat),
        in the order the store first saw the ids; no graph (as `upload`).  Returns the number of rows added."""
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_upload_vector_store(self._h, directory.encode(), C.byref(n)))
        return int(n.value)

    # ---- maintenance (index/hnsw/index/vacuum.rs) ------------------------------------------
    def tombstone_count(self) -> int:
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_tombstone_count(self._h, C.byref(n)))
        return int(n.value)

    def tombstone_ratio(self) -> float:  # vacuum.rs:60-67
        total = self.node_count()
        return 0.0 if total == 0 else self.tombstone_count() / total

    def needs_vacuum(self) -> bool:  # vacuum.rs:74-76
        return self.tombstone_ratio() > 0.2

    def vacuum(self) -> int:
        """Rebuild without tombstones (vacuum.rs:110-184); returns the number of vectors in the rebuilt index."""
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_vacuum(self._h, C.byref(n)))
        self.params = HnswParams.auto(self._dimension)
        return int(n.value)

    def set_searching_mode(self) -> None:  # search.rs:380-384: no-op for the native engine
        pass

    def save(self, directory: str, basename: Optional[str] = None) -> None:
        """HnswIndex::save (constructors.rs:255-287): native_hnsw.{vectors,graph} + native_mappings.bin +
        native_meta.bin in `directory`.  With a `basename`: only the graph + vector files under that name
        (NativeHnsw::file_dump, backend_adapter.rs:184-261)."""
        os.makedirs(directory, exist_ok=True)
        if basename is None:
            check(lib().vdb_hip_index_save_dir(self._h, directory.encode()))
        else:
            check(lib().vdb_hip_index_save_reference_files(self._h, directory.encode(), basename.encode()))

    @classmethod
    def load(cls, directory: str, dimension: int = 0, metric: Optional[DistanceMetric] = None, device: int = 0):
        """HnswIndex::load (constructors.rs:190-253); dimension / metric are read from the metadata file, the
        arguments exist for API compatibility like the reference's."""
        h = C.c_void_p()
        check(lib().vdb_hip_index_load_dir(directory.encode(), device, C.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        d, m = C.c_uint32(0), C.c_int32(0)
        check(lib().vdb_hip_index_dimension(h, C.byref(d)))
        check(lib().vdb_hip_index_metric(h, C.byref(m)))
        self._dimension, self._metric = int(d.value), DistanceMetric(m.value)
        self.params = HnswParams.auto(self._dimension)
        return self

    def load_reference_files(self, directory: str, basename: str = "native_hnsw") -> None:
        check(lib().vdb_hip_index_load_reference_files(self._h, directory.encode(), basename.encode()))

    def sweep_arith_mode(self, k: int) -> str:
        """'M' if exact searches with this k run on the matrix-core kernel (oracle mode M), else 'C'."""
        m = C.c_int32(0)
        check(lib().vdb_hip_index_sweep_arith_mode(self._h, k, C.byref(m)))
        return "M" if m.value else "C"

    # ---- introspection ------------------------------------------------------------------
    def node_count(self) -> int:
        n = C.c_uint64(0)
        check(lib().vdb_hip_index_node_count(self._h, C.byref(n)))
        return int(n.value)

    def neighbors(self, layer: int, node: int) -> List[int]:
        buf = np.empty(1024, dtype=np.uint32)
        n = C.c_uint32(0)
        check(lib().vdb_hip_index_get_neighbors(self._h, layer, node, _ptr(buf), buf.size, C.byref(n)))
        return buf[: n.value].tolist()

    def graph_info(self):
        nl, ml, ep = C.c_uint32(0), C.c_uint32(0), C.c_int64(-1)
        check(lib().vdb_hip_index_graph_info(self._h, C.byref(nl), C.byref(ml), C.byref(ep)))
        return int(nl.value), int(ml.value), int(ep.value)

    def last_search_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().vdb_hip_index_last_search_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def build_stats(self):
        """Construction counters, cumulative since the handle was created: (rows whose distance was evaluated by the insert kernel's
        search_layer / select_neighbors phases, distance phases = dependent memory round trips, nodes inserted, the rows of the first
        count that were select_neighbors evaluations — re-reads of a node's <= ef_construction candidate rows, cache hits)."""
        a, b, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().vdb_hip_index_build_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    def last_prefetch_hits(self):
        """Expansions of the last graph search batch whose neighbour ids had been requested one pop ahead (the walk's prediction)."""
        a = C.c_uint64(0)
        check(lib().vdb_hip_index_last_prefetch_hits(self._h, C.byref(a)))
        return int(a.value)

    def last_split_stats(self):
        """(queries, unproven) of the last split-selector batch: unproven ones were answered by the exact fallback kernel."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        check(lib().vdb_hip_index_last_split_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_option(self, option: int, value: int) -> None:
        """Per-handle tuning option (OPT_*); value < 0 = follow the process-wide default again.  Results never depend on it."""
        check(lib().vdb_hip_index_set_option(self._h, int(option), int(value)))

    def get_option(self, option: int) -> int:
        v = C.c_int64(0)
        check(lib().vdb_hip_index_get_option(self._h, int(option), C.byref(v)))
        return int(v.value)

    def combine_stats(self):
        """Counters of the combining front: (launches, calls, queries, largest batch) since the handle was created."""
        v = [C.c_uint64(0) for _ in range(4)]
        check(lib().vdb_hip_index_combine_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def last_select_level(self) -> int:
        """Selection level the last exact batch of this handle ran at: 0 = exact kernels, 1 = split-bf16, 2 = plain bf16 (Cosine: normalised
        images), 3 = the SQ8 storage mode's, 4 = the WIDE selection of 10 < k <= 128 (csrc/sweep_wide.hip)."""
        v = C.c_int32(0)
        check(lib().vdb_hip_index_last_select_level(self._h, C.byref(v)))
        return int(v.value)

    def last_kernels(self) -> int:
        """Bit set (KERNEL_*) of the kernel families that served the last search call."""
        v = C.c_uint32(0)
        check(lib().vdb_hip_index_last_kernels(self._h, C.byref(v)))
        return int(v.value)

    def last_selection_ms(self):
        """(total ms, launches) of the selection kernel in the last search call (kernel timing on)."""
        ms, n = C.c_float(0), C.c_uint32(0)
        check(lib().vdb_hip_index_last_selection_ms(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def last_kernel_ms(self):
        ms, n = C.c_float(0), C.c_uint32(0)
        check(lib().vdb_hip_index_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    # ---- device-pointer entry points (torch / raw HIP pointers) --------------------------
    def upload_dev(self, id_base: int, d_ptr: int, n: int, stream: int = 0) -> None:
        check(lib().vdb_hip_index_upload_dev(self._h, id_base, C.c_void_p(d_ptr), n, C.c_void_p(stream)))

    def search_batch_dev(self, d_queries: int, nq: int, k: int, ef: int, mode: int, d_ids: int, d_scores: int,
                         d_n: int, stream: int = 0) -> None:
        check(lib().vdb_hip_index_search_batch_dev(self._h, C.c_void_p(d_queries), nq, k, ef, mode,
                                                   C.c_void_p(d_ids), C.c_void_p(d_scores), C.c_void_p(d_n),
                                                   C.c_void_p(stream)))


class NativeHnswIndex(HnswIndex):
    """index/hnsw/native_index.rs: the reference's second `impl VectorIndex` (:403-427) over the same NativeHnsw graph.  What
    differs from HnswIndex is the search entry point: `search_with_quality` ALWAYS walks the graph with
    ef = quality.ef_search(k) (:230-249) — no exact-scan shortcut for Perfect or for indexes of <= 100 vectors, scores always
    through transform_score; removed ids are dropped after the cut (:241-247, mappings.get_id).  Deviation kept from
    HnswIndex: a duplicate id is skipped (the reference re-inserts the vector under the existing internal index, :256-263,
    which links one node twice)."""

    def search_with_quality(self, query, k: int, quality: SearchQuality) -> List[Tuple[int, float]]:
        q = _f32(query).reshape(1, -1)
        self._validate(q)
        ids, sc, cnt = self._search_raw(q, k, quality.ef_search(k), MODE_HNSW)
        return self._tuples(ids[0], sc[0], cnt[0])

    def insert_batch(self, items) -> None:  # native_index.rs:275-295
        self.insert_batch_parallel(items)


class HipDistance:
    """DistanceEngine (native/distance.rs:14-28) whose batch_distance runs on the GPU."""

    def __init__(self, metric: DistanceMetric, device: int = 0):
        self._metric = DistanceMetric(metric)
        self.device = device

    def metric(self) -> DistanceMetric:
        return self._metric

    def batch_distance(self, query, candidates) -> np.ndarray:
        q = _f32(query).reshape(-1)
        c = _f32(candidates)
        if c.size == 0:
            return np.empty(0, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == q.size, "Vector dimensions must match"
        out = np.empty(c.shape[0], dtype=np.float32)
        check(lib().vdb_hip_batch_distance(self.device, int(self._metric), KIND_ENGINE, _ptr(q), _ptr(c),
                                           c.shape[0], q.size, _ptr(out)))
        return out

    def batch_distance_dev(self, d_query: int, d_rows: int, n: int, dim: int, d_out: int, stream: int = 0,
                           kind: int = KIND_ENGINE) -> None:
        """The same over device-resident buffers (vdb_hip_batch_distance_dev): `d_query` dim floats, `d_rows` n x dim floats row-major,
        `d_out` n floats — device addresses aligned to 4 bytes or better — enqueued on `stream`; nothing synchronises.  Runs on the
        device the buffers live on (the caller's current device), not on `self.device`."""
        check(lib().vdb_hip_batch_distance_dev(int(self._metric), kind, C.c_void_p(d_query), C.c_void_p(d_rows), n, dim,
                                               C.c_void_p(d_out), C.c_void_p(stream)))

    def distance(self, a, b) -> float:
        return float(self.batch_distance(a, _f32(b).reshape(1, -1))[0])


class GpuAccelerator:
    """gpu/gpu_backend.rs:33-415: new() -> None without a GPU; batch_* return raw similarities."""

    def __init__(self, device: int = 0):
        self.device = device

    @staticmethod
    def new(device: int = 0) -> Optional["GpuAccelerator"]:
        return GpuAccelerator(device) if device_count() > 0 else None

    @staticmethod
    def is_available() -> bool:
        return device_count() > 0

    def _batch(self, metric, vectors, query, dimension) -> np.ndarray:
        v = _f32(vectors).reshape(-1)
        q = _f32(query).reshape(-1)
        if dimension == 0 or v.size == 0:
            return np.empty(0, dtype=np.float32)  # gpu_backend.rs:163-169
        assert q.size == dimension, f"Query dimension mismatch: expected {dimension}, got {q.size}"
        n = v.size // dimension
        if n == 0:
            return np.empty(0, dtype=np.float32)
        out = np.empty(n, dtype=np.float32)
        check(lib().vdb_hip_batch_distance(self.device, int(metric), KIND_RAW, _ptr(q), _ptr(v), n, dimension,
                                           _ptr(out)))
        return out

    def batch_cosine_similarity(self, vectors, query, dimension) -> np.ndarray:
        return self._batch(DistanceMetric.Cosine, vectors, query, dimension)

    def batch_euclidean_distance(self, vectors, query, dimension) -> np.ndarray:
        return self._batch(DistanceMetric.Euclidean, vectors, query, dimension)

    def batch_dot_product(self, vectors, query, dimension) -> np.ndarray:
        return self._batch(DistanceMetric.DotProduct, vectors, query, dimension)
