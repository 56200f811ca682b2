/*
 * velesdb_hip.h — C ABI of libvelesdb_hip.so: an MI355X (gfx950) implementation of
 * velesdb-core's HNSW similarity-search hot path.
 *
 * This is the drop-in boundary.  A Rust `velesdb-hip` shim binds these
 * symbols and implements the reference's own traits over the opaque handle:
 *   trait VectorIndex          crates/velesdb-core/src/index/mod.rs:30-83
 *   impl VectorIndex for HnswIndex   .../index/hnsw/index/trait_impl.rs:8-71
 *   HnswIndex inherent methods .../index/hnsw/index/search.rs, batch.rs, constructors.rs
 *   trait DistanceEngine       .../index/hnsw/native/distance.rs:14-28
 *   GpuAccelerator             crates/velesdb-core/src/gpu/gpu_backend.rs:33,136,157,355,397
 *
 * Conventions
 *   - every call returns an int32 status (0 = VDB_OK, >0 informational, <0 error); nothing
 *     unwinds across the boundary; vdb_hip_last_error() gives the thread-local message.
 *   - all buffers are caller-owned, plain pointers + sizes, row-major, little-endian.
 *   - "host" entry points take host pointers (what a Rust &[f32] is); "_dev" entry points take
 *     device pointers and a hipStream_t (as void*) and enqueue without synchronising.
 *   - a handle may be used from any thread (internally synchronised: Send + Sync).
 *   - there is NO CPU fallback: without a HIP device every compute call fails with
 *     VDB_ERR_NO_DEVICE (the reference's GpuAccelerator::new() == None, gpu_backend.rs:33).
 *   - result order: best first; equal scores are ordered by internal insertion index
 *     ascending (declared canonical tie-break; the reference's tie order is an artefact of
 *     heap / hash-map layout, SURVEY.md §8a note 8).
 */
#ifndef VELESDB_HIP_H
#define VELESDB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vdb_hip_index vdb_hip_index; /* opaque */

/* DistanceMetric, same discriminants as the reference's on-disk order
 * (index/hnsw/index/constructors.rs:204-210; core/distance.rs:16-38). */
enum vdb_metric {
  VDB_COSINE = 0,
  VDB_EUCLIDEAN = 1,
  VDB_DOT = 2,
  VDB_HAMMING = 3,
  VDB_JACCARD = 4
};

enum vdb_status {
  VDB_OK = 0,
  VDB_DUPLICATE_IGNORED = 1,  /* insert of an existing id: no-op (trait_impl.rs:23-25) */
  VDB_ERR_INVALID_ARG = -1,
  VDB_ERR_DIM_MISMATCH = -2,  /* the shim panics "… dimension mismatch: expected {}, got {}" */
  VDB_ERR_NO_DEVICE = -3,
  VDB_ERR_HIP = -4,
  VDB_ERR_IO = -5,
  VDB_ERR_OOM = -6,
  VDB_ERR_UNSUPPORTED = -7,
  VDB_ERR_STATE = -8
};

/* search `mode` */
enum vdb_search_mode {
  VDB_SEARCH_AUTO = 0,  /* HnswIndex::search_with_quality (search.rs:59-94): brute force when
                           len<=100, else HNSW with `ef`; scores = transform_score           */
  VDB_SEARCH_BRUTE = 1, /* HnswIndex::search_brute_force (search.rs:176-219): exact scan, raw
                           similarity/distance scores, metric.sort_results order             */
  VDB_SEARCH_HNSW = 2,  /* always the graph (search_batch_parallel, batch.rs:180-194)        */
  VDB_SEARCH_HNSW_INT8 = 4, /* DualPrecisionHnsw::search_with_config(use_int8_traversal) (native/dual_precision.rs:
                           223-441): the graph is walked with integer L2^2 distances between u8 codes (4x fewer bytes
                           per visited node), the k * oversampling best are re-scored with the exact f32 distance.
                           `ef` = ef_search; needs vdb_hip_index_train_quantizer.  Scores as in VDB_SEARCH_HNSW. */
  VDB_SEARCH_BRUTE_SQ8 = 5, /* exact scan of the f32 queries over the SQ8 codes of the rows with the reference's asymmetric
                           distances (core/quantization.rs:410-554): Cosine -> cosine_similarity_quantized_simd, DotProduct
                           -> dot_product_quantized_simd (best = largest), Euclidean -> euclidean_squared_quantized_simd (the
                           SQUARED distance, best = smallest).  Needs vdb_hip_index_set_storage_mode(VDB_STORAGE_SQ8).  */
  VDB_SEARCH_BRUTE_BINARY = 6, /* exact scan by BinaryQuantizedVector::hamming_distance (quantization.rs:123-135) between
                           the sign bits of the query and of every row; scores = the distance as f32, smallest first.
                           Needs VDB_STORAGE_BINARY; any metric.                                              */
  VDB_SEARCH_BRUTE_BF16 = 3, /* exact scan over the bf16 copy of the rows with bf16-rounded queries and f32
                           accumulation on the matrix cores: half_precision::dot_product / cosine_similarity on
                           VectorData::BF16 (half_precision.rs:199-255); needs vdb_hip_index_enable_bf16 or
                           vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16).  On a Euclidean handle (the second call
                           only): half_precision::euclidean_distance (:257-287), sqrt of an f32 chain of (q - v)^2 over the
                           rounded values, smallest first.  Raw scores, best first.                  */
  VDB_SEARCH_BRUTE_F16 = 7, /* the same over the IEEE f16 copy of the rows (VectorData::F16: round to nearest even, overflow to
                           +-inf beyond 65 504, f16 subnormals kept) with f16-rounded queries: Cosine / DotProduct on the matrix
                           cores (v_mfma_f32_16x16x32_f16, f32 accumulation); Euclidean (half_precision.rs:257-279) as sqrt of an f32
                           chain of (q - v)^2 over the rounded values, smallest first.  Needs
                           vdb_hip_index_enable_half_precision(VDB_PRECISION_F16).                                   */
  VDB_SEARCH_HNSW_F16 = 8,  /* VDB_SEARCH_HNSW over the IEEE f16 copy of the rows: NativeHnsw::search (graph.rs:251-270) on the handle's
                           graph under the same result mapping (`ef` = 0 -> Balanced, max(ef, k), soft-deleted rows dropped after
                           the cut, scores through transform_score), every distance of the walk taken between the query rounded
                           to f16 (VectorData::from_f32_slice) and the row's f16 image: -dot, 1 - cosine_similarity (0.0
                           similarity when a norm is < f32::EPSILON), euclidean_distance (half_precision.rs:199-287), summed in
                           the canonical order of the f32 walk.  Half the bytes per visited node, no training step.  Needs
                           vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) (VDB_ERR_STATE otherwise, as
                           VDB_SEARCH_BRUTE_F16) and a graph (VDB_ERR_STATE).  Served by vdb_hip_index_search / _search_batch /
                           _search_batch_dev and by REPLICA device groups; RANGE groups answer VDB_ERR_UNSUPPORTED.  The
                           rerank / multi-entry / with_config entry points and VDB_SEARCH_AUTO never take this walk; the form
                           that re-scores the walk's candidates with the exact f32 distance is a call of its own,
                           vdb_hip_index_search_graph_filters_half_rescore (with or without filters).                  */
  VDB_SEARCH_HNSW_BF16 = 9  /* the same over the bf16 copy (VDB_PRECISION_BF16)                                                 */
};

/* VectorPrecision (half_precision.rs:36-44), the reference's order */
enum vdb_vector_precision {
  VDB_PRECISION_F32 = 0,
  VDB_PRECISION_F16 = 1,
  VDB_PRECISION_BF16 = 2
};

/* StorageMode (core/quantization.rs:17-29): which quantised copy of the rows the index keeps next to the f32 rows */
enum vdb_storage_mode {
  VDB_STORAGE_FULL = 0,  /* f32 only (default)                                                                  */
  VDB_STORAGE_SQ8 = 1,   /* QuantizedVector: one byte per dimension, per-vector min / max (quantization.rs:204-255) */
  VDB_STORAGE_BINARY = 2 /* BinaryQuantizedVector: bit = (x >= 0.0), LSB first (quantization.rs:48-86)           */
};

/* score convention of vdb_hip_batch_distance */
enum vdb_distance_kind {
  VDB_KIND_ENGINE = 0, /* DistanceEngine::distance (native/distance.rs:75-85): 1-cos, sqrt(l2),
                          -dot, hamming, 1-jaccard                                          */
  VDB_KIND_RAW = 1,    /* HnswIndex::compute_distance / GpuAccelerator::batch_* (search.rs:30-38;
                          gpu_backend.rs:157,355,397): cos, sqrt(l2), dot, hamming, jaccard.  With VDB_DOT this is also
                          simd::cosine_similarity_normalized / batch_cosine_normalized (simd_avx512.rs:390-422: the
                          cosine of pre-normalised vectors IS their dot product)                     */
  VDB_KIND_SQUARED = 2 /* simd::squared_l2_distance (simd.rs:207-211): VDB_EUCLIDEAN without the sqrt */
};

/* ---- device discovery: GpuAccelerator::new()/is_available() (gpu_backend.rs:33,136) ---- */
int32_t vdb_hip_device_count(int32_t* n);
int32_t vdb_hip_device_name(int32_t device, char* buf, size_t cap);

/* how a handle spreads over several GPUs of one node */
enum vdb_shard_mode {
  VDB_SHARD_REPLICA = 0, /* every device holds every row (and the graph); a query batch is split between the devices,
                            no collective — the mode of the graph path                                           */
  VDB_SHARD_RANGE = 1    /* contiguous ranges of the internal rows: row r lives on device min(r / C, n - 1),
                            C = ceil(max_elements / n); exact searches = per-shard top-k, ONE RCCL all-gather of
                            k (id, score) records per query and device, merge — BASELINE configs[4]              */
};

/* ---- lifecycle: HnswIndex::with_params (constructors.rs:117-160) ----
 * M = max_connections, M0 = 2M (native/graph.rs:62); max_elements is a capacity hint (storage grows; with
 * VDB_SHARD_RANGE it also fixes the rows per shard).  `devices` = n_devices HIP device ordinals (NULL / 0 = device 0).
 * One VectorIndex object whatever is behind it (index/mod.rs:30-83): with n_devices > 1 the handle owns one shard per
 * device and every entry point below works on the whole; results (ids, ranks, score bits, tie order) of the exact
 * search modes are those of the single-device index over the same rows.  The same device may be named more than once
 * (co-located shards: the exchange is then a device-to-device copy instead of RCCL — a test configuration).
 * HNSW modes on a VDB_SHARD_RANGE handle search one graph per shard and merge (recall differs from one big graph).
 * A single-device index (one shard) holds at most 2^32 - 512 rows: inserts past that answer VDB_ERR_UNSUPPORTED. */
int32_t vdb_hip_index_create(uint32_t dim, int32_t metric, uint32_t M, uint32_t ef_construction,
                             uint64_t max_elements, const int32_t* devices, int32_t n_devices, int32_t shard_mode,
                             vdb_hip_index** out);
/* One process per GPU (torchrun, MPI): every rank creates its own single-device index = ONE shard of a range-sharded
 * corpus (rank order = row order) and joins the group with the 128-byte id rank 0 generated and distributed out of
 * band.  From then on the exact search modes of this handle return the GLOBAL top-k on every rank: local top-k, one
 * ncclAllGather of nq * k 12-byte (u64 id, f32 score) records per rank, merge kernel.  Collective: every rank must
 * call search with the same queries, k and mode.  world == 1 is allowed (the collective degenerates). */
#define VDB_COMM_ID_BYTES 128
int32_t vdb_hip_comm_unique_id(uint8_t* id /* VDB_COMM_ID_BYTES */);
int32_t vdb_hip_index_join_group(vdb_hip_index* idx, const uint8_t* id, int32_t rank, int32_t world);
/* n_shards = devices behind the handle (1 for a plain index), shard_mode as created, rank / world of the process
 * group (0 / 1 without one), transport of the exchange: 0 none, 1 RCCL, 2 device-to-device copies */
int32_t vdb_hip_index_shard_info(vdb_hip_index* idx, int32_t* n_shards, int32_t* shard_mode, int32_t* rank,
                                 int32_t* world, int32_t* transport);
void vdb_hip_index_destroy(vdb_hip_index* idx);

/* ---- VectorIndex::insert (index/mod.rs:46, trait_impl.rs:10-36) ---- */
int32_t vdb_hip_index_insert(vdb_hip_index* idx, uint64_t id, const float* vec, uint32_t vec_len);
/* HnswIndex::insert_batch_sequential / insert_batch_parallel (batch.rs:83-149): rows are
 * dim floats each; *inserted = number of new ids (duplicates skipped). */
int32_t vdb_hip_index_insert_batch(vdb_hip_index* idx, const uint64_t* ids, const float* vecs_rowmajor,
                                   uint64_t n, uint64_t* inserted);
/* HnswIndex::insert_batch_parallel (batch.rs:83-108).  The reference inserts with rayon and is
 * non-deterministic; here the batch is inserted batch-synchronously (every node of a sub-batch
 * searches the graph as it was before the sub-batch, links applied sources ascending): deterministic,
 * restated in oracle/vdb_oracle.cpp hnsw_insert_batch_sync.  max_batch = largest sub-batch (0 =
 * default 2048; 1 = identical to insert_batch). */
int32_t vdb_hip_index_insert_batch_parallel(vdb_hip_index* idx, const uint64_t* ids, const float* vecs_rowmajor,
                                            uint64_t n, uint32_t max_batch, uint64_t* inserted);
/* ScalarQuantizer::train (native/quantization.rs:191-233) on the first sample_rows rows (0 = min(1000, rows), what
 * DualPrecisionHnsw uses) + u8 codes for every present and future row (+1 byte per element of HBM). */
int32_t vdb_hip_index_train_quantizer(vdb_hip_index* idx, uint32_t sample_rows);
/* DualPrecisionHnsw::is_quantizer_trained (native/dual_precision.rs:117-120): *trained = 1 once vdb_hip_index_train_quantizer ran
 * on this handle, else 0 (the codes are a derived image: they are not part of a saved directory, a loaded handle starts untrained). */
int32_t vdb_hip_index_quantizer_trained(const vdb_hip_index* idx, int32_t* trained);
/* DualPrecisionHnsw::search_with_config (native/dual_precision.rs:259-278) for a batch, the DualPrecisionConfig passed per call as
 * the reference passes it: the int8 graph traversal + exact f32 re-scoring of the k * oversampling_ratio best (dual_precision.rs:
 * 284-321) only when the quantiser is trained AND use_int8_traversal != 0 AND the index holds >= min_index_size vectors; otherwise
 * the plain f32 graph search — NativeHnsw::search with ef_search AS GIVEN (dual_precision.rs:269,274; graph.rs:251-270): the same
 * answer as VDB_SEARCH_HNSW when 0 < k <= ef_search; with ef_search < k at most ef_search results, ef_search = 0 acts as 1 (no
 * SearchQuality rule at this level; a device group keeps the HnswIndex rule).  oversampling_ratio = 0 or > 64 =>
 * VDB_ERR_INVALID_ARG (reference default 4, min_index_size default 10 000).  Ids / scores as VDB_SEARCH_HNSW reports them.  Does
 * not touch VDB_OPT_INT8_OVERSAMPLING. */
int32_t vdb_hip_index_search_with_config(vdb_hip_index* idx, const float* queries_rowmajor, uint32_t nq, uint32_t k,
                                         uint32_t ef_search, uint32_t oversampling_ratio, int32_t use_int8_traversal,
                                         uint64_t min_index_size, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* DualPrecisionConfig::oversampling_ratio (default 4) of VDB_SEARCH_HNSW_INT8, process-wide */
int32_t vdb_hip_set_int8_oversampling(uint32_t ratio);
/* Collection StorageMode (quantization.rs:17-29; collection/core/crud.rs:66-82 quantises every upserted vector):
 * encodes every present and future row on the device (SQ8: +dim+12 bytes per row, Binary: +dim/8) for the
 * VDB_SEARCH_BRUTE_SQ8 / VDB_SEARCH_BRUTE_BINARY scans.  Switching modes drops the previous codes. */
int32_t vdb_hip_index_set_storage_mode(vdb_hip_index* idx, int32_t mode);
/* the stored code of one vector in the reference's serialisation: QuantizedVector::to_bytes (min f32, max f32, dim
 * bytes; quantization.rs:289-295) or BinaryQuantizedVector::to_bytes (dimension u32, ceil(dim/8) bytes; :155-169).
 * *len = bytes needed / written. */
int32_t vdb_hip_index_get_quantized(vdb_hip_index* idx, uint64_t id, uint8_t* out, size_t cap, size_t* len);
/* keeps a bf16 copy (round to nearest even, VectorData::from_f32_slice(.., BF16), half_precision.rs:94-101) of every
 * row next to the f32 rows, for VDB_SEARCH_BRUTE_BF16; +2 bytes per element of HBM */
int32_t vdb_hip_index_enable_bf16(vdb_hip_index* idx);
/* VectorData::from_f32_slice(.., precision) for every row (half_precision.rs:94-101): keeps a half-precision copy (rows present now and
 * rows that arrive later through insert / upload / upload_dev; soft deletes honoured) next to the f32 rows, +2 bytes per element of
 * HBM, for VDB_SEARCH_BRUTE_F16 (VDB_PRECISION_F16) / VDB_SEARCH_BRUTE_BF16 (VDB_PRECISION_BF16).  Cosine, DotProduct and Euclidean
 * handles; VDB_ERR_UNSUPPORTED for Hamming / Jaccard and for VDB_PRECISION_F32.  Both precisions may be enabled on one handle (two
 * images).  On Cosine / DotProduct, VDB_PRECISION_BF16 is vdb_hip_index_enable_bf16 (which keeps refusing Euclidean handles).  A
 * multi-device handle forwards the call to every shard. */
int32_t vdb_hip_index_enable_half_precision(vdb_hip_index* idx, int32_t precision);
/* The graph precision: the row format every distance of graph CONSTRUCTION is taken over from this call on (insert, insert_batch,
 * insert_batch_parallel, build_graph, the rebuild inside vacuum).  VDB_PRECISION_F32 (the default): the f32 rows.  VDB_PRECISION_F16 /
 * _BF16: the distance between two nodes is half_precision::{dot_product, cosine_similarity, euclidean_distance}
 * (half_precision.rs:199-287) over their two image rows, reported as DistanceEngine::distance reports it; the inserted node's query is
 * its own image row dequantised (exact), its Cosine norm the stored norm of the rounded row.  The graph is then the one the
 * reference's sequential / batch-synchronous insert builds over the dequantised rows, link for link — the graph modes 8 / 9 and the
 * filtered half walks are meant to run on.  Needs the matching image (vdb_hip_index_enable_half_precision; VDB_ERR_STATE otherwise, as
 * modes 8 / 9); VDB_ERR_UNSUPPORTED on Hamming / Jaccard and multi-device handles, VDB_ERR_INVALID_ARG for an unknown precision; a
 * refused call changes nothing.  Allowed at any time, also on a graph that has nodes or was loaded from files: a change of precision
 * recomputes the cached neighbour distances in the new precision before the next insert (back-link pruning ranks by them).  Searches
 * are unaffected; filters stay valid; vacuum keeps the precision.  NOT persisted: neither the reference's file formats nor the index
 * directory has a field for it — a loaded handle starts at VDB_PRECISION_F32, call this again after a load. */
int32_t vdb_hip_index_set_graph_precision(vdb_hip_index* idx, int32_t precision);
int32_t vdb_hip_index_graph_precision(const vdb_hip_index* idx, int32_t* precision);
/* links every row that is not in the graph yet (rows that arrived through upload/upload_dev), same
 * schedule as insert_batch_parallel; afterwards the HNSW search modes are available. */
int32_t vdb_hip_index_build_graph(vdb_hip_index* idx, uint32_t max_batch);
/* bulk upload without graph construction: vectors become searchable by VDB_SEARCH_BRUTE at
 * once; the graph is absent until vdb_hip_index_build_graph / load_reference_files.
 * (HnswIndex keeps exact search available independently of the graph, search.rs:176-219.) */
int32_t vdb_hip_index_upload(vdb_hip_index* idx, const uint64_t* ids, const float* vecs_rowmajor,
                             uint64_t n, uint64_t* inserted);
/* same, rows already resident in HBM on the index's device (device pointer), ids = base..base+n-1 */
int32_t vdb_hip_index_upload_dev(vdb_hip_index* idx, uint64_t id_base, const float* d_vecs_rowmajor,
                                 uint64_t n, void* stream);

/* ---- VectorIndex::remove / len / dimension / metric (index/mod.rs:62-82) ---- */
int32_t vdb_hip_index_remove(vdb_hip_index* idx, uint64_t id, int32_t* removed); /* soft delete */
int32_t vdb_hip_index_len(const vdb_hip_index* idx, uint64_t* n);
int32_t vdb_hip_index_dimension(const vdb_hip_index* idx, uint32_t* dim);
int32_t vdb_hip_index_metric(const vdb_hip_index* idx, int32_t* metric);
/* HnswIndex::tombstone_count / vacuum (index/hnsw/index/vacuum.rs:45-52,110-184).  tombstone_ratio = count / node_count,
 * needs_vacuum = ratio > 0.2 (:60-76).  vacuum rebuilds the graph over the active vectors with HnswParams::auto(dim);
 * *count = vectors in the rebuilt index. */
int32_t vdb_hip_index_tombstone_count(const vdb_hip_index* idx, uint64_t* n);
int32_t vdb_hip_index_vacuum(vdb_hip_index* idx, uint64_t* count);
/* number of graph nodes (NativeHnsw::len, native/graph.rs:130-132; includes soft-deleted) */
int32_t vdb_hip_index_node_count(const vdb_hip_index* idx, uint64_t* n);

/* ---- VectorIndex::search + HnswIndex::search_with_quality/search_brute_force ----
 * ef = 0 => SearchQuality::Balanced rule max(128, 4k) (params.rs:309-319).
 * out_ids/out_scores hold k entries; *out_n <= k (soft-deleted rows can shorten HNSW results,
 * search.rs:86-91). */
int32_t vdb_hip_index_search(vdb_hip_index* idx, const float* query, uint32_t query_len, uint32_t k,
                             uint32_t ef, int32_t mode, uint64_t* out_ids, float* out_scores,
                             uint32_t* out_n);
/* HnswIndex::search_batch_parallel (batch.rs:159-197) for mode HNSW; one launch for all
 * queries.  out_ids/out_scores are nq*k, out_n is nq. */
int32_t vdb_hip_index_search_batch(vdb_hip_index* idx, const float* queries_rowmajor, uint32_t nq,
                                   uint32_t k, uint32_t ef, int32_t mode, uint64_t* out_ids,
                                   float* out_scores, uint32_t* out_n);
/* HnswIndex::search_with_rerank (search.rs:118-160) / search_with_rerank_quality (search.rs:297-350) for nq
 * queries: candidates = search_with_quality(query, rerank_k, quality) (ef = 0 => Accurate: max(512, 16*rerank_k);
 * otherwise Custom(ef)), re-scored with the raw compute_distance, stable-sorted in the metric's order, cut to
 * k.  Scores are RAW (similarity for Cosine/Dot/Jaccard, distance for Euclidean/Hamming), like search_brute_force. */
int32_t vdb_hip_index_search_rerank(vdb_hip_index* idx, const float* queries_rowmajor, uint32_t nq, uint32_t k,
                                    uint32_t rerank_k, uint32_t ef, uint64_t* out_ids, float* out_scores,
                                    uint32_t* out_n);
/* NativeHnsw::search_multi_entry (native/graph.rs:288-348; "improved recall on hard queries"): the layer-0 search starts from the
 * descent's result AND up to min(num_probes, 4) - 1 further nodes drawn from the graph's own xorshift stream (the stream that
 * draws insertion levels: like the reference, the call advances it — query i of the batch takes the draws nq sequential calls
 * would give it; duplicates are skipped; no draw when num_probes <= 1 or the graph has <= 10 nodes), same ef.  Ids / scores as
 * VDB_SEARCH_HNSW reports them.  `ef` is NativeHnsw's raw ef_search (graph.rs:343): no SearchQuality rule, no max(ef, k) — a call
 * with ef < k returns at most ef results per query (with more entry points than ef: as many as there are entry points, which is what
 * the reference's uncut `results` heap gives, graph.rs:463-468; ef = 0 therefore acts as ef = 1, NOT as "Balanced"). */
int32_t vdb_hip_index_search_multi_entry(vdb_hip_index* idx, const float* queries_rowmajor, uint32_t nq, uint32_t k, uint32_t ef,
                                         uint32_t num_probes, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* device-resident variant: d_queries nq*dim f32 (16-byte aligned), outputs device buffers of nq*k / nq; enqueued on `stream`,
 * no host synchronisation — with two exceptions: (1) Euclidean VDB_SEARCH_BRUTE batches of >= 64 queries that the selection
 * stage does not take (dim % 64 != 0, dim < 128, k > 10, or fewer than 65 536 rows) read their per-query verdicts back once per
 * <= 1 024-query chunk; (2) the first search that needs a derived image of the rows (bf16 / split / augmented / SQ8-dequantised /
 * four-bit bit image) builds it on `stream` and waits for it, so that other search contexts may use it.
 * In HNSW mode d_out_n[i] == 0xFFFFFFFF marks a query whose LDS candidate list overflowed (needs very many exact distance
 * ties) or, in calls of at most one query per CU, whose walk visited more nodes than the LDS visited set holds (> ~24 000 at
 * ef <= 270); the host variant above re-runs such batches with a larger list and the HBM visited bitmaps by itself. */
int32_t vdb_hip_index_search_batch_dev(vdb_hip_index* idx, const float* d_queries, uint32_t nq,
                                       uint32_t k, uint32_t ef, int32_t mode, uint64_t* d_out_ids,
                                       float* d_out_scores, uint32_t* d_out_n, void* stream);

/* ---- filtered exact search: an id allow-list applied inside the sweep ----
 * The reference's `_with_filter` searches (collection/search/vector.rs:164-239, batch.rs:26-136) post-filter: they over-fetch
 * max(4k, k + 10) candidates and drop what the predicate rejects, so a selective filter returns fewer than k results although many
 * rows match.  Here the caller hands over the SET OF IDS that matched (payloads and predicates stay the caller's) and the device
 * answers the exact top-k among exactly those rows.
 *
 * A filter is an immutable snapshot of internal rows.  `ids` are mapped through the handle's id map at creation (under the handle's
 * lock); unknown ids and duplicates are ignored; negate != 0 = "every row present now except these".  *matched (nullable) = rows in
 * the set (rows that are soft-deleted but still present count; they are dropped at search time).  n_ids == 0 with negate == 0 is a
 * legal empty filter: every search with it answers out_n = 0.  Rows inserted after creation are not in the filter; rows removed
 * after creation are excluded (the live flags are read at search time).  vdb_hip_index_vacuum and the load_* calls renumber the
 * rows of a handle: a filter created before them answers VDB_ERR_STATE, a filter of another handle VDB_ERR_INVALID_ARG — never
 * results.  A filter may be used by any number of concurrent searches.  It must be destroyed before its index; after the index is
 * gone it is valid for vdb_hip_filter_destroy only.  Costs n_rows / 8 + 4 * matched bytes of HBM.
 * VDB_ERR_UNSUPPORTED: a multi-device handle or a member of a process group. */
/* opaque.  At this boundary the filter handle is an untyped pointer: callers declare `vdb_hip_filter* f` and pass `&f` / `f` as
 * below; the index handle stays the one struct type of the ABI (what the binding checks of this project and sys.rs know). */
typedef void vdb_hip_filter;
int32_t vdb_hip_index_filter_create(vdb_hip_index* idx, const uint64_t* ids, uint64_t n_ids, int32_t negate, uint64_t* matched,
                                    void** out);
void vdb_hip_filter_destroy(void* f);
/* vdb_hip_index_search_batch in VDB_SEARCH_BRUTE restricted to the filter's rows, all five metrics: ids, ranks and score bits are
 * those VDB_SEARCH_BRUTE returns on an index that holds only the allowed live rows, inserted in the same order under the same ids
 * (the arithmetic is the handle's: vdb_hip_index_sweep_arith_mode) — a filter never changes a score.  Outputs, tie order, padding,
 * raw scores, k limits and errors as vdb_hip_index_search_batch.  f == NULL: VDB_ERR_INVALID_ARG.  Every other mode and every
 * multi-device handle: VDB_ERR_UNSUPPORTED (HnswIndex::search_filtered's over-fetch rule stays the shim's for the graph modes).
 * Two routes, same bits: the LISTED sweep (sweep_topk_listed: only the filter's rows are read, gathered by index; Cosine /
 * DotProduct / Euclidean; VDB_KERNEL_SWEEP_LISTED) and MASK SUBSTITUTION (the filter AND the live flags become the call's row mask
 * and every tier of the exact path serves it).  VDB_OPT_FILTER_ROUTE picks; auto = listed iff matched <= rows / 4 and
 * matched * nq <= 8 * rows (a stated guess, not a measurement: DESIGN 4.1g).  A filtered call never shares a launch with another
 * call (it does not go through the combining front) and leaves the handle's adaptive selection state as it found it. */
int32_t vdb_hip_index_search_batch_filtered(vdb_hip_index* idx, const void* f, const float* queries_rowmajor, uint32_t nq,
                                            uint32_t k, int32_t mode, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* The same over the SQ8 codes, the sign bits or a half image of the rows: the reference's search_with_filter works
 * whatever the collection's storage mode.  mode is one of VDB_SEARCH_BRUTE_SQ8, VDB_SEARCH_BRUTE_BINARY, VDB_SEARCH_BRUTE_BF16,
 * VDB_SEARCH_BRUTE_F16.
 * THE CONTRACT: the call returns what vdb_hip_index_search_batch(mode) returns on an index that holds only the filter's live rows,
 * inserted in the same order under the same ids, with the same storage mode / precision enabled — ids, ranks, score values, out_n and
 * padding.  SQ8, Binary and Euclidean over a half image: bit for bit (their summation orders are declared).  Cosine / DotProduct over
 * a half image: within the tolerance that mode carries, tie-aware (bit for bit on data whose partial sums are exact).
 * The filter semantics are vdb_hip_index_search_batch_filtered's: a snapshot; negate; the empty filter answers out_n = 0; rows removed
 * later are excluded, rows inserted later are not in it.
 * Two routes (VDB_OPT_FILTER_ROUTE, the same three values): the LISTED kernels — sweep_topk_sq8_listed (SQ8, all three metrics) and
 * sweep_topk_half_l2_listed (Euclidean over a half image) read only the filter's rows, gathered by index — and MASK SUBSTITUTION,
 * the mode's own dispatch with every tier of it under the call's row mask (the only route of Binary and of Cosine / DotProduct over a
 * half image).  Same bits on both where the bits are declared.  Auto (checked against one measurement): Euclidean over a
 * half image takes the listed kernel iff matched <= 3/4 rows; SQ8 only for calls of at most three queries, with the same cut.  With
 * fewer than 1/16 of the rows allowed the SQ8 selection stage is skipped, as the f32 one.
 * vdb_hip_index_last_kernels: the mode's usual bits, plus VDB_KERNEL_SWEEP_LISTED when a listed kernel ran.
 * Errors: null arguments and a filter of another handle VDB_ERR_INVALID_ARG; a stale filter VDB_ERR_STATE; a mode whose storage mode or
 * image is not enabled VDB_ERR_STATE, as the plain call; any other mode (VDB_SEARCH_BRUTE has the call above), multi-device handles and
 * process-group members VDB_ERR_UNSUPPORTED.  The outputs are untouched on error.  The call never goes through the combining front,
 * leaves the handle's adaptive selection state as it found it and posts no selection verdicts.  Host pointers only. */
int32_t vdb_hip_index_search_batch_filtered_mode(vdb_hip_index* idx, const void* f, int32_t mode, const float* queries_rowmajor,
                                                 uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* One filter PER QUERY on the exact sweep: the collection layer's search_batch_with_filters (collection/search/batch.rs:26-115;
 * DESIGN 4.1n).  The table follows vdb_hip_index_search_graph_filters below: filters = n_filters distinct filter handles of this
 * index; filter_of_query[i] in 0..n_filters-1 names query i's filter, filter_of_query[i] == n_filters = query i has NO filter;
 * n_filters == 0 with filters == NULL is legal.
 * THE CONTRACT: query i gets, bit for bit, what vdb_hip_index_search_batch_filtered returns for that query ALONE with its filter and
 * the same k — ids, ranks, score bits, out_n, padding — and a query without a filter what vdb_hip_index_search_batch(VDB_SEARCH_BRUTE)
 * returns for it alone.  A query's answer never depends on its companions, on its position in the batch, on VDB_OPT_FILTER_ROUTE or
 * on how the call grouped its work; a query with an empty filter gets out_n = 0 while the others are answered.
 * Queries are grouped by filter and every group takes the route vdb_hip_index_search_batch_filtered's rule gives it with ITS matched
 * count and ITS number of queries (VDB_OPT_FILTER_ROUTE applies per group).  The groups on the listed route share one set of
 * launches — sweep_topk_listed_groups / _groups_m, at most three launches (mode C: one per pass width 8 / 4 / 1) or one (mode M) and
 * ONE merge, whatever n_filters and nq are: VDB_KERNEL_SWEEP_LISTED_GROUPS —; the groups on mask substitution run one after another
 * through the exact path, and the unfiltered queries together as one such job.  A call whose queries all name ONE filter runs
 * vdb_hip_index_search_batch_filtered itself: the same launches, the same vdb_hip_index_last_kernels.
 * The call leaves the handle's adaptive selection state as it found it and posts no selection verdicts, for its unfiltered queries
 * too.  It never goes through the combining front.  All five metrics (Hamming / Jaccard: mask substitution per group).  k limits
 * and k errors as vdb_hip_index_search_batch_filtered.
 * Errors, checked for every filter of the table before anything runs: a NULL table entry or a filter of another handle, a
 * filter_of_query value > n_filters: VDB_ERR_INVALID_ARG; a stale filter: VDB_ERR_STATE; mode other than VDB_SEARCH_BRUTE,
 * multi-device handles and process-group members: VDB_ERR_UNSUPPORTED.  The outputs are untouched on error.  Host pointers only. */
int32_t vdb_hip_index_search_batch_filters(vdb_hip_index* idx, void** filters, uint32_t n_filters,
                                           const uint32_t* filter_of_query, const float* queries_rowmajor, uint32_t nq,
                                           uint32_t k, int32_t mode, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* One filter PER QUERY over the SQ8 codes, the sign bits or a half image of the rows: the reference's search_batch_with_filters works
 * whatever the collection's storage mode.  mode is one of VDB_SEARCH_BRUTE_SQ8, VDB_SEARCH_BRUTE_BINARY,
 * VDB_SEARCH_BRUTE_BF16, VDB_SEARCH_BRUTE_F16.  The table's conventions are vdb_hip_index_search_batch_filters': the filters are
 * distinct handles of this index; filter_of_query[i] == n_filters means query i has no filter; n_filters == 0 with filters == NULL is
 * legal; every filter is checked before anything runs; the outputs are untouched on error; host pointers only; the call never goes
 * through the combining front.
 * THE CONTRACT:
 *  - SQ8, Binary, Euclidean over a half image: query i gets, bit for bit, what vdb_hip_index_search_batch_filtered_mode returns for
 *    that query ALONE with its filter, the same mode and the same k — ids, ranks, score bits, out_n and padding.  A query without a
 *    filter gets what vdb_hip_index_search_batch(mode) returns for it alone.  (These modes' summation orders are declared.)
 *  - Cosine / DotProduct over a half image: the bits depend on the matrix-core tier, which depends on the batch size.  Query i gets
 *    bit for bit what the one-filter mode call returns for its GROUP — the queries that name the same filter, in call order; the
 *    group runs as exactly that job.  That result is within the mode's existing tolerance, tie-aware, of the query alone, and bit for
 *    bit on data whose partial sums are exact.  The unfiltered queries are held to the plain mode call over them, in call order, the
 *    same way.
 *  - Independence: an answer never depends on the query's companions outside its group, on its position in the batch, or on
 *    VDB_OPT_FILTER_ROUTE — the half Cosine / DotProduct tier being the one exception, as stated above.
 *  - Empty filters: a query of an empty filter gets out_n = 0 behind the merge's padding, as vdb_hip_index_search_batch_filters
 *    defines it, while the others are answered.
 * Queries are grouped by filter, call order kept inside a group, and every group takes the route the one-filter mode call's rule gives
 * it with ITS matched count and ITS number of queries (VDB_OPT_FILTER_ROUTE applies per group; auto sends an SQ8 group to the listed
 * kernel only with at most three queries; Binary and Cosine / DotProduct over a half image have no listed kernel).  The groups on the
 * listed route share launches — sweep_topk_sq8_listed_groups / sweep_topk_half_l2_listed_groups, at most three (one per pass width:
 * 8 / 4 / 1 for SQ8, 16 / 4 / 1 for half Euclidean) and ONE merge, whatever n_filters and nq are —; the groups on mask substitution run
 * one after another through the mode's own dispatch, the unfiltered queries together as one job of the plain mode call.  A call whose
 * queries all name ONE filter runs vdb_hip_index_search_batch_filtered_mode itself: the same launches, the same
 * vdb_hip_index_last_kernels.
 * vdb_hip_index_last_kernels: the mode's usual bits, plus VDB_KERNEL_SWEEP_LISTED_GROUPS when a grouped launch ran;
 * vdb_hip_index_last_filters_exact_plan reports this call's plan too.
 * The call leaves the handle's adaptive selection state (the hold counters of the selection stages, the verdict sequence) as it found
 * it and posts no selection verdicts, for its unfiltered job too.
 * Errors: the table's are vdb_hip_index_search_batch_filters' (a NULL table entry or a filter of another handle, a filter_of_query
 * value > n_filters: VDB_ERR_INVALID_ARG; a stale filter: VDB_ERR_STATE); the mode's and the state's are
 * vdb_hip_index_search_batch_filtered_mode's: a mode whose storage mode or image is not enabled VDB_ERR_STATE (checked before an empty
 * filter's out_n = 0); VDB_SEARCH_BRUTE (it has vdb_hip_index_search_batch_filters), every other mode, multi-device handles and
 * process-group members VDB_ERR_UNSUPPORTED. */
int32_t vdb_hip_index_search_batch_filters_mode(vdb_hip_index* idx, void** filters, uint32_t n_filters,
                                                const uint32_t* filter_of_query, int32_t mode, const float* queries_rowmajor,
                                                uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* diagnostic: the plan of THIS THREAD's last vdb_hip_index_search_batch_filters or vdb_hip_index_search_batch_filters_mode call on the handle (the rule of
 * vdb_hip_index_last_kernels).  out holds six values: out[0] distinct filter groups, out[1] groups on the listed route, out[2] groups on mask
 * substitution, out[3] unfiltered queries, out[4] grouped sweep launches, out[5] merge launches behind them (a call that ran the
 * one-filter path itself has none of either: out[4] = out[5] = 0). */
int32_t vdb_hip_index_last_filters_exact_plan(vdb_hip_index* idx, uint32_t* out);
/* Filtered GRAPH search: VDB_SEARCH_HNSW with the allow-list consulted inside the walk (hnsw_filtered.hip).
 * allowed(r) = r < the filter's row count, its bit r set, row r alive at search time (the rules above).  The greedy descent over the
 * upper layers is unfiltered (rejected nodes navigate); layer 0 is search_layer (native/graph.rs:438-520) with ONE change: `results`
 * receives allowed nodes only, `candidates` and `visited` what they receive today — furthest = the largest distance among the (at
 * most ef) allowed results, f32::MAX while there are none; a neighbour is pushed to candidates when `dist < furthest ||
 * results.len() < ef` and to results when it is also allowed.  Answer: the first min(k, results.len()) results, ids through the id
 * map, scores through transform_score — no post-drop.  ef as VDB_SEARCH_HNSW (0 = Balanced max(128, 4k); max(ef, k)); mode C
 * arithmetic; ties by (total-order(distance), internal row).  With a filter that allows every row the call IS VDB_SEARCH_HNSW: ids,
 * score bits, out_n and the search counters.
 * Cost: while fewer than ef allowed nodes are known the walk admits every node it sees, so its candidate list — LDS, per query in
 * flight — grows with 1 / density, and a query whose list would pass the largest one allowed is answered EXACTLY instead: top-k of
 * the allowed live rows by (total-order(distance), row), distances by the walk's own function (same score bits for the same id).
 * The largest list = what 160 KB of LDS hold at the graph's neighbour-list length, lowered by max_list when non-zero.
 * route 0 (auto): the whole call takes the exact pass when matched < ef, or when the density-sized list
 *   64-rounded(2 * ef * rows / matched + 64) exceeds the largest list; otherwise it walks with that list, re-runs queries that
 *   overflow it with four times the room up to the largest list, and answers those that still overflow exactly, one by one.  The
 *   factor 2 and the `matched < ef` cut are STATED GUESSES, nothing is measured (tools/filter_probe.py, graph leg).
 * route 1 (walk): always the walk; a query that overflows the largest list fails the call with VDB_ERR_UNSUPPORTED.
 * route 2: the exact pass for every query.
 * out_route (nullable, [nq]): 1 = the walk answered, 2 = the exact pass, 0 = nothing ran (empty filter, k = 0, empty graph: out_n = 0).
 * A query's route depends on the query, the filter, ef and max_list — never on the other queries of the call.
 * mode other than VDB_SEARCH_HNSW, multi-device handles and process-group members: VDB_ERR_UNSUPPORTED; f == NULL or route outside
 * 0..2: VDB_ERR_INVALID_ARG; a filter of another handle: VDB_ERR_INVALID_ARG; a stale filter or no graph: VDB_ERR_STATE.  Host
 * pointers only; a launch of its own (no combining front).  vdb_hip_index_last_kernels: VDB_KERNEL_HNSW_FILTERED and / or
 * VDB_KERNEL_FILTER_RANK; vdb_hip_index_last_search_stats: per query the counters of its last walk attempt plus the rows its exact
 * pass evaluated (n_dist only), summed over the call. */
int32_t vdb_hip_index_search_graph_filtered(vdb_hip_index* idx, const void* f, const float* queries_rowmajor, uint32_t nq,
                                            uint32_t k, uint32_t ef, int32_t mode, int32_t route, uint32_t max_list,
                                            uint64_t* out_ids, float* out_scores, uint32_t* out_n, uint32_t* out_route);
/* One filter PER QUERY in one graph call: the collection layer's search_batch_with_filters (collection/search/batch.rs:26-115;
 * DESIGN 4.1i).  filters = n_filters distinct filter handles of this index; filter_of_query[i] in 0..n_filters-1 names query i's
 * filter, filter_of_query[i] == n_filters = query i has NO filter, defined as a filter created at the moment of the call with
 * negate = 1 and no ids (every row present now; dead rows are dropped inside the walk).  n_filters == 0 with filters == NULL is
 * legal: every query is unfiltered.
 * THE CONTRACT: query i gets, bit for bit, what vdb_hip_index_search_graph_filtered returns for that query ALONE with its filter and
 * the same k, ef, route, max_list — ids, ranks, score bits, out_n, padding, out_route[i], and its share of the search counters
 * (vdb_hip_index_last_search_stats = the sum of the single calls' counters).  A query's answer and route never depend on its
 * companions or on its position in the batch: a query with an empty filter gets out_n = 0 and route 0 while the others are
 * answered.  Queries whose candidate lists differ in size share launches (at most four walk launches per attempt round, one launch
 * for every exact pass of the call).  route 1: a query that overflows the largest list fails the WHOLE call with
 * VDB_ERR_UNSUPPORTED (the message says how many did).
 * Errors, checked for every filter of the table before anything runs: a NULL table entry or a filter of another handle, a
 * filter_of_query value > n_filters, route outside 0..2: VDB_ERR_INVALID_ARG; a stale filter or no graph: VDB_ERR_STATE; mode other
 * than VDB_SEARCH_HNSW, multi-device handles and process-group members: VDB_ERR_UNSUPPORTED.  The outputs are untouched on error.
 * Host pointers only; launches of its own (no combining front).  vdb_hip_index_last_kernels: VDB_KERNEL_HNSW_FILTERED and / or
 * VDB_KERNEL_FILTER_RANK (one kernel family serves this call and the one above). */
int32_t vdb_hip_index_search_graph_filters(vdb_hip_index* idx, void** filters, uint32_t n_filters,
                                           const uint32_t* filter_of_query, const float* queries_rowmajor, uint32_t nq,
                                           uint32_t k, uint32_t ef, int32_t mode, int32_t route, uint32_t max_list,
                                           uint64_t* out_ids, float* out_scores, uint32_t* out_n, uint32_t* out_route);
/* vdb_hip_index_search_graph_filters over the HALF-PRECISION image of the rows (hnsw_filtered.hip): mode is
 * VDB_SEARCH_HNSW_F16 or VDB_SEARCH_HNSW_BF16.  Everything vdb_hip_index_search_graph_filters promises holds — the filter table,
 * "no filter" = n_filters, allowed(r), routes 0 / 1 / 2, max_list, out_route, padding, a query's independence from its companions
 * and its position, the summed counters — with every distance of the walk AND of the exact pass taken as the plain
 * VDB_SEARCH_HNSW_F16 / _BF16 walk takes it: between the query rounded to the precision and the row's image, mode C summation order,
 * the Cosine EPSILON rule.  A row has the same score bits on either route.  One filter for a whole call is a table of one.
 * Two corollaries:
 *   - with no query filtered (n_filters = 0, or "no filter" everywhere) on a handle without dead rows the call IS
 *     vdb_hip_index_search_batch(mode): ids, score bits, out_n, n_dist and n_expand;
 *   - on a handle whose f32 rows already equal their image (rows inserted already rounded), with queries already rounded, the call
 *     equals vdb_hip_index_search_graph_filters(VDB_SEARCH_HNSW) bit for bit, routes and counters included — DotProduct and Euclidean
 *     on any data, Cosine when no norm is below f32::EPSILON.
 * The route plan, the list sizes, the attempt rounds and the largest list are the f32 call's (the lists hold f32 distances and the
 * query scratch is f32); a visited node costs 2 * stride bytes (+ 4 for the Cosine norm) instead of 4 * stride.
 * Errors, all checked before anything runs, the outputs untouched: mode other than VDB_SEARCH_HNSW_F16 / _BF16, Hamming / Jaccard
 * handles, multi-device handles and process-group members: VDB_ERR_UNSUPPORTED; no image of that precision
 * (vdb_hip_index_enable_half_precision): VDB_ERR_STATE, as modes 8 / 9 of vdb_hip_index_search_batch; a NULL table entry, a filter of
 * another handle, a filter_of_query value > n_filters, route outside 0..2: VDB_ERR_INVALID_ARG; a stale filter or no graph:
 * VDB_ERR_STATE.  vdb_hip_index_last_kernels: VDB_KERNEL_HNSW_FILTERED and / or VDB_KERNEL_FILTER_RANK together with
 * VDB_KERNEL_HNSW_HALF, plus VDB_KERNEL_F16 for f16.  The two calls above keep refusing modes 8 and 9. */
int32_t vdb_hip_index_search_graph_filters_half(vdb_hip_index* idx, int32_t mode, void** filters, uint32_t n_filters,
                                                const uint32_t* filter_of_query, const float* queries_rowmajor, uint32_t nq,
                                                uint32_t k, uint32_t ef, int32_t route, uint32_t max_list, uint64_t* out_ids,
                                                float* out_scores, uint32_t* out_n, uint32_t* out_route);
/* vdb_hip_index_search_graph_filters over the U8 CODES of the trained scalar quantiser (hnsw_filtered.hip): the walk of
 * DualPrecisionHnsw::search_with_config(use_int8_traversal) (native/dual_precision.rs:223-441) with the allow-list consulted inside
 * it.  For one query: ef_search' = ef_search, or the Balanced rule max(128, 4k) when 0; ratio = oversampling_ratio, or the handle's
 * VDB_OPT_INT8_OVERSAMPLING / the process default when 0; cand_k = k * ratio; ef_w = max(ef_search', cand_k) (dual_precision.rs:334).
 * Every distance of the walk is the INTEGER L2^2 between the quantised query and the row's codes, ordered as an integer, keys
 * (distance, row); the greedy descent is unfiltered; layer 0 is the filtered search_layer of vdb_hip_index_search_graph_filters with
 * ef_w for ef, unchanged in every rule (results take allowed rows only, the pivot is the ef_w-th allowed entry, the overflow
 * report).  The first min(cand_k, results) allowed entries are re-scored with the exact f32 engine distance, stable-sorted by
 * total_cmp (equal distances keep the coarse order, dual_precision.rs:267-281) and cut to k; out_n = min(k, results); there is no
 * post-drop, allowed means alive.  The exact pass (route 2, the plan's whole-call cut, queries the largest list cannot hold) is the
 * f32 one of vdb_hip_index_search_graph_filters: the top-k of the allowed live rows by f32 engine distance — a row has the same score
 * bits on either route.  The route plan, ladders, max_list, out_route, padding, "no filter" = n_filters and a query's independence
 * from its companions and its position are that call's, with ef_w where the plan takes ef; the largest list follows the int8 walk's
 * LDS layout (the query's code words and the re-score output lie behind the lists).
 * Two corollaries:
 *   - with no query filtered (n_filters = 0, or "no filter" everywhere) on a handle without dead rows the call IS
 *     vdb_hip_index_search_batch(VDB_SEARCH_HNSW_INT8) at the same ef_search and ratio: ids, score bits, out_n, n_dist and n_expand;
 *   - for every id both routes return, route 1 and route 2 report identical score bits.
 * vdb_hip_index_last_search_stats: n_dist counts the int8 evaluations of a query's last walk attempt (re-scored rows are not
 * counted, as in mode 4) plus the rows its exact pass evaluated.
 * Errors, all checked before anything runs, the outputs untouched: oversampling_ratio > 64: VDB_ERR_INVALID_ARG; quantiser not
 * trained (vdb_hip_index_train_quantizer): VDB_ERR_STATE, as mode 4; Hamming / Jaccard handles, multi-device handles and
 * process-group members: VDB_ERR_UNSUPPORTED; a NULL table entry, a filter of another handle, a filter_of_query value > n_filters,
 * route outside 0..2: VDB_ERR_INVALID_ARG; a stale filter or no graph: VDB_ERR_STATE.  vdb_hip_index_last_kernels:
 * VDB_KERNEL_HNSW_FILTERED | VDB_KERNEL_HNSW_INT8 and / or VDB_KERNEL_FILTER_RANK.  The three calls above keep refusing mode 4. */
int32_t vdb_hip_index_search_graph_filters_int8(vdb_hip_index* idx, void** filters, uint32_t n_filters,
                                                const uint32_t* filter_of_query, const float* queries_rowmajor, uint32_t nq,
                                                uint32_t k, uint32_t ef_search, uint32_t oversampling_ratio, int32_t route,
                                                uint32_t max_list, uint64_t* out_ids, float* out_scores, uint32_t* out_n,
                                                uint32_t* out_route);
/* vdb_hip_index_search_graph_filters_half with EXACT F32 ANSWERS (hnsw_filtered.hip): the walk over the f16 / bf16 image,
 * the re-score of its best candidates over the f32 rows.  mode is VDB_SEARCH_HNSW_F16 or VDB_SEARCH_HNSW_BF16.  The contract is that of
 * vdb_hip_index_search_graph_filters_int8 with the half image in place of the u8 codes.  For one query: ef_s = ef_search, or the
 * Balanced rule max(128, 4k) when 0; ratio = oversampling_ratio, or 4 (DualPrecisionConfig::default) when 0 — the handle's
 * VDB_OPT_INT8_OVERSAMPLING is NOT read; cand_k = k * ratio; ef_w = max(ef_s, cand_k).  The walk is exactly that of
 * vdb_hip_index_search_graph_filters_half at ef = ef_w: the query rounded to the precision, every distance between the rounded query
 * and the row's image in mode C order with the Cosine EPSILON rule, the descent unfiltered, layer 0 the filtered search_layer
 * unchanged in every rule (the pivot, truncation, the overflow report, keys (distance, row)).  The first min(cand_k, results) allowed
 * entries are re-scored with the exact f32 engine distance between the UNROUNDED query and the f32 row — the distance the exact pass
 * gives that row —, stable-sorted by total_cmp (equal exact distances keep the coarse order) and cut to k; scores go through
 * transform_score; out_n = min(k, results); there is no post-drop, allowed means alive.  The exact pass (route 2, the plan's
 * whole-call cut, queries the largest list cannot hold) is the f32 one of vdb_hip_index_search_graph_filters, so a row has the same
 * score bits on either route.  The route plan, ladders, max_list, out_route, padding, "no filter" = n_filters and a query's
 * independence from its companions and its position are that call's, with ef_w where the plan takes ef.  The largest list follows
 * THIS launch's LDS layout, because the re-score output lies behind the lists: list keys [cap] u64 | neighbour ids [nbmax] u32 |
 * neighbour distances [nbmax] f32 | 16 control bytes | flags [cap rounded to 16] u8 | f32 query scratch (4 * dim rounded to 16 bytes,
 * only when dim is not 256 / 512 / 768 / 1024) | pad to 16 | re-score output [nbmax] u64, where nbmax = max(longest neighbour list,
 * cand_k) rounded up to 64; the largest list is the largest multiple of 64 entries for which this stays within 160 KB.
 * With n_filters = 0 the call is the plain dual-precision half search; there is no separate unfiltered kernel.
 * vdb_hip_index_last_search_stats: n_dist counts the half evaluations of a query's last walk attempt (re-scored rows are not
 * counted, as in mode 4) plus the rows its exact pass evaluated.
 * Errors, all checked before anything runs, the outputs untouched: mode other than VDB_SEARCH_HNSW_F16 / _BF16, Hamming / Jaccard
 * handles, multi-device handles and process-group members: VDB_ERR_UNSUPPORTED; oversampling_ratio > 64: VDB_ERR_INVALID_ARG; no
 * image of that precision (vdb_hip_index_enable_half_precision): VDB_ERR_STATE; a NULL table entry, a filter of another handle, a
 * filter_of_query value > n_filters, route outside 0..2: VDB_ERR_INVALID_ARG; a stale filter or no graph: VDB_ERR_STATE.  The k and
 * list limits are the int8 call's.  vdb_hip_index_last_kernels: VDB_KERNEL_HNSW_FILTERED | VDB_KERNEL_HNSW_HALF |
 * VDB_KERNEL_HALF_RESCORE (plus VDB_KERNEL_F16 for f16) and / or VDB_KERNEL_FILTER_RANK. */
int32_t vdb_hip_index_search_graph_filters_half_rescore(vdb_hip_index* idx, int32_t mode, void** filters, uint32_t n_filters,
                                                        const uint32_t* filter_of_query, const float* queries_rowmajor, uint32_t nq,
                                                        uint32_t k, uint32_t ef_search, uint32_t oversampling_ratio, int32_t route,
                                                        uint32_t max_list, uint64_t* out_ids, float* out_scores, uint32_t* out_n,
                                                        uint32_t* out_route);

/* ---- multi-query search with result fusion: Collection::multi_query_search / multi_query_search_ids (collection/search/batch.rs:
 * 206-403) and FusionStrategy::fuse (fusion/strategy.rs:138-300) on the device (fusion.hip, vdb_fusion.hpp) ----
 * The reference searches up to MAX_VECTORS = 10 reformulations of one user query at an over-fetched k (top_k 0-10: x 20, 11-50: x 10,
 * 51-100: x 5, larger: x 2; batch.rs:270-275), fuses the lists and keeps top_k.
 * The rule, for one group of V lists (list q = n_q records (id, score), best first):
 *   per (id, q): best_q = the maximum over the id's occurrences in list q, rank_q = the 0-based position of the first one;
 *   AVERAGE   the sum of best_q over the lists that hold the id (ascending q, a left fold from the first term) / (float)count;
 *   MAXIMUM   the maximum over all occurrences;
 *   RRF       0.0f + the sum over those lists of 1.0f / ((float)rrf_k + (float)(rank_q + 1)), ascending q;
 *   WEIGHTED  (avg_w * avg + max_w * mx) + hit_w * ((float)count / (float)V), every operation rounded on its own; V counts empty lists.
 * Result: descending by the IEEE total order of the fused score, EQUAL SCORES BY ID ASCENDING (the reference leaves ties to HashMap
 * iteration: any tie order is one of its outputs, this one is fixed).  WEIGHTED weights: any weight < 0, a sum off 1.0 by more than
 * 0.001 (in f32) and NaN weights are VDB_ERR_INVALID_ARG (the reference's weighted() lets NaN through).  NaN scores and an id whose
 * scores mix +0.0 and -0.0 are outside the contract (resolved by total order). */
enum vdb_fusion_strategy { VDB_FUSION_AVERAGE = 0, VDB_FUSION_MAXIMUM = 1, VDB_FUSION_RRF = 2, VDB_FUSION_WEIGHTED = 3 };
/* FusionStrategy::fuse for n_groups independent groups in ONE launch (one block per group), host pointers.  Lists are
 * [n_lists][list_stride]; list j holds list_n[j] <= list_stride records; consecutive lists form the groups: group g = the next
 * group_sizes[g] lists (0 and more than 10 are legal here: fuse has no limit); the sizes must sum to n_lists.  weights = [3] avg, max,
 * hit (VDB_FUSION_WEIGHTED only, else ignored, nullable); rrf_k: VDB_FUSION_RRF only (the reference's default is 60).
 * Outputs [n_groups][max(top_k, 1)] / out_n [n_groups]: the first min(top_k, distinct ids) fused records, padded as the search calls
 * pad (id ~0, score NaN); top_k = 0: out_n = 0, nothing else written.  A group of more than 8192 records (what one block's LDS
 * takes, 128 of 160 KB) answers VDB_ERR_UNSUPPORTED before anything runs; a size sum != n_lists, list_n[j] > list_stride, a null
 * pointer, a strategy outside 0..3, invalid weights: VDB_ERR_INVALID_ARG.  The outputs are untouched on error. */
int32_t vdb_hip_fuse_results(int32_t device, int32_t strategy, uint32_t rrf_k, const float* weights, const uint64_t* ids,
                             const float* scores, const uint32_t* list_n, uint32_t n_lists, uint32_t list_stride,
                             const uint32_t* group_sizes, uint32_t n_groups, uint32_t top_k, uint64_t* out_ids, float* out_scores,
                             uint32_t* out_n);
/* multi_query_search_ids for n_groups user queries in one call: queries_rowmajor holds the vectors of group 0, then of group 1, ...;
 * group_sizes[g] in 1..10 (VDB_ERR_INVALID_ARG otherwise, the message names the group); n_groups = 0 is VDB_OK.
 * THE CONTRACT: group g gets, bit for bit, the rule above applied to
 *   filter == NULL: the lists vdb_hip_index_search_batch(mode = VDB_SEARCH_HNSW, ef = 0, k = overfetch(top_k)) returns for its vectors
 *     (search_batch_parallel with SearchQuality::Balanced is what the reference calls);
 *   filter != NULL: the lists vdb_hip_index_search_graph_filtered(filter, k = overfetch(top_k), ef = 0, route 0, max_list 0) returns —
 *     the in-walk allow-list of DESIGN 4.1h: rows the filter rejects never take a place in a list.  The reference POST-filters the
 *     over-fetched lists instead (batch.rs:283-302), so a selective filter leaves it fewer candidates than it leaves this call.
 * Scores are the FUSED scores, sorted descending whatever the metric, as the reference sorts them: AVERAGE / MAXIMUM / WEIGHTED over
 * a distance metric (Euclidean, Hamming: smaller = better) therefore rank the worst first — the reference's behaviour, inherited;
 * RRF uses ranks only and is the metric-agnostic default (FusionStrategy::default()).
 * A group's answer never depends on its companions or on its position in the call.  Outputs as vdb_hip_fuse_results.  A group of
 * V vectors with V * overfetch(top_k) > 8192 answers VDB_ERR_UNSUPPORTED before anything runs (top_k <= 409 is always served);
 * every other limit or error of the per-query call it stands on is passed through (no graph: VDB_ERR_STATE; a filter of another handle:
 * VDB_ERR_INVALID_ARG; a stale filter: VDB_ERR_STATE).  Multi-device handles and process-group members: VDB_ERR_UNSUPPORTED.  The
 * outputs are untouched on error.  Host pointers; launches of its own on one leased search context (no combining front): the walks,
 * then fuse_lists_kernel over the context's result lists on the same stream — only the fused block comes back.
 * vdb_hip_index_last_kernels: VDB_KERNEL_FUSE next to the walk's bits. */
int32_t vdb_hip_index_multi_query_search(vdb_hip_index* idx, const void* filter, const float* queries_rowmajor,
                                         const uint32_t* group_sizes, uint32_t n_groups, uint32_t top_k, int32_t strategy,
                                         uint32_t rrf_k, const float* weights, uint64_t* out_ids, float* out_scores, uint32_t* out_n);

/* ---- hybrid search: Collection::hybrid_search / hybrid_search_with_filter (collection/search/text.rs:113-299) — one vector query
 * plus the hits of one BM25 text query, fused by a weighted Reciprocal Rank Fusion on the device (hybrid.hip, vdb_hybrid.hpp;
 * DESIGN 4.1p).  The BM25 index stays the caller's, as payload predicates do: the caller runs its text search and hands over the ids,
 * best first.  The rule uses ranks only, so no entry point takes scores.
 * The rule, for one user query with a vector list V, a text list T (ids, best first) and a vector_weight:
 *   w = clamp(vector_weight, 0, 1) in f32 (default 0.5f), tw = 1.0f - w;
 *   score(id) = 0.0f, + w / ((float)r + 60.0f) for EVERY occurrence of the id at 0-based position r of V in ascending r, then
 *               + tw / ((float)r + 60.0f) for every occurrence at position r of T in ascending r, every operation rounded on its own
 *               (no in-list de-duplication: the reference has none here, unlike FusionStrategy::fuse);
 *   one sort key: the fused score descending by the IEEE total order, EQUAL SCORES BY ID DESCENDING; the first k ids under it are the
 *   result.  Membership at the cut is the reference's (its heap pops the smallest (score, id), text.rs:166-173); the order among
 *   equal scores is unspecified there and fixed here.  This is NOT the tie rule of vdb_hip_fuse_results (id ascending), on purpose.
 * Deviation: a NaN weight is VDB_ERR_INVALID_ARG (Rust's clamp lets NaN through and the reference then returns NaN scores).
 *
 * vdb_hip_hybrid_fuse: the rule alone over nq caller list pairs in ONE launch (one block per query), every id treated as live, no
 * filter; host pointers.  vec_ids [nq][vec_stride] / text_ids [nq][text_stride], query i holds vec_n[i] <= vec_stride and
 * text_n[i] <= text_stride ids; vector_weights [nq], NULL = 0.5 for all.  Outputs [nq][max(k, 1)] / out_n [nq]: the first
 * min(k, distinct ids) fused records, padded as the search calls pad (id ~0, score NaN); k = 0: out_n = 0, nothing else written;
 * nq = 0: VDB_OK.  A query with vec_n[i] + text_n[i] > 8192 (what one block's LDS takes, 128 of 160 KB) answers
 * VDB_ERR_UNSUPPORTED before anything runs (the message names the query); a list longer than its stride, a null pointer, a NaN weight:
 * VDB_ERR_INVALID_ARG.  The outputs are untouched on error. */
int32_t vdb_hip_hybrid_fuse(int32_t device, const uint64_t* vec_ids, const uint32_t* vec_n, uint32_t vec_stride,
                            const uint64_t* text_ids, const uint32_t* text_n, uint32_t text_stride, const float* vector_weights,
                            uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
/* hybrid_search / hybrid_search_with_filter for nq user queries in one call: queries_rowmajor [nq][dim]; text_ids / text_n /
 * text_stride / vector_weights / outputs as above.
 * THE CONTRACT: query i gets, bit for bit, the rule above applied to its text ids and to
 *   filter == NULL: the list vdb_hip_index_search_batch(mode = VDB_SEARCH_HNSW, ef = 0, k' = 2k) returns for it.  A text id the handle
 *     does not know, or whose row is removed, takes its rank, its score and its place in the cut and is then dropped from the output
 *     (the reference's filter_map over the vector storage BEHIND the cut, text.rs:186-200): out_n can be below min(k, distinct ids);
 *   filter != NULL: the list vdb_hip_index_search_graph_filtered(filter, k' = max(4k, k + 10), ef = 0, route 0, max_list 0) returns
 *     for it — the in-walk allow-list of DESIGN 4.1h — and text hits whose row is unknown, removed or outside the filter are dropped
 *     BEFORE ranks are assigned (a stable compaction).  Deviation: the reference ranks, fuses, sorts, post-filters and takes k
 *     (text.rs:244-296), so a selective filter leaves it short; this form does not come back short while allowed candidates exist.
 * The text ids are mapped through the handle's id map under the handle's lock, as vdb_hip_index_filter_create maps ids; the live
 * flags are read at search time.  A query's answer never depends on its companions or on its position in the call.
 * k' + text_n[i] > 8192 answers VDB_ERR_UNSUPPORTED before anything runs (the message names the query); a NaN weight, a null
 * pointer, text_n[i] > text_stride: VDB_ERR_INVALID_ARG; every other limit or error of the per-query call it stands on is passed
 * through (no graph: VDB_ERR_STATE; a filter of another handle: VDB_ERR_INVALID_ARG; a stale filter: VDB_ERR_STATE).  Multi-device
 * handles and process-group members: VDB_ERR_UNSUPPORTED.  The outputs are untouched on error.  Host pointers; launches of its own
 * on one leased search context (no combining front): the walks — the per-query call's own code, which still brings its whole result
 * block (nq x k' records and the counts) to pinned host memory and synchronises —, then hybrid_fuse_kernel over the context's DEVICE
 * copy of the lists on the same stream, the nq x k fused records back and a second synchronisation.  What the call saves a caller is
 * the copy of nq x k' records into its arrays and the hashing and sorting there, not that transfer.
 * vdb_hip_index_last_kernels: VDB_KERNEL_HYBRID_FUSE next to the walk's bits. */
int32_t vdb_hip_index_hybrid_search(vdb_hip_index* idx, const void* filter, const float* queries_rowmajor, uint32_t nq, uint32_t k,
                                    const uint64_t* text_ids, const uint32_t* text_n, uint32_t text_stride,
                                    const float* vector_weights, uint64_t* out_ids, float* out_scores, uint32_t* out_n);

/* ---- the two fused searches over every form of the walk, with one optional filter PER QUERY ----
 * rows: what the walk's distances are taken over — the f32 rows, the f16 / bf16 image (vdb_hip_index_enable_half_precision first),
 * the u8 codes with the f32 re-score (vdb_hip_index_train_quantizer first), or a half image with the f32 re-score.
 * oversampling_ratio is read for VDB_WALK_ROWS_INT8 (0 = the handle's option) and the two _RESCORE forms (0 = 4) only; there a value
 * above 64 is VDB_ERR_INVALID_ARG.  ef is 0 (SearchQuality::Balanced) throughout, as in the two calls above.
 * The filter table is vdb_hip_index_search_graph_filters': filters[n_filters] handles, filter_of_query[i] in 0..n_filters, the value
 * n_filters = no filter; n_filters = 0 with filters = NULL is legal. */
enum vdb_walk_rows { VDB_WALK_ROWS_F32 = 0, VDB_WALK_ROWS_F16 = 1, VDB_WALK_ROWS_BF16 = 2, VDB_WALK_ROWS_INT8 = 3,
                     VDB_WALK_ROWS_F16_RESCORE = 4, VDB_WALK_ROWS_BF16_RESCORE = 5 };
/* vdb_hip_index_hybrid_search for nq user queries, each with its own filter or none.  THE CONTRACT: query i gets, bit for bit, the
 * rule of vdb_hip_hybrid_fuse applied to its text ids and to
 *   no filter: the list the plain call of the rows form returns for it alone at k' = 2k — vdb_hip_index_search_batch with mode
 *     VDB_SEARCH_HNSW / _HNSW_F16 / _HNSW_BF16 / _HNSW_INT8 (with a ratio of the call's own: vdb_hip_index_search_with_config at
 *     ef_search 0, that ratio, int8 traversal, min_index_size 0), for the _RESCORE forms
 *     vdb_hip_index_search_graph_filters_half_rescore with n_filters = 0.  Unknown or removed text ids take their rank and their
 *     place in the cut and are dropped behind it, as in vdb_hip_index_hybrid_search;
 *   a filter: the list the call with one filter per query of the rows form returns for it alone at k' = max(4k, k + 10), route 0,
 *     max_list 0 — vdb_hip_index_search_graph_filters / _half / _int8 / _half_rescore — and text hits that are unknown, removed or
 *     outside ITS filter are compacted away before ranks exist.  A query with an empty filter gets out_n = 0.
 * A query's answer never depends on its companions or on its position.  With VDB_WALK_ROWS_F32 and no query filtered the call is
 * vdb_hip_index_hybrid_search(filter = NULL) byte for byte, with every query on the same filter vdb_hip_index_hybrid_search(filter).
 * Everything below is decided before anything runs, and the outputs stay untouched: rows outside 0..5, a ratio above 64, a NULL
 * table entry, a filter of another handle, a table value above n_filters, a NaN weight, text_n[i] > text_stride, a null pointer:
 * VDB_ERR_INVALID_ARG; the image of the rows form not enabled, the quantiser not trained, no graph, a stale filter: VDB_ERR_STATE; a
 * Hamming / Jaccard handle with rows other than VDB_WALK_ROWS_F32, a multi-device handle, a member of a process group, a query whose
 * OWN k' plus text_n[i] exceeds 8192 (the message names the query): VDB_ERR_UNSUPPORTED.
 * One lease, two phases: the unfiltered queries are walked at 2k and fused into their output rows, then the filtered ones at
 * max(4k, k + 10) (hybrid_fuse_filters_kernel reads every query's own filter); a phase without queries launches nothing; one copy
 * back and one synchronisation behind the last fusion.  vdb_hip_index_last_kernels: the bits of both walks and
 * VDB_KERNEL_HYBRID_FUSE; vdb_hip_index_last_search_stats: the sum over both walks. */
int32_t vdb_hip_index_hybrid_search_filters(vdb_hip_index* idx, int32_t rows, uint32_t oversampling_ratio, void** filters,
                                            uint32_t n_filters, const uint32_t* filter_of_query, const float* queries_rowmajor,
                                            uint32_t nq, uint32_t k, const uint64_t* text_ids, const uint32_t* text_n,
                                            uint32_t text_stride, const float* vector_weights, uint64_t* out_ids, float* out_scores,
                                            uint32_t* out_n);
/* vdb_hip_index_multi_query_search for n_groups user queries, each GROUP with its own filter or none (filter_of_group [n_groups]).
 * The same contract per group, both kinds at k' = overfetch(top_k): an unfiltered group's lists are the plain call's of the rows form
 * (removed rows never enter a walk's list), a filtered group's the lists of the call with one filter per query, every vector of the
 * group on the group's filter.  The rule, its tie order, the group-size limits and the outputs are vdb_hip_index_multi_query_search's;
 * with VDB_WALK_ROWS_F32 and no filter or one shared filter the call is that call byte for byte.  Errors as above (a group of V
 * vectors with V * overfetch(top_k) > 8192: VDB_ERR_UNSUPPORTED, the message names the group).  fuse_lists_kernel is unchanged: a
 * phase's groups are fused into consecutive rows of one block and handed out on the host.
 * vdb_hip_index_last_kernels: the bits of both walks and VDB_KERNEL_FUSE. */
int32_t vdb_hip_index_multi_query_search_filters(vdb_hip_index* idx, int32_t rows, uint32_t oversampling_ratio, void** filters,
                                                 uint32_t n_filters, const uint32_t* filter_of_group, const float* queries_rowmajor,
                                                 const uint32_t* group_sizes, uint32_t n_groups, uint32_t top_k, int32_t strategy,
                                                 uint32_t rrf_k, const float* weights, uint64_t* out_ids, float* out_scores,
                                                 uint32_t* out_n);

/* ---- DistanceEngine::batch_distance / GpuAccelerator::batch_{cosine_similarity,
 * euclidean_distance,dot_product} (native/distance.rs:21-24; gpu_backend.rs:157,355,397) ----
 * n rows of dim floats against one query; out has n floats, same order as the rows. */
int32_t vdb_hip_batch_distance(int32_t device, int32_t metric, int32_t kind, const float* query,
                               const float* vecs_rowmajor, uint64_t n, uint32_t dim, float* out);
int32_t vdb_hip_batch_distance_dev(int32_t metric, int32_t kind, const float* d_query,
                                   const float* d_vecs_rowmajor, uint64_t n, uint32_t dim, float* d_out,
                                   void* stream);

/* ---- the other free functions of the reference's SIMD module on the path, n vectors per call
 * (host pointers, row-major; vec_utils.hip) ---- */
/* simd::norm / simd_explicit::norm_simd (simd.rs:240-242; simd_explicit.rs:194-215): out[i] = |vecs[i]| */
int32_t vdb_hip_batch_norm(int32_t device, const float* vecs_rowmajor, uint64_t n, uint32_t dim, float* out);
/* simd::normalize_inplace (simd.rs:217-219; simd_explicit.rs:638-664): rows scaled to unit length in place; a zero
 * vector stays as it is */
int32_t vdb_hip_normalize_rows(int32_t device, float* vecs_rowmajor, uint64_t n, uint32_t dim);
/* simd_explicit::batch_dot_product (simd_explicit.rs:519-560): out[i * n + j] = dot(queries[i], vecs[j]) */
int32_t vdb_hip_batch_dot_product(int32_t device, const float* queries_rowmajor, uint32_t nq, const float* vecs_rowmajor,
                                  uint64_t n, uint32_t dim, float* out);
/* hamming_distance_binary(_fast) / jaccard_similarity_binary over packed u64 words (simd_explicit.rs:308-360,457-500):
 * one query of `words` u64 against n rows of `words` u64 */
int32_t vdb_hip_batch_hamming_binary(int32_t device, const uint64_t* query_words, const uint64_t* rows_words, uint64_t n,
                                     uint32_t words, uint32_t* out);
int32_t vdb_hip_batch_jaccard_binary(int32_t device, const uint64_t* query_words, const uint64_t* rows_words, uint64_t n,
                                     uint32_t words, float* out);

/* ---- persistence hand-off: NativeHnsw::file_dump / file_load, format v1
 * (native/backend_adapter.rs:184-381): <dir>/<basename>.vectors and .graph ---- */
int32_t vdb_hip_index_load_reference_files(vdb_hip_index* idx, const char* dir, const char* basename);
int32_t vdb_hip_index_save_reference_files(vdb_hip_index* idx, const char* dir, const char* basename);

/* HnswIndex::save / HnswIndex::load (index/hnsw/index/constructors.rs:190-287): a directory holding
 * native_hnsw.{vectors,graph} (above), native_mappings.bin (bincode 1.3.3: id_to_idx map, idx_to_id map, next_idx) and
 * native_meta.bin (bincode: dimension, metric, enable_vector_storage) — what a VelesDB collection keeps on disk for its
 * HNSW index.  load_dir creates the index (dimension / metric from the meta file, M / ef_construction from the graph
 * file, ids from the mappings; ids the reference removed are absent from the mappings and come back soft-deleted). */
int32_t vdb_hip_index_save_dir(vdb_hip_index* idx, const char* dir);
int32_t vdb_hip_index_load_dir(const char* dir, int32_t device, vdb_hip_index** out);
/* A flushed MmapStorage directory (core/storage/mmap.rs:96-160,402-455,602-626: vectors.idx = bincode
 * FxHashMap<u64 id, usize byte offset>, vectors.dat = raw f32 at those offsets) as an upload source: every vector
 * the store's index names is uploaded (no graph, as vdb_hip_index_upload) in ascending byte offset, i.e. in the order
 * the store first saw the ids.  The index's dimension must be the store's.  Ids already present are skipped.
 * VDB_ERR_IO: missing / truncated files, an offset past the end of vectors.dat ("Offset out of bounds", :563-568). */
int32_t vdb_hip_index_upload_vector_store(vdb_hip_index* idx, const char* dir, uint64_t* inserted);

/* ---- tuning options ----
 * Every option has a process-wide default (vdb_hip_set_* below) and a per-handle value: a handle follows the default until
 * vdb_hip_index_set_option gives it its own (value < 0: follow the default again).  A multi-device handle passes the option to
 * every shard.  Results never depend on an option. */
enum vdb_option {
  VDB_OPT_MAX_QUERY_TILE = 0,   /* vdb_hip_set_max_query_tile    */
  VDB_OPT_SWEEP_ENGINE = 1,     /* vdb_hip_set_sweep_engine      */
  VDB_OPT_SELECTOR_LEVEL = 2,   /* vdb_hip_set_split_selector    */
  VDB_OPT_INT8_OVERSAMPLING = 3,/* vdb_hip_set_int8_oversampling */
  VDB_OPT_KERNEL_TIMING = 4,    /* vdb_hip_set_kernel_timing     */
  /* The combining front of the host-pointer search entry points (vdb_hip_index_search / _search_batch / _search_rerank).  The
   * reference serves many threads that each search ONE query under a read lock (index/hnsw/index/search.rs:80; the server calls
   * collection.search once per request); a GPU serves that pattern at its own rate only when callers that arrive together share
   * a launch.  Calls of <= 64 queries queue up; one of the waiting callers becomes the leader, gathers the queued calls with the
   * same (k, ef, mode, rerank_k) into one batch of <= COMBINE_MAX_BATCH queries (default 256; 0 = every call launches alone),
   * runs it and hands every caller its slice.  At most COMBINE_INFLIGHT batches run at a time (default 0 = by kind of search:
   * two for graph walks — latency-bound, one CU per query, two launches overlap for free — and one for sweeps: an HBM-bound
   * pass gains nothing from a second launch beside it, and callers that split into groups wait for each other).  Batches
   * form from the calls that arrive while the launch in front of them runs; a leader that has evidence of company (the batch
   * that finished last carried several calls) waits until as many calls have arrived as that batch had callers, at most
   * COMBINE_WINDOW_US microseconds (default 100; 0 = never wait).  A lone caller is never delayed.
   * Results are per-query independent: bits do not depend on the batch a call lands in. */
  VDB_OPT_COMBINE_MAX_BATCH = 5,
  VDB_OPT_COMBINE_WINDOW_US = 6,
  VDB_OPT_COMBINE_INFLIGHT = 7,
  /* route of vdb_hip_index_search_batch_filtered: <= 0 = auto (the rule stated there), 1 = the listed sweep wherever the metric has
   * it, 2 = mask substitution.  Like every option it never changes a result. */
  VDB_OPT_FILTER_ROUTE = 8,
  VDB_OPT_COUNT_ = 9
};
int32_t vdb_hip_index_set_option(vdb_hip_index* idx, int32_t option, int64_t value);
int32_t vdb_hip_index_get_option(vdb_hip_index* idx, int32_t option, int64_t* value); /* the effective value */

/* counters of the combining front since the handle was created: launches it issued, calls and queries they carried, the largest
 * batch (queries) — calls / launches is the average number of callers that shared a launch */
int32_t vdb_hip_index_combine_stats(vdb_hip_index* idx, uint64_t* launches, uint64_t* calls, uint64_t* queries,
                                    uint64_t* max_batch);

/* ---- introspection used by tests and the bench ---- */
/* neighbours of `node` on `layer`; returns count in *n, writes up to cap ids */
int32_t vdb_hip_index_get_neighbors(vdb_hip_index* idx, uint32_t layer, uint64_t node, uint32_t* out,
                                    uint32_t cap, uint32_t* n);
int32_t vdb_hip_index_graph_info(vdb_hip_index* idx, uint32_t* num_layers, uint32_t* max_layer,
                                 int64_t* entry_point);
/* counters of graph CONSTRUCTION (NativeHnsw::insert, graph.rs:158-237, with select_neighbors :526-581), cumulative since the
 * handle was created: rows whose distance to the inserted node (search_layer at ef_construction) or to a selected neighbour
 * (select_neighbors) was evaluated — the algorithmic gather traffic of the build is that x dim x 4 bytes —, the number of
 * distance phases (dependent memory round trips), the nodes inserted, and how many of the evaluated rows were select_neighbors
 * evaluations (the <= ef_construction candidate rows of a node re-read once per selected neighbour: cache hits, not HBM traffic).
 * Synchronises the device. */
int32_t vdb_hip_index_build_stats(vdb_hip_index* idx, uint64_t* rows_evaluated, uint64_t* distance_phases, uint64_t* nodes,
                                  uint64_t* select_rows);
/* counters of the last HNSW search batch: distance evaluations and expansions.
 * NOTE for every vdb_hip_index_last_* diagnostic below: with the combining front on (VDB_OPT_COMBINE_MAX_BATCH > 1, the default)
 * a host-pointer call of <= 64 queries may have travelled in ONE launch with other callers' requests; the diagnostics then describe
 * that whole combined launch (all its queries), not the caller's own call, and the next batch served by the same search context may
 * overwrite them before they are read.  A caller that wants per-call numbers sets VDB_OPT_COMBINE_MAX_BATCH to 0 on the handle
 * (bench.py reads them after single-threaded calls only). */
int32_t vdb_hip_index_last_search_stats(vdb_hip_index* idx, uint64_t* n_dist, uint64_t* n_expand);
/* of the last HNSW search batch's expansions: how many found their neighbour list already requested — the walk kernel asks for the
 * list of the nearest candidate it leaves unexpanded together with the list of the one it expands (the predicted next pop); a measure
 * of the prediction, not a count the reference has */
int32_t vdb_hip_index_last_prefetch_hits(vdb_hip_index* idx, uint64_t* hits);
/* average duration (ms) of the dominant kernel in the last search call, measured with HIP
 * events on the launch stream; 0 if timing is off.  Enable with vdb_hip_set_kernel_timing(1) — for measurements only: an event
 * record idles the GPU ~6 us on either side of the launch it brackets (a 1 024-query exact batch brackets four selection launches
 * and itself: ~50 us of a 1.7 ms batch). */
int32_t vdb_hip_set_kernel_timing(int32_t on);
/* tuning knob of the exact sweep: largest number of queries served by one corpus pass
 * (vector-ALU kernels: 1,2,4,8 register-resident tiles, 16,32 LDS-resident tiles; matrix-core streaming kernel:
 * 16, 32 or 48 queries; 128 = batches of >= 64 queries go to the GEMM-structured matrix-core kernel, up to 128
 * queries per block tile).  Default 128.  Results do not depend on it. */
int32_t vdb_hip_set_max_query_tile(uint32_t b);
/* arithmetic engine of the exact sweep for Cosine / DotProduct: 1 (default) = matrix-core kernel
 * (v_mfma_f32_16x16x4_f32: exact f32, one k-ordered fmaf chain per pair, oracle mode M); 0 = vector-ALU kernels
 * (canonical lane-chain order, oracle mode C — what Euclidean, the graph kernels and batch_distance always use).
 * Both are exact f32 arithmetic; scores differ in the last bits because the summation order does.  The choice
 * never depends on the batch size. */
int32_t vdb_hip_set_sweep_engine(int32_t engine);
/* Exact Cosine / DotProduct (and Euclidean, SQ8) batches of >= 16 queries, up to 1 024 per pass (round 2: 80 .. 256, or more that filled 256-query tiles to 7/8)
 * (k <= 10, >= 65 536 rows, dim % 32 == 0):
 * the matrix cores SELECT candidates on a reduced-precision image of rows and queries, the best candidates per query are
 * re-scored with the exact chain (oracle mode M), and every query's answer is PROVEN from an error bound or recomputed by
 * the exact kernel — same ids, ranks and score bits as the exact f32 matrix-core kernel for the whole batch.
 *   0 = no selection stage: the exact f32 matrix-core kernel;
 *   1 = split-bf16 selection (x = hi + lo, three bf16 MFMAs per product, error ~2^-15 + accumulation; 32 candidates);
 *       costs +4 bytes per element of HBM (the split image, built at first use);
 *   2 = plain bf16 selection first (one MFMA per product over the bf16 copy of the rows, error ~2^-7; 64
 *       candidates; +2 bytes per element, dim % 64 == 0), level 1 where that does not apply; a handle whose data defeats
 *       the wider bound (> 1/16 of a batch unproven: near-duplicate clusters) moves itself to level 1 for the next 64
 *       batches and then tries again.  Cosine (round 6): the image holds the NORMALISED rows v / |v| and the batch the
 *       normalised queries, so the selection is a DotProduct of unit vectors (no row norm in the kernel's bound).
 * 10 < k <= 128 (round 6; Cosine / DotProduct / Euclidean, level 2's eligibility): the WIDE selection — no block-local top-k at all:
 * every row whose approximate score passes the query's bound (k-th best approximate score seen so far - 2 x the error
 * bound, raised between the launches of the batch) becomes a candidate, all of them are re-scored exactly; a query is
 * unproven only when its candidate list overflows (4 096 per launch, 1 024 at the end) or its data is not finite.
 * Reported as level 4 by vdb_hip_index_last_select_level.  Larger k, other metrics at k > 10: the exact kernels.
 *   3 (default since round 6) = level 2, and Cosine / DotProduct / Euclidean batches over f32 rows and Cosine / DotProduct batches of the
 *       SQ8 storage mode take the WIDE selection at EVERY k <= 128 (k <= 10 included: faster than the block-local lists, ~30 instead
 *       of 64 rows to re-score); a handle with > 1/16 of a batch unproven there answers its next 64 batches by level 2's rules. */
int32_t vdb_hip_set_split_selector(int32_t level);
/* diagnostic: queries in the last split-selector batch (its last chunk of <= 1024) and how many of them the exact
 * fallback kernel answered because the selection could not be proven (near-ties inside the error bound, non-finite data) */
int32_t vdb_hip_index_last_split_stats(vdb_hip_index* idx, uint32_t* queries, uint32_t* unproven);
/* selection level (0 / 1 / 2; 3 = the SQ8 storage mode's block-local form; 4 = the WIDE selection; see vdb_hip_set_split_selector) the last
 * exact batch of this handle actually ran at */
int32_t vdb_hip_index_last_select_level(vdb_hip_index* idx, int32_t* level);
/* which kernel families served the last search call of this handle (a bit set; what a test asserts when it claims to have
 * driven a particular kernel — e.g. BASELINE configs[3] is VDB_KERNEL_GEMM_BF16_GLDS, which needs >= 65 536 rows) */
enum vdb_kernel_bit {
  VDB_KERNEL_SWEEP_VALU = 1,       /* sweep_topk_f32 / sweep_topk_f32_qlds (vector ALU, mode C)                       */
  VDB_KERNEL_SWEEP_MFMA_F32 = 2,   /* sweep_topk_mfma_f32 (streaming, <= 48 queries per corpus pass, mode M)           */
  VDB_KERNEL_GEMM_F32 = 4,         /* sweep_topk_gemm_f32 (GEMM-structured exact f32; also the selection stage's seed) */
  VDB_KERNEL_SWEEP_MFMA_BF16 = 8,  /* sweep_topk_mfma_bf16 (streaming over the bf16 rows, <= 96 queries per pass)      */
  VDB_KERNEL_GEMM_BF16 = 16,       /* register-staged bf16 GEMM kernels of sweep_gemm.hip (128 x 128 / 256 x 256)      */
  VDB_KERNEL_GEMM_BF16_GLDS = 32,  /* sweep_topk_gemm_bf16_glds reporting bf16 RESULTS (VDB_SEARCH_BRUTE_BF16)         */
  VDB_KERNEL_SELECT_BF16 = 64,     /* the same kernel as the selection stage of an exact / SQ8 batch (levels 2, 3)     */
  VDB_KERNEL_SELECT_SPLIT = 128,   /* ... its split-bf16 instance (level 1)                                            */
  VDB_KERNEL_BITS = 256,           /* packed-bit sweeps (Hamming / Jaccard / sign-bit codes)                           */
  VDB_KERNEL_SQ8 = 512,            /* sweep_topk_sq8                                                                   */
  VDB_KERNEL_HNSW = 1024,          /* hnsw_search_kernel                                                               */
  VDB_KERNEL_HNSW_INT8 = 2048,     /* hnsw_search_int8_kernel                                                          */
  VDB_KERNEL_BITS_GEMM = 4096,     /* Hamming / Jaccard batches as a four-bit GEMM distance (sweep_topk_gemm_bf16_pp<.., FP4>) */
  VDB_KERNEL_F16 = 8192,           /* an IEEE f16 instance of a matrix-core family ran (VDB_SEARCH_BRUTE_F16): set NEXT TO the family's
                                      bit — SWEEP_MFMA_BF16 / GEMM_BF16 / GEMM_BF16_GLDS then name the f16 instance of that kernel      */
  VDB_KERNEL_SWEEP_HALF_L2 = 16384, /* sweep_topk_half_l2 (Euclidean difference chain over the f16 / bf16 rows)                       */
  VDB_KERNEL_HNSW_HALF = 32768,    /* hnsw_search_half_kernel (VDB_SEARCH_HNSW_F16 / _BF16; VDB_KERNEL_F16 next to it for the f16 instance) */
  VDB_KERNEL_SWEEP_LISTED = 65536, /* sweep_topk_listed / sweep_topk_listed_m (vdb_hip_index_search_batch_filtered, the listed route) */
  VDB_KERNEL_HNSW_FILTERED = 131072, /* hnsw_search_filters_kernel (vdb_hip_index_search_graph_filtered / _filters, the walk)            */
  VDB_KERNEL_FILTER_RANK = 262144  /* filters_rank_kernel (vdb_hip_index_search_graph_filtered / _filters, the exact pass)             */
};
/* one more bit of the same mask: fuse_lists_kernel ran (vdb_hip_index_multi_query_search sets it next to the walk's bits).  A macro
 * beside the enum, not an enumerator: tests/test_filters_graph_cpu.py pins VDB_KERNEL_FILTER_RANK as the enum's last member. */
#define VDB_KERNEL_FUSE 524288
/* ... and one more, for the same reason a macro: hnsw_search_filters_half_rescore_kernel ran (vdb_hip_index_search_graph_filters_half_rescore,
 * the walk; next to VDB_KERNEL_HNSW_FILTERED | VDB_KERNEL_HNSW_HALF) */
#define VDB_KERNEL_HALF_RESCORE 1048576
/* ... and one more: sweep_topk_listed_groups / sweep_topk_listed_groups_m ran (vdb_hip_index_search_batch_filters, the grouped
 * launches of its groups on the listed route), or sweep_topk_sq8_listed_groups / sweep_topk_half_l2_listed_groups
 * (vdb_hip_index_search_batch_filters_mode, the same over the SQ8 codes / Euclidean over a half image) */
#define VDB_KERNEL_SWEEP_LISTED_GROUPS 2097152
/* ... and one more: hybrid_fuse_kernel ran (vdb_hip_index_hybrid_search sets it next to the walk's bits) */
#define VDB_KERNEL_HYBRID_FUSE 4194304
/* which kernels served THIS THREAD's last search on the handle: taken when that search's context was released (or, for a call the
 * combining front had another thread launch, handed back with the call's result), so a search of another thread that takes the same
 * context a moment later does not change it. */
int32_t vdb_hip_index_last_kernels(vdb_hip_index* idx, uint32_t* mask);
/* *mode = 1 if searches in VDB_SEARCH_BRUTE mode with this k run on the matrix-core kernel (mode M), else 0 */
int32_t vdb_hip_index_sweep_arith_mode(vdb_hip_index* idx, uint32_t k, int32_t* mode);
int32_t vdb_hip_index_last_kernel_ms(vdb_hip_index* idx, float* ms, uint32_t* launches);
/* with kernel timing on: the launches of the selection kernel (sweep_topk_gemm_bf16_glds) in the last search call — their
 * number and the SUM of their durations in ms (HIP events around each launch); 0 / 0 when the call had no selection stage */
int32_t vdb_hip_index_last_selection_ms(vdb_hip_index* idx, float* total_ms, uint32_t* launches);

const char* vdb_hip_last_error(void); /* thread-local, never NULL */
const char* vdb_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VELESDB_HIP_H */
