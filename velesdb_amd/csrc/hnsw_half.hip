// hnsw_half.hip — graph search over the half-precision image of the rows (VDB_SEARCH_HNSW_F16 / VDB_SEARCH_HNSW_BF16):
// NativeHnsw::search (native/graph.rs:251-270) over the handle's existing graph under HnswIndex's result mapping, exactly as
// VDB_SEARCH_HNSW — the walk IS hnsw_walk_body (vdb_hnsw_device.hpp), the text the f32 kernel runs — with every distance taken
// between the query rounded to the precision (VectorData::from_f32_slice, half_precision.rs:94-101) and the row's f16 / bf16
// image (enable_half_precision): half_precision::dot_product / cosine_similarity / euclidean_distance (half_precision.rs:199-287).
//
// Declared summation order: mode C of vdb_device.hpp, unchanged (dist_phase_half).  Over image H the walk is therefore bit for bit
// the f32 walk over the f32 rows dequant(H) with the rounded query (DotProduct and Euclidean on any data; Cosine differs only in
// the reference's own rule for tiny norms, `< f32::EPSILON` instead of `== 0`), and the oracle's mode-C graph search is its
// reference.  A visited node costs 2 * stride bytes (+ 4 for the Cosine norm) instead of 4 * stride:
// algorithmic HBM bytes per query = n_dist * (2 * stride [+ 4]) + n_expand * M0 * 4.
//
// Instances: the throughput form only (256-thread blocks, four walks per CU, HBM visited bitmaps); small calls take it too.
#include <algorithm>

#include "vdb_hnsw_device.hpp"
#include "vdb_index.hpp"
#include "vdb_walk_launch.hpp"

namespace vdb {

// (.., 4): 128 registers, four walks per CU — the f32 walk's measured occupancy rule (hnsw_kernels.hip); a row group holds
// 8 rows x CPL x 2 registers here, half of the f32 instance's.  1 024 dimensions (CPL 4): groups of 4 rows — with 8 the
// register-list instances kept 12-28 bytes per lane in scratch memory; the group size does not change a bit (reduce_rows).
template <int METRIC, int CPL, int NS, bool F16>
__global__ __launch_bounds__(256, 4) void hnsw_search_half_kernel(HnswSearchArgs a) {
  hnsw_walk_body<METRIC, CPL, NS, false, false, false, WalkDistHalf<METRIC, CPL, 4, (CPL == 4 ? 4 : 8), F16>>(a);
}

// list_slots: 0 = LDS list (any ef), kSearchRegSlots = register list, as the f32 walk
template <int METRIC, int CPL, bool F16>
static hipError_t launch_half_t(const HnswSearchArgs& a, int slots, size_t lds, hipStream_t st) {
  if (a.list_slots == kSearchRegSlots)
    return launch_walk_blocks(hnsw_search_half_kernel<METRIC, CPL, kSearchRegSlots, F16>, a, a.n_cus, slots, lds, st);
  return launch_walk_blocks(hnsw_search_half_kernel<METRIC, CPL, 0, F16>, a, a.n_cus, slots, lds, st);
}
// (Cosine, Euclidean and DotProduct: refused in front of the call otherwise)
template <bool F16>
static hipError_t launch_half(const HnswSearchArgs& a, int slots, size_t lds, hipStream_t st) {
  return walk_dispatch<BitMetrics::kFallToDot>(a.metric, a.dim, [&](auto M, auto C) { return launch_half_t<M(), C(), F16>(a, slots, lds, st); });
}

// NativeHnsw::search over the f16 (f16 = true) or bf16 image for nq device-resident f32 queries + result mapping.  Enqueues on
// `st`; no host synchronisation.
int32_t hnsw_search_half_dev(vdb_hip_index* ix, bool f16, const float* d_q, uint64_t q_stride, uint32_t nq, uint32_t k, uint32_t ef,
                             uint32_t cap_mult, uint64_t* d_ids, float* d_scores, uint32_t* d_n, hipStream_t st) {
  // (the statuses of the exact half sweeps, select_stage.hip brute_bf16_dev)
  if (f16) {
    if (!ix->f16_enabled) return fail(VDB_ERR_STATE, "f16 graph search: call vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) first");
  } else if (!ix->bf16_enabled) {
    return fail(VDB_ERR_STATE, "bf16 graph search: call vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16) first");
  }
  if (ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, "half-precision graph search: Cosine, DotProduct and Euclidean only");
  HnswSearchArgs a{};
  int slots = 0;
  const int32_t rc = hnsw_search_prepare(ix, d_q, q_stride, nq, k, ef, cap_mult, d_ids, d_scores, d_n, st, 0, nullptr, &a, &slots);
  if (rc != VDB_OK || slots == 0) return rc;
  // the image instead of the f32 rows: same fields, the stride in half elements
  a.rows = reinterpret_cast<const float*>(f16 ? ix->rows_f16.as<uint16_t>() : ix->rows_bf16.as<uint16_t>());
  a.norms = f16 ? ix->norms_f16.as<float>() : ix->norms_bf16.as<float>();
  a.row_stride = ix->bf16_stride;
  a.bits = nullptr;
  a.vis_log2 = 0;  // HBM bitmaps
  const size_t lds = hnsw_lds_bytes(a.cap, a.nbmax, a.dim, a.words, a.metric);
  EventPair* ev = next_events(ix);
  if (ev) (void)hipEventRecord(ev->a, st);
  const hipError_t e = f16 ? launch_half<true>(a, slots, lds, st) : launch_half<false>(a, slots, lds, st);
  if (ev) (void)hipEventRecord(ev->b, st);
  if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("half-precision hnsw_search launch: ") + hipGetErrorString(e));
  ix->stats_pending = true;
  return VDB_OK;
}

}  // namespace vdb
