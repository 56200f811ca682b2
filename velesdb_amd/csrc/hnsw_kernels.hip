// hnsw_kernels.hip — graph traversal on the GPU: NativeHnsw::search (native/graph.rs:251-270) =
// greedy descent search_layer_single (graph.rs:405-428) on layers max_layer..1, then the layer-0
// best-first beam search_layer (graph.rs:438-520); result mapping of HnswIndex::search_with_quality
// (index/hnsw/index/search.rs:79-93, transform_score backend_adapter.rs:160-168).
//
// Design (MI355X-first; the path is bound by random 3 KB row gathers from HBM):
//   * one 256-thread block per query in flight ("slot"); slots loop over the batch.  With 4 blocks
//     per CU that is 1024 queries x 4 waves x 8 rows x 3 KB = several hundred KB of loads in flight
//     per CU, far more than the latency-bandwidth product needs.
//   * a step = (leader wave decides what to evaluate) -> barrier -> (all 4 waves evaluate up to
//     `nbmax` distances: wave w takes groups of 8 neighbours, every row is read as float4 per lane,
//     1 KiB per load instruction, canonical per-lane fmaf chains + xor-butterfly, vdb_device.hpp)
//     -> barrier.  The decision logic is the reference's, statement for statement, executed by one
//     wave with wave-uniform control flow; the 64 lanes are used for the list operations.
//   * candidates + results live in ONE sorted list in LDS keyed by (total-order(dist), node) with
//     an "expanded" flag per entry:  results  = the first min(len, ef) entries (the reference's
//     max-heap bounded to ef holds exactly the ef smallest keys pushed so far), candidates = the
//     entries not yet expanded (the reference pushes every admitted node to both heaps).  Entries
//     past position ef were evicted from results; they stay only while the reference's
//     termination test `c_dist > furthest` (graph.rs:474) could still let them be expanded
//     (exact ties with the current furthest distance: common for Hamming, never for f32).
//   * visited set = one bit per node in HBM per slot (atomicOr test-and-set, L2-resident), undone
//     after each query from a log of the ids it set.
// Algorithmic HBM bytes per query: n_dist * dim * 4 + n_expand * M0 * 4, with n_dist / n_expand
// counted by the kernel (stats), SURVEY.md §8(d).
#include <algorithm>
#include <cstdlib>

#include "vdb_probe_env.hpp"
#include "vdb_hnsw_device.hpp"
#include "vdb_index.hpp"
#include "vdb_walk_launch.hpp"

namespace vdb {


// ------------------------------------------------------------------------------------------
// LDS: keys[cap] u64 | nb_id[nbmax] u32 | nb_d[nbmax] f32 | ctl[4] u32 | flags[cap] u8 (padded to 16)
//      | query scratch: generic f32 dims: d4*4 floats; bit metrics: `words` u32
// ------------------------------------------------------------------------------------------
// LAT (latency mode: calls of at most one query per CU, f32 metrics; the speculative step below: layer-0 lists of <= 64 neighbours,
// longer lists take the test-first form — launch_hnsw_search): a 1 024-thread block per query and a speculative layer-0 step.  A walk is a chain of dependent memory round trips — neighbour ids, visited
// test-and-set, rows — and a single query cannot hide them behind other queries: here all (<= 64) neighbours' rows are fetched
// at once by 16 waves (4 rows each) WITHOUT waiting for the visited test, which the leader wave issues alongside; the
// verdicts select, in list order, which of the evaluated distances are admitted.  Same ids, scores and counters (n_dist counts
// the unvisited neighbours, as the reference's loop evaluates them); the rows of visited neighbours are wasted bandwidth that a
// single query has to spare.
// __launch_bounds__(.., 4): four waves per SIMD = four 256-thread walks per CU.  Left alone the register-list instance took 143
// registers = three walks per CU; the walk is a chain of dependent memory round trips, and the rows in flight per CU are what
// the chip's random-gather bandwidth follows: 126 registers (no scratch) took the 8 192-query launch at 1 M x 768, ef 128 from
// 49.1 to 42.1 ms on one box (0.61 -> 0.72 of HBM; profiles/r04m_f32_walk_occupancy_ab.log), same ids / scores / counters.
// RAWEF: NativeHnsw-level calls whose ef_search may be smaller than the number of layer-0 entry points (search_multi_entry with
// ef_search < 4 and several probes, or ef_search = 0): ef is then raised per query at the layer-0 start (see P_START).  Only the
// generic instance (LDS list, any dimension) exists in this form: in every other instance ef stays the launch constant it was —
// as a loop-carried value it put 48 bytes of the register-list instances into scratch memory.
template <int METRIC, int CPL, int NS, bool LAT = false, bool VIS = false, bool RAWEF = false>
__global__ __launch_bounds__(LAT ? 1024 : 256, 4) void hnsw_search_kernel(HnswSearchArgs a) {
  // (the walk itself: hnsw_walk_body, vdb_hnsw_device.hpp — shared with the half-precision walk of hnsw_half.hip)
  hnsw_walk_body<METRIC, CPL, NS, LAT, VIS, RAWEF, WalkDistF32<METRIC, CPL, LAT ? 16 : 4, LAT ? 4 : 8>>(a);
}

// ---- host side -----------------------------------------------------------------------------
// the arrays WalkLds (vdb_hnsw_device.hpp) carves out of a walk block's dynamic LDS — the same offsets, change both together
static size_t walk_lds_base(uint32_t cap, uint32_t nbmax) {
  return (size_t)cap * 8 + (size_t)nbmax * 8 + 16 + (((size_t)cap + 15) & ~(size_t)15);
}
// the dynamic LDS of a walk block: WalkLds plus the query scratch of the distance phase
size_t hnsw_lds_bytes(uint32_t cap, uint32_t nbmax, uint32_t dim, uint32_t words, int metric) {
  size_t s = walk_lds_base(cap, nbmax);
  if (metric == kHamming || metric == kJaccard)
    s += (size_t)words * 4;
  else if (sweep_cpl_for_dim(dim) == 0)
    s += (size_t)((dim + 3) / 4) * 16;
  return (s + 15) & ~(size_t)15;
}
// ... of an int8 walk block (hnsw_search_int8_kernel, hnsw_int8.hip; hnsw_search_filters_int8_kernel, hnsw_filtered.hip): WalkLds |
// f32 query scratch (generic dims: the re-score) | the query's code words [code_words] | (pad 16) | re-score output [nbmax] u64
size_t hnsw_int8_lds_bytes(uint32_t cap, uint32_t nbmax, uint32_t dim, uint32_t code_words) {
  size_t s = walk_lds_base(cap, nbmax);
  if (sweep_cpl_for_dim(dim) == 0) s += (size_t)((dim + 3) / 4) * 16;
  s += (size_t)code_words * 4;
  s = (s + 15) & ~(size_t)15;
  return s + (size_t)nbmax * 8;
}
// ... of a half walk block with the f32 re-score behind it (hnsw_search_filters_half_rescore_kernel, hnsw_filtered.hip): WalkLds |
// f32 query scratch (generic dims: the rounded query of the walk, then the unrounded one of the re-score) | (pad 16) | re-score
// output [nbmax] u64
size_t hnsw_half_rescore_lds_bytes(uint32_t cap, uint32_t nbmax, uint32_t dim) {
  return hnsw_lds_bytes(cap, nbmax, dim, 0, kCosine) + (size_t)nbmax * 8;
}

// latency mode: one 1 024-thread block per query (at most one query per CU per call); vis_log2: the LDS visited set or the HBM bitmaps
template <int METRIC, int CPL>
static hipError_t launch_lat(const HnswSearchArgs& a, int slots, size_t lds, hipStream_t st) {
  return dispatch_bool(a.vis_log2 != 0, [&](auto VIS) {
    return launch_walk_grid(hnsw_search_kernel<METRIC, CPL, kSearchRegSlots, true, VIS()>, a, slots, lds, st, 1024);
  });
}
// the throughput kernel.  list_slots: 0 = LDS list (any ef), kSearchRegSlots = register list (ef + 64 <= kSearchRegSlots * 64)
template <int METRIC, int CPL>
static hipError_t launch_t(const HnswSearchArgs& a, int slots, size_t lds, hipStream_t st) {
  return dispatch_bool(a.list_slots == kSearchRegSlots, [&](auto REG) {
    constexpr int NS = REG() ? kSearchRegSlots : 0;
    return dispatch_bool(a.vis_log2 != 0, [&](auto VIS) {
      return launch_walk_blocks(hnsw_search_kernel<METRIC, CPL, NS, false, VIS()>, a, a.n_cus, slots, lds, st);
    });
  });
}
// VELESDB_HNSW_LATENCY_MODE=0 keeps the throughput kernel for every call (A / B measurements), =2 takes the latency-mode kernel
// whatever the corpus size (fuzzing it over small graphs: tools/fuzz_hnsw.py)
static const int g_hnsw_lat = [] {
  const char* e = probe_env("VELESDB_HNSW_LATENCY_MODE");
  return e ? atoi(e) : 1;
}();
static const uint32_t g_hnsw_lat_max = [] {  // 0: one query per CU (the default); VELESDB_HNSW_LATENCY_MAX_QUERIES overrides
  const char* e = probe_env("VELESDB_HNSW_LATENCY_MAX_QUERIES");
  return e ? (uint32_t)atoi(e) : 0u;
}();

// VELESDB_HNSW_PREFETCH_IDS: 0 = every pop requests its own neighbour list, 1 = the latency-mode walk always asks for the predicted
// next pop's list too, unset = the measured default: only over a corpus beyond the Infinity Cache (1 M x 768: 1 102 -> 1 091 us per
// one-query call at a 48 % hit rate; 10 K x 768, cache-resident: 659 -> 671 us at 55 % — profiles/r04q2_*)
static const int g_hnsw_pf = [] {
  const char* e = probe_env("VELESDB_HNSW_PREFETCH_IDS");
  return e ? atoi(e) : -1;
}();
// VELESDB_HNSW_VIS_LDS: 0 = HBM bitmaps everywhere, 1 = the exact LDS set in the throughput kernel too (two blocks per CU
// instead of four), unset = the measured default (see pick_vis)
static const int g_hnsw_vis = [] {
  const char* e = probe_env("VELESDB_HNSW_VIS_LDS");
  return e ? atoi(e) : -1;
}();
// the LDS visited set of a launch: 2^log2 entries behind the kernel's other LDS, or none.  A walk at ef visits ~75 ef nodes
// (1 M x 768, M0 = 64: 9 570 at ef 128) and the kernel stops a query at 3/4 of the table (the caller re-runs it on the bitmap):
// offered where that is unlikely.
static uint32_t pick_vis(const HnswSearchArgs& a, size_t lds, bool lat) {
  if (!a.vis_log2 || g_hnsw_vis == 0) return 0;  // (a.vis_log2 != 0 on entry: the caller allows it — not a re-run)
  if (!lat && g_hnsw_vis != 1) return 0;
  for (uint32_t lg = lat ? 15u : 14u; lg >= 14u; lg--) {
    const uint64_t limit = (3ull << lg) / 4;
    if ((uint64_t)a.ef * 90 + a.nbmax <= limit && lds + ((size_t)4 << lg) <= 160 * 1024) return lg;
  }
  return 0;
}

hipError_t launch_hnsw_search(const HnswSearchArgs& a0, int slots, hipStream_t st) {
  HnswSearchArgs a = a0;
  size_t lds = hnsw_lds_bytes(a.cap, a.nbmax, a.dim, a.words, a.metric);
  if (a.raw_small_ef) {  // NativeHnsw-level call with ef_search < 4: the generic instance that raises ef to the entry points per query
    a.vis_log2 = 0;      // (HBM bitmaps)
    a.pf_ids = 0;
    return walk_dispatch_metric<BitMetrics::kTaken>(a.metric, [&](auto M) {
      return launch_walk_blocks(hnsw_search_kernel<M(), 0, 0, false, false, true>, a, a.n_cus, slots, lds, st);
    });
  }
  // at most one query per CU (measured at 1 M x 768, ef 128: 64 queries 1.57 ms against 2.68 ms on the throughput kernel, 256
  // queries 2.12 against 3.21 ms — a 1 024-thread block per CU is all the chip holds of this kernel) over a corpus that does not
  // sit in the 256 MB Infinity Cache: the latency-mode kernel (f32 metrics,
  // register list, layer-0 lists of <= 64 neighbours).  Over a cache-resident corpus the walk is not latency-bound the same way
  // (10 K x 768: 408 us per query on the throughput kernel, 599 us in latency mode, whose speculation fetches visited rows too)
  // (round 3: with the visited set in LDS the latency-mode kernel also serves cache-resident corpora — WITHOUT the speculation:
  // test first, fetch the unvisited; VELESDB_HNSW_LATENCY_MODE=2 forces the speculative form, =3 the other one)
  const bool beyond_cache = (uint64_t)a.n_rows * a.row_stride * 4 >= (256ull << 20);
  a.pf_ids = g_hnsw_pf >= 0 ? (g_hnsw_pf ? 1u : 0u) : (beyond_cache ? 1u : 0u);
  const uint32_t lat_vis = pick_vis(a0, lds, true);
  // Layer-0 lists of more than 64 neighbours (HnswParams::for_dataset_size, params.rs:72-147: M 128 => M0 256 from 10 001 vectors of
  // more than 256 dimensions up): the speculative step holds one neighbour per lane of the leader wave, so such graphs take the
  // latency-mode kernel in its test-first form — the LDS set answers in a few cycles, the 16 waves then fetch only the unvisited
  // neighbours' rows (at M0 256 most of a list is already visited: fetching every row would be 768 KB per expansion) — and only
  // when that set fits (otherwise the throughput kernel: same walk, four waves).
  const bool wide_lists = a.layers[0].stride > 64;
  if (g_hnsw_lat && a.nq <= (g_hnsw_lat_max ? g_hnsw_lat_max : a.n_cus) && (g_hnsw_lat >= 2 || beyond_cache || lat_vis) && a.list_slots == kSearchRegSlots && a.rerank_k == 0 &&
      (!wide_lists || lat_vis) && a.nbmax >= 64 && (a.metric == kCosine || a.metric == kEuclidean || a.metric == kDot)) {
    a.lat_spec = wide_lists ? 0u : (g_hnsw_lat == 2 ? 1u : (g_hnsw_lat == 3 ? 0u : (beyond_cache ? 1u : 0u)));
    a.vis_log2 = pick_vis(a0, lds, true);
    a.vis_off = (uint32_t)lds;
    if (a.vis_log2) lds += (size_t)4 << a.vis_log2;
    return walk_dispatch<BitMetrics::kFallToDot>(a.metric, a.dim, [&](auto M, auto C) { return launch_lat<M(), C()>(a, (int)a.nq, lds, st); });
  }
  a.vis_log2 = pick_vis(a0, lds, false);
  a.vis_off = (uint32_t)lds;
  if (a.vis_log2) lds += (size_t)4 << a.vis_log2;
  return walk_dispatch<BitMetrics::kTaken>(a.metric, a.dim, [&](auto M, auto C) { return launch_t<M(), C()>(a, slots, lds, st); });
}

// one visited bitmap (capacity bits) + one id log per resident block, zero between launches.  want_slots = the blocks the
// coming launch runs (0: as many as the chip holds of any walk kernel): a search context that only ever serves small calls — the
// combining front's batches, search_front.hip — keeps 125 KB + 64 KB per query in flight at 1 M rows instead of 0.4 GB
int32_t ensure_traversal_scratch(vdb_hip_index* ix, hipStream_t st, int want_slots) {
  const uint64_t vis_words = (ix->capacity + 31) / 32;
  const int chip_slots = ix->n_cus * kTraversalSlotsPerCu;
  int max_slots = want_slots > 0 ? std::min(want_slots, chip_slots) : chip_slots;
  if (max_slots < chip_slots) max_slots = std::min(chip_slots, (max_slots + 63) / 64 * 64);
  if (ix->vis_words == vis_words) max_slots = std::max<int>(max_slots, (int)std::min<size_t>((size_t)chip_slots, ix->s_visited.cap / std::max<uint64_t>(vis_words * 4, 1)));  // (never shrinks)
  if (ix->vis_words != vis_words || ix->s_visited.cap < (size_t)max_slots * vis_words * 4) {
    hipError_t e = ix->s_visited.reserve((size_t)max_slots * vis_words * 4, false, st);
    if (e == hipSuccess) e = ix->s_vlog.reserve((size_t)max_slots * kVlogCap * 4, false, st);
    if (e == hipSuccess) e = ix->s_stats.reserve(64, false, st);
    if (e == hipSuccess) e = hipMemsetAsync(ix->s_visited.p, 0, ix->s_visited.cap, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(VDB_ERR_OOM, std::string("visited scratch: ") + hipGetErrorString(e));
    ix->vis_words = vis_words;
  }
  return VDB_OK;
}

// Index -> HnswSearchArgs, the one copy every walk launch fills its arguments from (the f32 and half walks below, hnsw_int8.hip,
// hnsw_filtered.hip).  The graph: every layer's lists (at most kMaxLayers: the callers refuse or never see more); returns the
// longest neighbour list, unrounded — the caller rounds it with whatever else shares its nb arrays ...
uint32_t walk_args_graph(const vdb_hip_index* ix, HnswSearchArgs& a) {
  uint32_t longest = 0;
  for (size_t l = 0; l < ix->layers.size() && l < (size_t)kMaxLayers; l++) {
    a.layers[l].nbr = ix->layers[l].nbr.as<uint32_t>();
    a.layers[l].cnt = ix->layers[l].cnt.as<uint32_t>();
    a.layers[l].stride = ix->layers[l].stride;
    longest = std::max(longest, ix->layers[l].stride);
  }
  return longest;
}
// ... and the index fields (rows = the f32 rows).  Queries, outputs, list sizes, scratch and counters are the caller's.
void walk_args_index(const vdb_hip_index* ix, HnswSearchArgs& a) {
  a.rows = ix->rows.as<float>();
  a.norms = ix->norms.as<float>();
  a.bits = ix->bits.as<uint32_t>();
  a.alive = ix->any_dead ? ix->alive.as<uint8_t>() : nullptr;
  a.ext_ids = ix->ext_ids.as<uint64_t>();
  a.row_stride = ix->row_stride;
  a.dim = ix->dim;
  a.words = ix->words;
  a.n_rows = (uint32_t)ix->n_rows;
  a.vlog_cap = kVlogCap;
  a.max_layer = ix->max_layer;
  a.entry_point = (uint32_t)ix->entry_point;
  a.metric = ix->metric;
  a.n_cus = (uint32_t)ix->n_cus;
}

// What a walk launch needs, shared by the f32 walk below and the half-precision walk (hnsw_half.hip): the graph checks, list
// capacity and LDS rule, the visited scratch, the zeroed counters and every HnswSearchArgs field (rows = the f32 rows).
// *slots = the resident blocks to launch; 0: nothing to launch, the outputs are already what the call returns.
int32_t hnsw_search_prepare(vdb_hip_index* ix, const float* d_q, uint64_t q_stride, uint32_t nq, uint32_t k, uint32_t ef,
                            uint32_t cap_mult, uint64_t* d_ids, float* d_scores, uint32_t* d_n, hipStream_t st,
                            uint32_t rerank_k, const uint32_t* d_extra_eps, HnswSearchArgs* out, int* out_slots) {
  *out_slots = 0;
  if (!ix->graph_valid) return fail(VDB_ERR_STATE, "HNSW graph not built for all rows (use mode BRUTE or build it)");
  if (nq == 0) return VDB_OK;
  if (ix->entry_point < 0 || ix->graph_nodes == 0 || k == 0) {  // graph.rs:252-255: no entry point => empty
    VDB_HIP(hipMemsetAsync(d_n, 0, (size_t)nq * 4, st));
    return VDB_OK;
  }
  if (ix->layers.size() > (size_t)kMaxLayers) return fail(VDB_ERR_UNSUPPORTED, "more than 16 graph layers");
  HnswSearchArgs& a = *out;
  a = HnswSearchArgs{};
  const uint32_t nbmax = (std::max(walk_args_graph(ix, a), rerank_k) + 63) / 64 * 64;
  // list capacity: ef results + room for evicted candidates that tie with the furthest result
  uint64_t cap = (uint64_t)ef + std::max<uint64_t>(64, (uint64_t)ef * cap_mult / 2);
  cap = (cap + 63) / 64 * 64;
  // small ef: the list lives in registers (first attempt only; an overflow re-run uses the larger LDS list)
  const bool raw_small = ix->raw_ef && ef < 4;  // (search_multi_entry: more entry points than ef_search are possible)
  const bool reg_list = !raw_small && cap_mult == 1 && rerank_k == 0 && (uint64_t)ef + 64 <= (uint64_t)kSearchRegSlots * 64 &&
                        ix->n_rows < (1ull << 31);
  if (reg_list) cap = (uint64_t)kSearchRegSlots * 64;
  const size_t lds = hnsw_lds_bytes((uint32_t)cap, nbmax, ix->dim, ix->words, ix->metric);
  if (cap > 0xFFFFFFFFull || lds > 160 * 1024)
    return fail(VDB_ERR_UNSUPPORTED, "ef too large for the LDS-resident candidate list (" + std::to_string(lds) + " B)");
  // slots: resident blocks; 4 per CU unless LDS limits it
  int per_cu = (int)std::min<size_t>(4, std::max<size_t>(1, (160 * 1024) / lds));
  int slots = (int)std::min<int64_t>((int64_t)nq, (int64_t)ix->n_cus * per_cu);
  int32_t rcs = ensure_traversal_scratch(ix, st, slots);
  if (rcs != VDB_OK) return rcs;
  const uint64_t vis_words = ix->vis_words;
  VDB_HIP(hipMemsetAsync(ix->s_stats.p, 0, 24, st));
  walk_args_index(ix, a);
  a.queries = d_q;
  a.q_stride = q_stride;
  a.visited = ix->s_visited.as<uint32_t>();
  a.vlog = ix->s_vlog.as<uint32_t>();
  a.vis_words = vis_words;
  a.out_ids = d_ids;
  a.out_scores = d_scores;
  a.out_n = d_n;
  a.stats = ix->s_stats.as<unsigned long long>();
  a.nq = nq;
  a.k = k;
  a.ef = ef;
  a.cap = (uint32_t)cap;
  a.nbmax = nbmax;
  a.rerank_k = rerank_k;
  a.extra_eps = d_extra_eps;
  a.raw_small_ef = raw_small ? 1u : 0u;
  a.list_slots = reg_list ? kSearchRegSlots : 0;
  a.vis_log2 = cap_mult == 1 ? 1u : 0u;  // "the LDS visited set is allowed" (a re-run after an overflow takes the bitmap)
  *out_slots = slots;
  return VDB_OK;
}

// NativeHnsw::search for nq device-resident queries (graph.rs:251-270) + result mapping
// (search.rs:79-93).  Enqueues on `st`; no host synchronisation.
int32_t hnsw_search_dev(vdb_hip_index* ix, const float* d_q, uint64_t q_stride, uint32_t nq, uint32_t k, uint32_t ef,
                        uint32_t cap_mult, uint64_t* d_ids, float* d_scores, uint32_t* d_n, hipStream_t st,
                        uint32_t rerank_k, const uint32_t* d_extra_eps) {
  HnswSearchArgs a{};
  int slots = 0;
  const int32_t rc = hnsw_search_prepare(ix, d_q, q_stride, nq, k, ef, cap_mult, d_ids, d_scores, d_n, st, rerank_k, d_extra_eps, &a, &slots);
  if (rc != VDB_OK || slots == 0) return rc;
  EventPair* ev = next_events(ix);
  if (ev) (void)hipEventRecord(ev->a, st);
  hipError_t e = launch_hnsw_search(a, slots, st);
  if (ev) (void)hipEventRecord(ev->b, st);
  if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("hnsw_search launch: ") + hipGetErrorString(e));
  ix->stats_pending = true;
  return VDB_OK;
}

}  // namespace vdb
