// search_front.hip — the host-pointer search entry points of the C ABI (VectorIndex::search, HnswIndex::search_with_quality /
// search_brute_force / search_batch_parallel / search_with_rerank) and the COMBINING FRONT in front of them.
//
// The reference's calling pattern: many threads, each searching ONE query under a read lock (index/hnsw/index/search.rs:80; its
// stress tests index/hnsw/native/tests.rs:264-416; the server calls collection.search once per request,
// velesdb-server/src/handlers/search.rs:34-73).  A GPU walk or sweep of one query leaves the chip empty (a graph walk occupies one
// CU of 256; a one-query sweep pays a whole corpus pass) and every call pays launch + copies + a synchronisation — one launch per
// caller tops out at a few thousand calls per second whatever the number of threads.  What the hardware needs is callers that
// arrive together SHARING a launch: 64 graph walks in one launch cost 1.4 ms, not 64 x 1.1 ms.
//
// Protocol (flat combining; per handle, state in vdb::Combiner):
//   * a call of <= kCombineMaxCall queries becomes a request in the handle's queue;
//   * a caller that finds fewer batches running than may run beside each other (leader_limit) becomes a LEADER: it takes its own
//     request and every queued request with the same (k, ef, mode, rerank_k) up to COMBINE_MAX_BATCH queries, leases a search
//     context (shared lock on the handle, like any search), stages all the queries in the context's pinned buffer, issues ONE
//     search, and hands every request its slice of the pinned result block; then it wakes the callers of its batch and hands its
//     slot to the first call still queued;
//   * everybody else sleeps on its own request until it is done — or until a leader slot is handed to it.
// A lone caller is its own leader at once (no timer in its way); under load the requests that arrive while the launches in front
// of them run form the next batch, so the batch size follows the load by itself; a leader that has evidence of company waits for
// the callers of the batch that just finished to come back first (at most COMBINE_WINDOW_US; see search_combined).
// Bits: every kernel behind search_dev answers a query independently of the batch it sits in (declared arithmetic per metric and
// mode; the tests compare single-query and batched calls bit for bit), so combining never changes a result.
#include <cstring>

#include "vdb_combiner.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_fusion.hpp"
#include "vdb_hybrid.hpp"
#include "vdb_index.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

void note_last_context(vdb_hip_index* handle, vdb_hip_index* ctx);  // index.hip
void note_last_kernels(uint32_t mask);                               // index.hip

void combiner_free(Combiner* c) { delete c; }

// one search of nq host queries on a leased context of `handle`; results land in ctx->h_out (the layout of reserve_out) and
// `deliver(ctx)` copies them out while the lease is still held
template <class Stage, class Deliver>
static int32_t run_search(vdb_hip_index* handle, uint32_t nq, uint32_t k, uint32_t ef, int32_t mode, uint32_t rerank_k, Stage&& stage,
                          Deliver&& deliver) {
  // searches share the handle (search.rs:80 takes the read lock); a member of a process group searches collectively on one
  // gather buffer: those calls stay exclusive
  std::shared_lock<IndexMutex> rd(handle->mu, std::defer_lock);
  std::unique_lock<IndexMutex> wr(handle->mu, std::defer_lock);
  if (handle->pcomm) wr.lock(); else rd.lock();
  CtxLease lease(handle);  // this search's scratch + stream: the handle itself, or one of its search contexts when it is busy
  if (lease.rc != VDB_OK) return lease.rc;
  vdb_hip_index* ix = lease.ctx;
  VDB_ENTER_SHARED(ix);
  int32_t rc = stage(ix);
  if (rc != VDB_OK) return rc;
  if (ix->pcomm && k) {  // member of a process group: every rank ends with the global top-k
    hipStream_t st = ix->stream;
    const int32_t m = (mode == VDB_SEARCH_AUTO) ? (ix->live <= 100 ? VDB_SEARCH_BRUTE : VDB_SEARCH_HNSW) : mode;
    rc = pcomm_exchange_merge(ix, nq, k, mode_higher_is_better(ix->metric, (rerank_k && mode != VDB_SEARCH_HNSW_INT8) ? VDB_SEARCH_BRUTE : m), ix->s_out_ids.as<uint64_t>(),
                              ix->s_out_scores.as<float>(), ix->s_out_n.as<uint32_t>(), st);
    if (rc != VDB_OK) return rc;
    VDB_HIP(hipMemcpyAsync(ix->h_out.p, ix->s_out.p, ix->s_out_bytes, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
  }
  deliver(ix);
  return VDB_OK;
}

// slice [at, at + nq) of a context's pinned result block (a batch of nq_total queries x k results) into a caller's arrays
static void deliver_slice(const vdb_hip_index* ix, uint32_t at, uint32_t nq, uint32_t nq_total, uint32_t k, uint64_t* out_ids,
                          float* out_scores, uint32_t* out_n) {
  const size_t kk = std::max<uint32_t>(k, 1);
  const unsigned char* h = ix->h_out.as<unsigned char>();
  const size_t o_sc = (size_t)nq_total * kk * 8, o_n = o_sc + (size_t)nq_total * kk * 4;
  if (k) {
    std::memcpy(out_ids, h + (size_t)at * k * 8, (size_t)nq * k * 8);
    std::memcpy(out_scores, h + o_sc + (size_t)at * k * 4, (size_t)nq * k * 4);
  }
  std::memcpy(out_n, h + o_n + (size_t)at * 4, (size_t)nq * 4);
}

static int32_t search_direct(vdb_hip_index* handle, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, int32_t mode,
                             uint32_t rerank_k, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return run_search(
      handle, nq, k, ef, mode, rerank_k,
      [&](vdb_hip_index* ix) { return search_to_device(ix, queries, nq, k, ef, mode, rerank_k, nullptr); },
      [&](vdb_hip_index* ix) { deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n); });
}

// vdb_hip_index_search_batch_filtered: always a launch of its own — callers with different filters must not share one, so a
// filtered call never queues at the combining front
static int32_t search_filtered_direct(vdb_hip_index* handle, const RowFilter* f, const float* queries, uint32_t nq, uint32_t k,
                                      uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return run_search(
      handle, nq, k, 0, VDB_SEARCH_BRUTE, 0,
      [&](vdb_hip_index* ix) { return search_filtered_to_device(ix, f, queries, nq, k); },
      [&](vdb_hip_index* ix) { deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n); });
}

// vdb_hip_index_search_batch_filtered_mode: the same in one of the SQ8 / Binary / half modes
static int32_t search_filtered_mode_direct(vdb_hip_index* handle, const RowFilter* f, int32_t mode, const float* queries, uint32_t nq, uint32_t k,
                                           uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return run_search(
      handle, nq, k, 0, mode, 0,
      [&](vdb_hip_index* ix) { return search_filtered_mode_to_device(ix, f, mode, queries, nq, k); },
      [&](vdb_hip_index* ix) { deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n); });
}

// vdb_hip_index_search_batch_filters (mode = VDB_SEARCH_BRUTE) and vdb_hip_index_search_batch_filters_mode (one of the
// SQ8 / Binary / half modes): the same with one optional filter per query; query i's answer sits in row row_of[i] of the
// context's result block
static int32_t search_filters_exact_direct(vdb_hip_index* handle, const RowFilter* const* filters, uint32_t n_filters, const uint32_t* fq,
                                           int32_t mode, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores,
                                           uint32_t* out_n) {
  std::vector<uint32_t> row_of;  // (stays empty when the call is one job whose rows are the call's: one copy out, as the calls above)
  uint32_t rows = 0;
  return run_search(
      handle, nq, k, 0, mode, 0,
      [&](vdb_hip_index* ix) { return search_filters_mode_to_device(ix, filters, n_filters, fq, mode, queries, nq, k, &row_of, &rows); },
      [&](vdb_hip_index* ix) {
        if (row_of.empty()) return deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n);
        for (uint32_t i = 0; i < nq; i++)
          deliver_slice(ix, row_of[i], 1, rows, k, out_ids + (size_t)i * k, out_scores + (size_t)i * k, out_n + i);
      });
}

// vdb_hip_index_search_graph_filtered: a launch (or a few) of its own on a leased context, like the exact filtered call
static int32_t search_graph_filtered_direct(vdb_hip_index* handle, const RowFilter* f, const float* queries, uint32_t nq, uint32_t k,
                                            uint32_t ef, int32_t route, uint32_t max_list, uint64_t* out_ids, float* out_scores,
                                            uint32_t* out_n, uint32_t* out_route) {
  return run_search(
      handle, nq, k, ef, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) { return search_graph_filtered_to_device(ix, f, queries, nq, k, ef, route, max_list, out_route); },
      [&](vdb_hip_index* ix) { deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n); });
}

// vdb_hip_index_search_graph_filters: the same, one filter per query; the routes travel with the results (nothing is written on error).
// rows: the rows of the walk (FiltersRows, vdb_index.hpp)
static int32_t search_graph_filters_direct(vdb_hip_index* handle, const RowFilter* const* filters, uint32_t n_filters, const uint32_t* fq,
                                           const float* queries, uint32_t nq, uint32_t k, uint32_t ef, int32_t route, uint32_t max_list,
                                           uint64_t* out_ids, float* out_scores, uint32_t* out_n, uint32_t* out_route, int rows = kFiltersF32,
                                           uint32_t ratio = 0) {
  std::vector<uint32_t> routes(nq, 0u);
  return run_search(
      handle, nq, k, ef, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) { return search_graph_filters_to_device(ix, filters, n_filters, fq, queries, nq, k, ef, route, max_list, routes.data(), rows, ratio); },
      [&](vdb_hip_index* ix) {
        deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n);
        if (out_route) std::memcpy(out_route, routes.data(), (size_t)nq * 4);
      });
}

// vdb_hip_index_multi_query_search: ONE lease — the walk of every vector of every group at the over-fetched k, the
// fusion kernel over the context's result lists (ix->s_out_ids / s_out_scores) on the same stream, the fused block back through
// pinned memory, one synchronisation behind the fusion.  The list lengths are the ones the search brought to the host (a search that
// had nothing to launch leaves them only there).
static int32_t multi_query_direct(vdb_hip_index* handle, const RowFilter* f, const float* queries, const uint32_t* group_sizes,
                                  uint32_t n_groups, uint32_t nq, uint32_t top_k, uint32_t kf, int32_t strategy, uint32_t rrf_k, const float* w,
                                  uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  const size_t kk = std::max<uint32_t>(top_k, 1);
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_gr = (size_t)nq * sizeof(FuseList), o_oi = o_gr + (size_t)n_groups * sizeof(FuseGroup), o_os = o_oi + up16((size_t)n_groups * kk * 8),
               o_on = o_os + up16((size_t)n_groups * kk * 4), total = o_on + up16((size_t)n_groups * 4);
  return run_search(
      handle, nq, kf, 0, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) -> int32_t {
        int32_t rc = f ? search_graph_filtered_to_device(ix, f, queries, nq, kf, 0, 0, 0, nullptr)
                       : search_to_device(ix, queries, nq, kf, 0, VDB_SEARCH_HNSW, 0, nullptr);
        if (rc != VDB_OK) return rc;
        hipStream_t st = ix->stream;
        const uint32_t* h_n = reinterpret_cast<const uint32_t*>(ix->h_out.as<unsigned char>() + ((unsigned char*)ix->s_out_n.p - (unsigned char*)ix->s_out.p));
        std::vector<FuseList> lists;
        std::vector<FuseGroup> groups;
        uint32_t most = 0;
        rc = fuse_plan(h_n, nq, std::max<uint32_t>(kf, 1), group_sizes, n_groups, &lists, &groups, &most);
        if (rc != VDB_OK) return rc;
        if (ix->s_fuse.reserve(total, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "fusion scratch");
        if (ix->h_fuse.reserve(total) != hipSuccess) return fail(VDB_ERR_OOM, "pinned fusion staging");
        unsigned char* h = ix->h_fuse.as<unsigned char>();
        unsigned char* d = ix->s_fuse.as<unsigned char>();
        std::memcpy(h, lists.data(), o_gr);
        std::memcpy(h + o_gr, groups.data(), o_oi - o_gr);
        VDB_HIP(hipMemcpyAsync(d, h, o_oi, hipMemcpyHostToDevice, st));
        FuseArgs a{};
        a.ids = ix->s_out_ids.as<uint64_t>();
        a.scores = ix->s_out_scores.as<float>();
        a.list_stride = std::max<uint32_t>(kf, 1);
        a.lists = reinterpret_cast<const FuseList*>(d);
        a.groups = reinterpret_cast<const FuseGroup*>(d + o_gr);
        a.strategy = strategy;
        a.rrf_k = rrf_k;
        a.w_avg = w[0];
        a.w_max = w[1];
        a.w_hit = w[2];
        a.top_k = top_k;
        a.out_ids = reinterpret_cast<uint64_t*>(d + o_oi);
        a.out_scores = reinterpret_cast<float*>(d + o_os);
        a.out_n = reinterpret_cast<uint32_t*>(d + o_on);
        rc = fuse_launch(a, n_groups, most, st);
        if (rc != VDB_OK) return rc;
        ix->last_kernels |= VDB_KERNEL_FUSE;
        VDB_HIP(hipMemcpyAsync(h + o_oi, d + o_oi, total - o_oi, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        return VDB_OK;
      },
      [&](vdb_hip_index* ix) {
        const unsigned char* h = ix->h_fuse.as<unsigned char>();
        if (top_k) {
          std::memcpy(out_ids, h + o_oi, (size_t)n_groups * top_k * 8);
          std::memcpy(out_scores, h + o_os, (size_t)n_groups * top_k * 4);
        }
        std::memcpy(out_n, h + o_on, (size_t)n_groups * 4);
      });
}

// text hits of a call from which their id-to-row mapping runs on a thread beside the walk
constexpr size_t kHybridMapThreadCells = 4096;
// vdb_hip_index_hybrid_search: ONE lease.  The walk of every query at the contract's k' is the per-query call's own
// code: it brings its whole result block (nq x k' records and the counts) to the context's pinned h_out and synchronises — the host
// needs the counts (a walk whose list overflowed is re-run).  Beside the walk a host thread maps the text ids to rows through the
// handle's id map (the shared lock is held: as vdb_hip_index_filter_create maps ids).  Then hybrid_fuse_kernel runs over the
// context's device lists (ix->s_out_ids at stride k': the fusion reads nothing of h_out but the counts) and the uploaded text ids on
// the same stream, the nq x k fused records come back through pinned memory and a second synchronisation ends the call.  The live
// flags and the filter's bitmap are read by the kernel.  `table` = hybrid_plan's (nv = the bound k'; set from the walk's counts here).
static int32_t hybrid_direct(vdb_hip_index* handle, const RowFilter* f, const float* queries, uint32_t nq, uint32_t k, uint32_t kf,
                             const uint64_t* text_ids, const uint32_t* text_n, uint32_t text_stride, std::vector<HybridQuery>& table,
                             uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  const size_t kk = std::max<uint32_t>(k, 1);
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t tcells = (size_t)nq * text_stride;
  const size_t o_tx = (size_t)nq * sizeof(HybridQuery), o_tr = o_tx + up16(tcells * 8), o_oi = o_tr + up16(tcells * 4),
               o_os = o_oi + up16((size_t)nq * kk * 8), o_on = o_os + up16((size_t)nq * kk * 4), total = o_on + up16((size_t)nq * 4);
  return run_search(
      handle, nq, kf, 0, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) -> int32_t {
        hipStream_t st = ix->stream;
        if (ix->s_fuse.reserve(total, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "hybrid fusion scratch");
        if (ix->h_fuse.reserve(total) != hipSuccess) return fail(VDB_ERR_OOM, "pinned hybrid fusion staging");
        unsigned char* h = ix->h_fuse.as<unsigned char>();
        unsigned char* d = ix->s_fuse.as<unsigned char>();
        // text ids -> rows, into the pinned block (the id map lives on the handle, not on its search contexts; removed ids are not in it)
        auto map_rows = [&, h]() {
          uint32_t* h_rows = reinterpret_cast<uint32_t*>(h + o_tr);
          const vdb_hip_index* own = primary_of(ix);
          for (uint32_t i = 0; i < nq; i++)
            for (uint32_t j = 0; j < text_stride; j++) {
              uint32_t row = 0xFFFFFFFFu;
              if (j < text_n[i]) {
                auto it = own->id_to_idx.find(text_ids[(size_t)i * text_stride + j]);
                if (it != own->id_to_idx.end() && it->second < ix->n_rows) row = (uint32_t)it->second;
              }
              h_rows[(size_t)i * text_stride + j] = row;
            }
        };
        // a call with many text hits maps them on a thread of its own while the walk runs (it only reads: the caller's arrays and the
        // id map, which the shared lock keeps as it is); a small one maps them in line (a thread costs more than a few hundred lookups)
        struct Joined {
          std::thread t;
          ~Joined() {
            if (t.joinable()) t.join();
          }
        } mapper;
        if (tcells >= kHybridMapThreadCells) mapper.t = std::thread(map_rows); else map_rows();
        int32_t rc = f ? search_graph_filtered_to_device(ix, f, queries, nq, kf, 0, 0, 0, nullptr)
                       : search_to_device(ix, queries, nq, kf, 0, VDB_SEARCH_HNSW, 0, nullptr);
        if (mapper.t.joinable()) mapper.t.join();
        if (rc != VDB_OK) return rc;
        const uint32_t* h_n = reinterpret_cast<const uint32_t*>(ix->h_out.as<unsigned char>() + ((unsigned char*)ix->s_out_n.p - (unsigned char*)ix->s_out.p));
        uint32_t most = 0;
        for (uint32_t i = 0; i < nq; i++) {
          table[i].nv = std::min<uint32_t>(h_n[i], kf);  // (a walk returns at most k' records)
          most = std::max(most, table[i].nv + table[i].nt);
        }
        std::memcpy(h, table.data(), o_tx);
        if (tcells) std::memcpy(h + o_tx, text_ids, tcells * 8);
        VDB_HIP(hipMemcpyAsync(d, h, o_oi, hipMemcpyHostToDevice, st));
        HybridArgs a{};
        a.vec_ids = ix->s_out_ids.as<uint64_t>();
        a.vec_stride = std::max<uint32_t>(kf, 1);
        a.text_ids = reinterpret_cast<const uint64_t*>(d + o_tx);
        a.text_rows = reinterpret_cast<const uint32_t*>(d + o_tr);
        a.text_stride = text_stride;
        a.queries = reinterpret_cast<const HybridQuery*>(d);
        a.alive = ix->any_dead ? ix->alive.as<uint8_t>() : nullptr;
        a.n_rows = (uint32_t)ix->n_rows;
        if (f) {
          a.filtered = 1;
          a.filter_bits = f->bitmap.as<uint32_t>();
          a.filter_rows = (uint32_t)f->n_rows;  // (<= ix->n_rows: filter_check, inside the filtered search above)
        }
        a.k = k;
        a.out_ids = reinterpret_cast<uint64_t*>(d + o_oi);
        a.out_scores = reinterpret_cast<float*>(d + o_os);
        a.out_n = reinterpret_cast<uint32_t*>(d + o_on);
        rc = hybrid_launch(a, nq, most, st);
        if (rc != VDB_OK) return rc;
        ix->last_kernels |= VDB_KERNEL_HYBRID_FUSE;
        VDB_HIP(hipMemcpyAsync(h + o_oi, d + o_oi, total - o_oi, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        return VDB_OK;
      },
      [&](vdb_hip_index* ix) {
        const unsigned char* h = ix->h_fuse.as<unsigned char>();
        if (k) {
          std::memcpy(out_ids, h + o_oi, (size_t)nq * k * 8);
          std::memcpy(out_scores, h + o_os, (size_t)nq * k * 4);
        }
        std::memcpy(out_n, h + o_on, (size_t)nq * 4);
      });
}

// ---- the fused searches with one optional filter per query over any rows form ----
// What the two calls below share.  A call runs in two phases on one lease (fused_phases_plan, vdb_filter_route.hpp): the walk of the
// unfiltered units through the plain call of the rows form and their fusion launch, then the walk of the filtered units through the
// call with one filter per query and theirs.  Either walk ends with the context's result block on the host and a synchronisation;
// a fusion launch is only enqueued behind it.  So the fusion of phase 1 may still be reading the result block when phase 2 reserves
// it: fused_reserve_out sizes the block for the larger phase in front of both, after which no reserve of the call moves it.
// the plain walk of a rows form (FiltersRows 4 / 5 have no mode of their own: the filters walk with an empty table)
static_assert((int)VDB_WALK_ROWS_F32 == (int)kFiltersF32 && (int)VDB_WALK_ROWS_F16 == (int)kFiltersF16 && (int)VDB_WALK_ROWS_BF16 == (int)kFiltersBF16 &&
                  (int)VDB_WALK_ROWS_INT8 == (int)kFiltersInt8 && (int)VDB_WALK_ROWS_F16_RESCORE == (int)kFiltersF16Rescore &&
                  (int)VDB_WALK_ROWS_BF16_RESCORE == (int)kFiltersBF16Rescore,
              "enum vdb_walk_rows is FiltersRows");
static int32_t fused_plain_mode(int rows) {
  return rows == kFiltersF16 ? VDB_SEARCH_HNSW_F16 : rows == kFiltersBF16 ? VDB_SEARCH_HNSW_BF16 : rows == kFiltersInt8 ? VDB_SEARCH_HNSW_INT8 : VDB_SEARCH_HNSW;
}
// every status the walks would decide on the handle's state, decided in front of both (the lock is held): the image or the quantiser
// of the rows form, every filter of the table (foreign: INVALID_ARG, stale: STATE), the graph
static int32_t fused_check_state(vdb_hip_index* ix, int rows, const RowFilter* const* filters, uint32_t n_filters, const char* what) {
  const bool f16 = rows == kFiltersF16 || rows == kFiltersF16Rescore, bf16 = rows == kFiltersBF16 || rows == kFiltersBF16Rescore;
  if (f16 && !ix->f16_enabled) return fail(VDB_ERR_STATE, std::string(what) + " over the f16 image: call vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) first");
  if (bf16 && !ix->bf16_enabled) return fail(VDB_ERR_STATE, std::string(what) + " over the bf16 image: call vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16) first");
  if (rows == kFiltersInt8 && !ix->quantizer_trained) return fail(VDB_ERR_STATE, std::string(what) + " over the int8 codes: call vdb_hip_index_train_quantizer first");
  for (uint32_t j = 0; j < n_filters; j++) {
    const int32_t rc = filter_check(ix, filters[j]);
    if (rc != VDB_OK) return rc;
  }
  if (!ix->graph_valid) return fail(VDB_ERR_STATE, std::string(what) + ": HNSW graph not built for all rows");
  return VDB_OK;
}
static size_t out_block_bytes(uint64_t lists, uint64_t list_len) {
  const size_t kk = (size_t)std::max<uint64_t>(list_len, 1);
  return (size_t)lists * kk * 12 + (size_t)lists * 4;  // reserve_out's layout
}
static int32_t fused_reserve_out(vdb_hip_index* ix, const FusedPhasesPlan& plan) {
  size_t bytes = 0;
  for (const FusedPhase& P : plan.phase)
    if (!P.units.empty()) bytes = std::max(bytes, out_block_bytes(P.lists, P.list_len));
  if (ix->s_out.reserve(bytes, false, ix->stream) != hipSuccess) return fail(VDB_ERR_OOM, "search scratch");
  return VDB_OK;
}
// the walk of one phase: n vectors (caller memory, gathered) at list length kf; the lists end in ix->s_out_ids at stride max(kf, 1),
// their lengths in ix->h_out.  fq_sub: the phase's table indices, one per vector (kPhaseFiltered only)
static int32_t fused_walk(vdb_hip_index* ix, int phase, int rows, uint32_t ratio, const RowFilter* const* filters, uint32_t n_filters,
                          const uint32_t* fq_sub, const float* q, uint32_t n, uint32_t kf) {
  if (phase == kPhaseUnfiltered && rows <= kFiltersInt8)  // (the int8 walk takes the call's ratio as its rerank_k; 0 = the handle's option)
    return search_to_device(ix, q, n, kf, 0, fused_plain_mode(rows), rows == kFiltersInt8 ? ratio : 0, nullptr);
  uint32_t r = ratio;
  if (rows == kFiltersInt8 && r == 0) r = (uint32_t)opt_value(ix, VDB_OPT_INT8_OVERSAMPLING);
  if (rows >= kFiltersF16Rescore && r == 0) r = 4u;  // DualPrecisionConfig::default, as vdb_hip_index_search_graph_filters_half_rescore
  std::vector<uint32_t> routes(n, 0u);
  if (phase == kPhaseFiltered) return search_graph_filters_to_device(ix, filters, n_filters, fq_sub, q, n, kf, 0, 0, 0, routes.data(), rows, r);
  const std::vector<uint32_t> none(n, 0u);  // (a table of no filters: value 0 = n_filters = no filter)
  return search_graph_filters_to_device(ix, nullptr, 0, none.data(), q, n, kf, 0, 0, 0, routes.data(), rows, r);
}
// the vectors of a phase's units in one array; `keep` owns the copy when the phase is not the whole call
template <class FirstOf>
static const float* fused_gather(const float* queries, uint32_t dim, const FusedPhase& P, uint64_t lists_total, FirstOf&& first_of,
                                 std::vector<float>* keep) {
  if (P.lists == lists_total) return queries;
  keep->resize((size_t)P.lists * dim);
  size_t at = 0;
  for (uint32_t u : P.units) {
    const uint64_t first = first_of(u), n = first_of(u + 1) - first;
    std::memcpy(keep->data() + at * dim, queries + (size_t)first * dim, (size_t)n * dim * 4);
    at += (size_t)n;
  }
  return keep->data();
}
// What a finished walk leaves on its context — the kernel bits and the counters of vdb_hip_index_last_search_stats — is reset by the
// next walk; a call of two phases reports the OR and the sum.  take(): behind the first walk (the plain walks keep their counters on
// the device until somebody asks: fetched here, the stream is idle behind the walk's own synchronisation); give(): behind the second
struct WalkCarry {
  bool any = false;
  uint32_t kernels = 0;
  uint64_t n_dist = 0, n_expand = 0, pf_hits = 0;
  static int32_t settle(vdb_hip_index* ix) {
    if (!ix->stats_pending) return VDB_OK;
    unsigned long long h[3] = {0, 0, 0};
    VDB_HIP(hipMemcpyAsync(h, ix->s_stats.p, 24, hipMemcpyDeviceToHost, ix->stream));
    VDB_HIP(hipStreamSynchronize(ix->stream));
    ix->last_n_dist = h[0];
    ix->last_n_expand = h[1];
    ix->last_pf_hits = h[2];
    ix->stats_pending = false;
    return VDB_OK;
  }
  int32_t take(vdb_hip_index* ix) {
    const int32_t rc = settle(ix);
    if (rc != VDB_OK) return rc;
    any = true;
    kernels = ix->last_kernels;
    n_dist = ix->last_n_dist;
    n_expand = ix->last_n_expand;
    pf_hits = ix->last_pf_hits;
    return VDB_OK;
  }
  int32_t give(vdb_hip_index* ix) const {
    if (!any) return VDB_OK;
    const int32_t rc = settle(ix);
    if (rc != VDB_OK) return rc;
    ix->last_kernels |= kernels;
    ix->last_n_dist += n_dist;
    ix->last_n_expand += n_expand;
    ix->last_pf_hits += pf_hits;
    return VDB_OK;
  }
};

// vdb_hip_index_hybrid_search_filters: hybrid_direct with one optional filter per query over any rows form.  ONE lease,
// one block in s_fuse / h_fuse: [HybridQuery of the filtered slots | HybridQuery of the unfiltered slots | slots, unfiltered first |
// filter descriptors | text ids | text rows | out ids | out scores | out n].  The phase that runs first uploads everything in front
// of the outputs but the other phase's HybridQuery entries, which go up behind that phase's walk (they hold the walk's counts) — the
// layout makes either upload one contiguous copy.  hybrid_fuse_filters_kernel writes every query's records into its own row of the
// one output block; one copy back and one synchronisation behind the last fusion.
static int32_t hybrid_filters_direct(vdb_hip_index* handle, int rows, uint32_t ratio, const RowFilter* const* filters, uint32_t n_filters,
                                     const uint32_t* fq, const float* queries, uint32_t nq, uint32_t k, const FusedPhasesPlan& plan,
                                     const uint64_t* text_ids, const uint32_t* text_n, uint32_t text_stride, const std::vector<HybridQuery>& table,
                                     uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  const size_t kk = std::max<uint32_t>(k, 1);
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t tcells = (size_t)nq * text_stride;
  const uint32_t n_un = (uint32_t)plan.phase[kPhaseUnfiltered].units.size(), n_fl = (uint32_t)plan.phase[kPhaseFiltered].units.size();
  const size_t o_hq_un = (size_t)n_fl * sizeof(HybridQuery), o_sl = (size_t)nq * sizeof(HybridQuery), o_de = o_sl + up16((size_t)nq * sizeof(HybridSlot)),
               o_tx = o_de + ((size_t)n_filters + 1) * sizeof(HybridFilterDesc), o_tr = o_tx + up16(tcells * 8), o_oi = o_tr + up16(tcells * 4),
               o_os = o_oi + up16((size_t)nq * kk * 8), o_on = o_os + up16((size_t)nq * kk * 4), total = o_on + up16((size_t)nq * 4);
  return run_search(
      handle, nq, k, 0, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) -> int32_t {
        int32_t rc = fused_check_state(ix, rows, filters, n_filters, "hybrid_search_filters");
        if (rc != VDB_OK) return rc;
        hipStream_t st = ix->stream;
        if (ix->s_fuse.reserve(total, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "hybrid fusion scratch");
        if (ix->h_fuse.reserve(total) != hipSuccess) return fail(VDB_ERR_OOM, "pinned hybrid fusion staging");
        if ((rc = fused_reserve_out(ix, plan)) != VDB_OK) return rc;
        unsigned char* h = ix->h_fuse.as<unsigned char>();
        unsigned char* d = ix->s_fuse.as<unsigned char>();
        // text ids -> rows, as hybrid_direct maps them: beside the first walk when there are many
        auto map_rows = [&, h]() {
          uint32_t* h_rows = reinterpret_cast<uint32_t*>(h + o_tr);
          const vdb_hip_index* own = primary_of(ix);
          for (uint32_t i = 0; i < nq; i++)
            for (uint32_t j = 0; j < text_stride; j++) {
              uint32_t row = 0xFFFFFFFFu;
              if (j < text_n[i]) {
                auto it = own->id_to_idx.find(text_ids[(size_t)i * text_stride + j]);
                if (it != own->id_to_idx.end() && it->second < ix->n_rows) row = (uint32_t)it->second;
              }
              h_rows[(size_t)i * text_stride + j] = row;
            }
        };
        struct Joined {
          std::thread t;
          ~Joined() {
            if (t.joinable()) t.join();
          }
        } mapper;
        if (tcells >= kHybridMapThreadCells) mapper.t = std::thread(map_rows); else map_rows();
        // what does not wait for a walk: the slots (unfiltered first), the descriptors, the text ids
        HybridSlot* h_slots = reinterpret_cast<HybridSlot*>(h + o_sl);
        uint32_t at = 0;
        for (int ph = 0; ph < 2; ph++)
          for (uint32_t i : plan.phase[ph].units) h_slots[at++] = HybridSlot{i, fq[i]};
        HybridFilterDesc* h_desc = reinterpret_cast<HybridFilterDesc*>(h + o_de);
        for (uint32_t j = 0; j < n_filters; j++)
          h_desc[j] = HybridFilterDesc{filters[j]->bitmap.as<uint32_t>(), (uint32_t)filters[j]->n_rows, 0};  // (n_rows <= ix->n_rows: filter_check)
        h_desc[n_filters] = HybridFilterDesc{nullptr, 0, 0};
        if (tcells) std::memcpy(h + o_tx, text_ids, tcells * 8);
        HybridFiltersArgs fa{};
        fa.h.text_ids = reinterpret_cast<const uint64_t*>(d + o_tx);
        fa.h.text_rows = reinterpret_cast<const uint32_t*>(d + o_tr);
        fa.h.text_stride = text_stride;
        fa.h.alive = ix->any_dead ? ix->alive.as<uint8_t>() : nullptr;
        fa.h.n_rows = (uint32_t)ix->n_rows;
        fa.h.k = k;
        fa.h.out_ids = reinterpret_cast<uint64_t*>(d + o_oi);
        fa.h.out_scores = reinterpret_cast<float*>(d + o_os);
        fa.h.out_n = reinterpret_cast<uint32_t*>(d + o_on);
        fa.descs = reinterpret_cast<const HybridFilterDesc*>(d + o_de);
        fa.n_filters = n_filters;
        WalkCarry carry;
        bool shared_up = false;  // the slots, descriptors and text hits are on the device
        std::vector<float> qbuf;
        std::vector<uint32_t> fq_sub;
        for (int ph = 0; ph < 2; ph++) {
          const FusedPhase& P = plan.phase[ph];
          const uint32_t n = (uint32_t)P.units.size(), kf = (uint32_t)P.list_len;  // (kf <= 8192: the plan's limit)
          if (n == 0) continue;
          const float* q = fused_gather(queries, ix->dim, P, nq, [](uint32_t u) { return (uint64_t)u; }, &qbuf);
          if (ph == kPhaseFiltered) {
            fq_sub.resize(n);
            for (uint32_t b = 0; b < n; b++) fq_sub[b] = fq[P.units[b]];
          }
          rc = fused_walk(ix, ph, rows, ratio, filters, n_filters, fq_sub.data(), q, n, kf);
          if (mapper.t.joinable()) mapper.t.join();
          if (rc != VDB_OK) {
            (void)hipStreamSynchronize(st);  // (the first phase's fusion may be in flight over this context's scratch)
            return rc;
          }
          const bool more = ph == kPhaseUnfiltered && n_fl != 0;
          if (more && (rc = carry.take(ix)) != VDB_OK) return rc;
          if (!more && (rc = carry.give(ix)) != VDB_OK) return rc;
          const uint32_t* h_n = reinterpret_cast<const uint32_t*>(ix->h_out.as<unsigned char>() + ((unsigned char*)ix->s_out_n.p - (unsigned char*)ix->s_out.p));
          const size_t o_hq = ph == kPhaseUnfiltered ? o_hq_un : 0;
          HybridQuery* h_q = reinterpret_cast<HybridQuery*>(h + o_hq);
          uint32_t most = 0;
          for (uint32_t b = 0; b < n; b++) {
            h_q[b] = table[P.units[b]];
            h_q[b].nv = std::min<uint32_t>(h_n[b], kf);  // (a walk returns at most k' records)
            most = std::max(most, h_q[b].nv + h_q[b].nt);
          }
          // this phase's HybridQuery entries, and with the first upload of the call everything behind them
          const size_t up_end = shared_up ? o_hq + (size_t)n * sizeof(HybridQuery) : o_oi;
          VDB_HIP(hipMemcpyAsync(d + o_hq, h + o_hq, up_end - o_hq, hipMemcpyHostToDevice, st));
          shared_up = true;
          fa.h.vec_ids = ix->s_out_ids.as<uint64_t>();
          fa.h.vec_stride = std::max<uint32_t>(kf, 1);
          fa.h.queries = reinterpret_cast<const HybridQuery*>(d + o_hq);
          fa.slots = reinterpret_cast<const HybridSlot*>(d + o_sl) + (ph == kPhaseFiltered ? n_un : 0);
          rc = hybrid_filters_launch(fa, n, most, st);
          if (rc != VDB_OK) return rc;
        }
        ix->last_kernels |= VDB_KERNEL_HYBRID_FUSE;
        VDB_HIP(hipMemcpyAsync(h + o_oi, d + o_oi, total - o_oi, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        return VDB_OK;
      },
      [&](vdb_hip_index* ix) {
        const unsigned char* h = ix->h_fuse.as<unsigned char>();
        if (k) {
          std::memcpy(out_ids, h + o_oi, (size_t)nq * k * 8);
          std::memcpy(out_scores, h + o_os, (size_t)nq * k * 4);
        }
        std::memcpy(out_n, h + o_on, (size_t)nq * 4);
      });
}

// vdb_hip_index_multi_query_search_filters: multi_query_direct with one optional filter per GROUP over any rows form.
// The same two phases, both at the over-fetched k; fuse_lists_kernel is unchanged — a phase's groups are fused into consecutive rows
// of the one output block (the unfiltered groups first) and the host hands every group its row.  One block in s_fuse / h_fuse:
// [lists and groups of the unfiltered phase | lists and groups of the filtered phase | out ids | out scores | out n]; a phase's tables
// go up behind its walk (they hold the walk's counts), one copy each.
static int32_t multi_query_filters_direct(vdb_hip_index* handle, int rows, uint32_t ratio, const RowFilter* const* filters, uint32_t n_filters,
                                          const uint32_t* fg, const float* queries, const uint32_t* group_sizes, uint32_t n_groups, uint32_t nq,
                                          uint32_t top_k, const FusedPhasesPlan& plan, int32_t strategy, uint32_t rrf_k, const float* w,
                                          uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  const size_t kk = std::max<uint32_t>(top_k, 1);
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const FusedPhase& UN = plan.phase[kPhaseUnfiltered];
  const uint32_t n_un = (uint32_t)UN.units.size();
  const size_t tab_un = (size_t)UN.lists * sizeof(FuseList) + (size_t)n_un * sizeof(FuseGroup);
  const size_t o_oi = (size_t)nq * sizeof(FuseList) + (size_t)n_groups * sizeof(FuseGroup), o_os = o_oi + up16((size_t)n_groups * kk * 8),
               o_on = o_os + up16((size_t)n_groups * kk * 4), total = o_on + up16((size_t)n_groups * 4);
  std::vector<uint64_t> first(n_groups + 1u, 0);  // the first vector of every group
  for (uint32_t g = 0; g < n_groups; g++) first[g + 1] = first[g] + group_sizes[g];
  std::vector<uint32_t> row_of(n_groups, 0u);     // where a group's answer sits in the output block
  return run_search(
      handle, nq, top_k, 0, VDB_SEARCH_HNSW, 0,
      [&](vdb_hip_index* ix) -> int32_t {
        int32_t rc = fused_check_state(ix, rows, filters, n_filters, "multi_query_search_filters");
        if (rc != VDB_OK) return rc;
        hipStream_t st = ix->stream;
        if (ix->s_fuse.reserve(total, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "fusion scratch");
        if (ix->h_fuse.reserve(total) != hipSuccess) return fail(VDB_ERR_OOM, "pinned fusion staging");
        if ((rc = fused_reserve_out(ix, plan)) != VDB_OK) return rc;
        unsigned char* h = ix->h_fuse.as<unsigned char>();
        unsigned char* d = ix->s_fuse.as<unsigned char>();
        FuseArgs a{};
        a.strategy = strategy;
        a.rrf_k = rrf_k;
        a.w_avg = w[0];
        a.w_max = w[1];
        a.w_hit = w[2];
        a.top_k = top_k;
        WalkCarry carry;
        std::vector<float> qbuf;
        std::vector<uint32_t> fq_sub, sizes;
        std::vector<FuseList> lists;
        std::vector<FuseGroup> groups;
        for (int ph = 0; ph < 2; ph++) {
          const FusedPhase& P = plan.phase[ph];
          const uint32_t n = (uint32_t)P.units.size(), nv = (uint32_t)P.lists, kf = (uint32_t)P.list_len;
          if (n == 0) continue;
          const uint32_t row0 = ph == kPhaseFiltered ? n_un : 0;
          const float* q = fused_gather(queries, ix->dim, P, nq, [&](uint32_t g) { return first[g]; }, &qbuf);
          sizes.resize(n);
          fq_sub.clear();
          for (uint32_t b = 0; b < n; b++) {
            const uint32_t g = P.units[b];
            sizes[b] = group_sizes[g];
            row_of[g] = row0 + b;
            if (ph == kPhaseFiltered) fq_sub.insert(fq_sub.end(), group_sizes[g], fg[g]);  // every vector of a group on the group's filter
          }
          rc = fused_walk(ix, ph, rows, ratio, filters, n_filters, fq_sub.data(), q, nv, kf);
          if (rc != VDB_OK) {
            (void)hipStreamSynchronize(st);  // (the first phase's fusion may be in flight over this context's scratch)
            return rc;
          }
          const bool more = ph == kPhaseUnfiltered && !plan.phase[kPhaseFiltered].units.empty();
          if (more && (rc = carry.take(ix)) != VDB_OK) return rc;
          if (!more && (rc = carry.give(ix)) != VDB_OK) return rc;
          const uint32_t* h_n = reinterpret_cast<const uint32_t*>(ix->h_out.as<unsigned char>() + ((unsigned char*)ix->s_out_n.p - (unsigned char*)ix->s_out.p));
          uint32_t most = 0;
          rc = fuse_plan(h_n, nv, std::max<uint32_t>(kf, 1), sizes.data(), n, &lists, &groups, &most);
          if (rc != VDB_OK) return rc;
          const size_t o_li = ph == kPhaseFiltered ? tab_un : 0, o_gr = o_li + (size_t)nv * sizeof(FuseList), o_end = o_gr + (size_t)n * sizeof(FuseGroup);
          std::memcpy(h + o_li, lists.data(), o_gr - o_li);
          std::memcpy(h + o_gr, groups.data(), o_end - o_gr);
          VDB_HIP(hipMemcpyAsync(d + o_li, h + o_li, o_end - o_li, hipMemcpyHostToDevice, st));
          a.ids = ix->s_out_ids.as<uint64_t>();
          a.scores = ix->s_out_scores.as<float>();
          a.list_stride = std::max<uint32_t>(kf, 1);
          a.lists = reinterpret_cast<const FuseList*>(d + o_li);
          a.groups = reinterpret_cast<const FuseGroup*>(d + o_gr);
          a.out_ids = reinterpret_cast<uint64_t*>(d + o_oi) + (size_t)row0 * kk;
          a.out_scores = reinterpret_cast<float*>(d + o_os) + (size_t)row0 * kk;
          a.out_n = reinterpret_cast<uint32_t*>(d + o_on) + row0;
          rc = fuse_launch(a, n, most, st);
          if (rc != VDB_OK) return rc;
        }
        ix->last_kernels |= VDB_KERNEL_FUSE;
        VDB_HIP(hipMemcpyAsync(h + o_oi, d + o_oi, total - o_oi, hipMemcpyDeviceToHost, st));
        VDB_HIP(hipStreamSynchronize(st));
        return VDB_OK;
      },
      [&](vdb_hip_index* ix) {
        const unsigned char* h = ix->h_fuse.as<unsigned char>();
        const uint64_t* h_ids = reinterpret_cast<const uint64_t*>(h + o_oi);
        const float* h_sc = reinterpret_cast<const float*>(h + o_os);
        const uint32_t* h_cnt = reinterpret_cast<const uint32_t*>(h + o_on);
        for (uint32_t g = 0; g < n_groups; g++) {
          if (top_k) {
            std::memcpy(out_ids + (size_t)g * top_k, h_ids + (size_t)row_of[g] * kk, (size_t)top_k * 8);
            std::memcpy(out_scores + (size_t)g * top_k, h_sc + (size_t)row_of[g] * kk, (size_t)top_k * 4);
          }
          out_n[g] = h_cnt[row_of[g]];
        }
      });
}

// the leader's part: one launch for `batch` (same shape; batch[0] is the leader's own request)
static void run_batch(vdb_hip_index* handle, CombineReq* const* reqs, size_t n_reqs) {
  struct Span {
    CombineReq* const* b;
    size_t n;
    CombineReq* const* begin() const { return b; }
    CombineReq* const* end() const { return b + n; }
  } batch{reqs, n_reqs};
  uint32_t total = 0;
  for (CombineReq* r : batch) total += r->nq;
  const CombineReq& s = *reqs[0];
  vdb_hip_index* served = nullptr;
  uint32_t served_kernels = 0;
  const int32_t rc = guarded([&]() -> int32_t {
    return run_search(
        handle, total, s.k, s.ef, s.mode, s.rerank_k,
        [&](vdb_hip_index* ix) -> int32_t {
          served = ix;
          uint32_t at = 0;
          for (CombineReq* r : batch) {
            const int32_t rs = stage_queries(ix, r->queries, at, r->nq, total);
            if (rs != VDB_OK) return rs;
            at += r->nq;
          }
          return search_staged(ix, total, s.k, s.ef, s.mode, s.rerank_k);
        },
        [&](vdb_hip_index* ix) {
          served_kernels = ix->last_kernels;  // (the context is still leased: a later search on it cannot have overwritten the mask)
          uint32_t at = 0;
          for (CombineReq* r : batch) {
            deliver_slice(ix, at, r->nq, total, s.k, r->out_ids, r->out_scores, r->out_n);
            at += r->nq;
          }
        });
  });
  const std::string err = rc != VDB_OK ? std::string(vdb_hip_last_error()) : std::string();
  for (CombineReq* r : batch) {
    r->rc = rc;
    r->err = err;
    r->served_by = served;
    r->kernels = served_kernels;
  }
}

// how many batches may run beside each other when this request leads one: graph walks are latency-bound (one CU per query in a
// small call: two launches overlap for free), sweeps are bandwidth-bound (a second launch beside the first only halves both
// batches: 16 callers on the 1 M exact sweep 26 K q/s with one batch in flight, 15 K with two)
static int leader_limit(const vdb_hip_index* handle, const CombineReq& r) {
  const int64_t o = opt_value(handle, VDB_OPT_COMBINE_INFLIGHT);
  if (o > 0) return (int)o;
  const bool walk = r.mode == VDB_SEARCH_HNSW || r.mode == VDB_SEARCH_HNSW_INT8 || r.mode == VDB_SEARCH_HNSW_F16 ||
                    r.mode == VDB_SEARCH_HNSW_BF16 || r.mode == VDB_SEARCH_AUTO;
  return walk ? 2 : 1;
}

// the protocol (vdb_combiner.hpp) over a handle: its options, one launch per batch
struct HandleFront {
  vdb_hip_index* handle;
  uint32_t max_batch() const { return (uint32_t)opt_value(handle, VDB_OPT_COMBINE_MAX_BATCH); }
  uint32_t window_us() const { return (uint32_t)opt_value(handle, VDB_OPT_COMBINE_WINDOW_US); }
  int leader_limit(const CombineReq& r) const { return vdb::leader_limit(handle, r); }
  void run_batch(CombineReq* const* reqs, size_t n) { vdb::run_batch(handle, reqs, n); }
  void finish(CombineReq& me) {
    if (me.served_by) {
      note_last_context(handle, me.served_by);
      if (me.rc == VDB_OK) note_last_kernels(me.kernels);  // this thread's diagnostics describe ITS search, whoever ran it
    }
    if (me.rc != VDB_OK) set_last_error(me.err);
  }
};

// HnswIndex::search_batch_parallel (batch.rs:159-197) / search_with_quality / search_brute_force
int32_t search_batch_host(vdb_hip_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, int32_t mode,
                          uint32_t rerank_k, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  if (!ix || (nq && (!queries || !out_n)) || (nq && k && (!out_ids || !out_scores)))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  if (nq == 0) return VDB_OK;
  if (ix->group) return group_search_host(ix, queries, nq, k, ef, mode, rerank_k, out_ids, out_scores, out_n);
  // (options are read without the handle's lock: set_option on a handle that is being searched is a benign race on an int)
  if (ix->combiner && !ix->pcomm && nq <= kCombineMaxCall && opt_value(ix, VDB_OPT_COMBINE_MAX_BATCH) >= (int64_t)nq &&
      opt_value(ix, VDB_OPT_COMBINE_MAX_BATCH) > 1) {
    CombineReq me;
    me.queries = queries;
    me.nq = nq;
    me.k = k;
    me.ef = ef;
    me.mode = mode;
    me.rerank_k = rerank_k;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_n = out_n;
    HandleFront front{ix};
    return search_combined(front, ix->combiner, me);
  }
  return search_direct(ix, queries, nq, k, ef, mode, rerank_k, out_ids, out_scores, out_n);
}

Combiner* combiner_new() { return new Combiner(); }

}  // namespace vdb

using namespace vdb;

extern "C" {

int32_t vdb_hip_index_search_batch(vdb_hip_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t ef,
                                   int32_t mode, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  return search_batch_host(ix, queries, nq, k, ef, mode, 0, out_ids, out_scores, out_n);
  });
}

// the `_with_filter` searches of the collection layer (collection/search/vector.rs:164-239, batch.rs:26-136) with the ids the
// caller's predicate matched: exact top-k among exactly those rows (include/velesdb_hip.h)
int32_t vdb_hip_index_search_batch_filtered(vdb_hip_index* ix, const void* filter, const float* queries, uint32_t nq, uint32_t k,
                                            int32_t mode, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  const RowFilter* f = static_cast<const RowFilter*>(filter);
  if (!ix || !f || (nq && (!queries || !out_n)) || (nq && k && (!out_ids || !out_scores))) return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "filtered search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "filtered search: not available on a member of a process group");
  if (mode != VDB_SEARCH_BRUTE) return fail(VDB_ERR_UNSUPPORTED, "filtered search: VDB_SEARCH_BRUTE only (the graph and quantised modes keep the over-fetch rule)");
  if (nq == 0) return VDB_OK;
  return search_filtered_direct(ix, f, queries, nq, k, out_ids, out_scores, out_n);
  });
}

// search_with_filter on a collection whose rows live as SQ8 codes, sign bits or a half image (the reference's filtered search works
// whatever the storage mode): exact top-k in that mode among exactly the filter's rows (include/velesdb_hip.h)
int32_t vdb_hip_index_search_batch_filtered_mode(vdb_hip_index* ix, const void* filter, int32_t mode, const float* queries, uint32_t nq,
                                                 uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  const RowFilter* f = static_cast<const RowFilter*>(filter);
  if (!ix || !f || (nq && (!queries || !out_n)) || (nq && k && (!out_ids || !out_scores))) return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "filtered search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "filtered search: not available on a member of a process group");
  if (mode != VDB_SEARCH_BRUTE_SQ8 && mode != VDB_SEARCH_BRUTE_BINARY && mode != VDB_SEARCH_BRUTE_BF16 && mode != VDB_SEARCH_BRUTE_F16)
    return fail(VDB_ERR_UNSUPPORTED, "filtered search by mode: VDB_SEARCH_BRUTE_SQ8 / _BINARY / _BF16 / _F16 only (VDB_SEARCH_BRUTE has "
                                     "vdb_hip_index_search_batch_filtered, the graph modes vdb_hip_index_search_graph_filtered)");
  if (nq == 0) return VDB_OK;
  return search_filtered_mode_direct(ix, f, mode, queries, nq, k, out_ids, out_scores, out_n);
  });
}

// search_batch_with_filters (collection/search/batch.rs:26-115) on the exact sweep: one optional filter per query.
// The table's conventions are those of vdb_hip_index_search_graph_filters below.
int32_t vdb_hip_index_search_batch_filters(vdb_hip_index* ix, void** filters, uint32_t n_filters, const uint32_t* filter_of_query,
                                           const float* queries, uint32_t nq, uint32_t k, int32_t mode, uint64_t* out_ids, float* out_scores,
                                           uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || (n_filters && !filters) || (nq && (!queries || !out_n || !filter_of_query)) || (nq && k && (!out_ids || !out_scores)))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "filtered search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "filtered search: not available on a member of a process group");
  if (mode != VDB_SEARCH_BRUTE) return fail(VDB_ERR_UNSUPPORTED, "filtered search: VDB_SEARCH_BRUTE only (the graph modes have vdb_hip_index_search_graph_filters)");
  for (uint32_t j = 0; j < n_filters; j++)
    if (!filters[j]) return fail(VDB_ERR_INVALID_ARG, "filtered search: filter " + std::to_string(j) + " of the table is null");
  for (uint32_t i = 0; i < nq; i++)
    if (filter_of_query[i] > n_filters)
      return fail(VDB_ERR_INVALID_ARG, "filtered search: query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) +
                                           " of a table of " + std::to_string(n_filters));
  if (nq == 0) return VDB_OK;
  return search_filters_exact_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, VDB_SEARCH_BRUTE, queries,
                                     nq, k, out_ids, out_scores, out_n);
  });
}

// search_batch_with_filters on a collection whose rows live as SQ8 codes, sign bits or a half image: one optional filter per query in one
// of those modes (include/velesdb_hip.h).  The table's errors are the call's above, the mode's those of
// vdb_hip_index_search_batch_filtered_mode.
int32_t vdb_hip_index_search_batch_filters_mode(vdb_hip_index* ix, void** filters, uint32_t n_filters, const uint32_t* filter_of_query, int32_t mode,
                                                const float* queries, uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || (n_filters && !filters) || (nq && (!queries || !out_n || !filter_of_query)) || (nq && k && (!out_ids || !out_scores)))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "filtered search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "filtered search: not available on a member of a process group");
  if (mode != VDB_SEARCH_BRUTE_SQ8 && mode != VDB_SEARCH_BRUTE_BINARY && mode != VDB_SEARCH_BRUTE_BF16 && mode != VDB_SEARCH_BRUTE_F16)
    return fail(VDB_ERR_UNSUPPORTED, "filtered search by mode: VDB_SEARCH_BRUTE_SQ8 / _BINARY / _BF16 / _F16 only (VDB_SEARCH_BRUTE has "
                                     "vdb_hip_index_search_batch_filters, the graph modes vdb_hip_index_search_graph_filters)");
  for (uint32_t j = 0; j < n_filters; j++)
    if (!filters[j]) return fail(VDB_ERR_INVALID_ARG, "filtered search: filter " + std::to_string(j) + " of the table is null");
  for (uint32_t i = 0; i < nq; i++)
    if (filter_of_query[i] > n_filters)
      return fail(VDB_ERR_INVALID_ARG, "filtered search: query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) +
                                           " of a table of " + std::to_string(n_filters));
  if (nq == 0) return VDB_OK;
  return search_filters_exact_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, mode, queries, nq, k,
                                     out_ids, out_scores, out_n);
  });
}

// diagnostic: the plan of this thread's last vdb_hip_index_search_batch_filters / _filters_mode call — {filter groups, groups on the listed route,
// groups on mask substitution, unfiltered queries, grouped sweep launches, merge launches behind them}
int32_t vdb_hip_index_last_filters_exact_plan(vdb_hip_index* ix, uint32_t* out) {
  return vdb::guarded([&]() -> int32_t {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARG, "null argument");
    VDB_NO_GROUP(ix, "last_filters_exact_plan");
    std::shared_lock<vdb::IndexMutex> g(ix->mu);
    last_fx_plan_of_this_thread(ix, out);
    return VDB_OK;
  });
}

// The argument checks the five filtered graph entry points below share, in two parts around each entry point's own mode, metric and
// ratio checks (their statuses come between these).  In front of them: the null arguments — table_ok: the call's filter, or its table and
// filter_of_query — the multi-device handle and the process group ...
static bool fg_table_ok(void** filters, uint32_t n_filters, const uint32_t* filter_of_query, uint32_t nq) {
  return !(n_filters && !filters) && !(nq && !filter_of_query);
}
static int32_t fg_check_handle(vdb_hip_index* ix, bool table_ok, const float* queries, uint32_t nq, uint32_t k, const uint64_t* out_ids,
                               const float* out_scores, const uint32_t* out_n) {
  if (!ix || !table_ok || (nq && (!queries || !out_n)) || (nq && k && (!out_ids || !out_scores))) return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "filtered graph search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: not available on a member of a process group");
  return VDB_OK;
}
// ... and behind them: the route, the table's entries and every query's index into the table (filter_of_query null: the one-filter
// call, which has no table).  A call of no queries returns VDB_OK behind this.
static int32_t fg_check_table(int32_t route, void** filters, uint32_t n_filters, const uint32_t* filter_of_query, uint32_t nq) {
  if (route < 0 || route > 2) return fail(VDB_ERR_INVALID_ARG, "filtered graph search: route 0 (auto), 1 (walk) or 2 (exact pass)");
  for (uint32_t j = 0; j < n_filters; j++)
    if (!filters[j]) return fail(VDB_ERR_INVALID_ARG, "filtered graph search: filter " + std::to_string(j) + " of the table is null");
  for (uint32_t i = 0; filter_of_query && i < nq; i++)
    if (filter_of_query[i] > n_filters)
      return fail(VDB_ERR_INVALID_ARG, "filtered graph search: query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) +
                                           " of a table of " + std::to_string(n_filters));
  return VDB_OK;
}

// VDB_SEARCH_HNSW with the allow-list consulted inside the walk, and the exact pass behind it (hnsw_filtered.hip)
int32_t vdb_hip_index_search_graph_filtered(vdb_hip_index* ix, const void* filter, const float* queries, uint32_t nq, uint32_t k,
                                            uint32_t ef, int32_t mode, int32_t route, uint32_t max_list, uint64_t* out_ids,
                                            float* out_scores, uint32_t* out_n, uint32_t* out_route) {
  return vdb::guarded([&]() -> int32_t {
  const RowFilter* f = static_cast<const RowFilter*>(filter);
  int32_t rc = fg_check_handle(ix, f != nullptr, queries, nq, k, out_ids, out_scores, out_n);
  if (rc != VDB_OK) return rc;
  if (mode != VDB_SEARCH_HNSW) return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: VDB_SEARCH_HNSW only (no filtered walk over the half / int8 images)");
  rc = fg_check_table(route, nullptr, 0, nullptr, nq);  // (no table: the route alone)
  if (rc != VDB_OK || nq == 0) return rc;
  return search_graph_filtered_direct(ix, f, queries, nq, k, ef, route, max_list, out_ids, out_scores, out_n, out_route);
  });
}

// search_batch_with_filters (collection/search/batch.rs:26-115): one optional filter per query in one graph call
int32_t vdb_hip_index_search_graph_filters(vdb_hip_index* ix, void** filters, uint32_t n_filters, const uint32_t* filter_of_query,
                                           const float* queries, uint32_t nq, uint32_t k, uint32_t ef, int32_t mode, int32_t route,
                                           uint32_t max_list, uint64_t* out_ids, float* out_scores, uint32_t* out_n, uint32_t* out_route) {
  return vdb::guarded([&]() -> int32_t {
  int32_t rc = fg_check_handle(ix, fg_table_ok(filters, n_filters, filter_of_query, nq), queries, nq, k, out_ids, out_scores, out_n);
  if (rc != VDB_OK) return rc;
  if (mode != VDB_SEARCH_HNSW) return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: VDB_SEARCH_HNSW only (no filtered walk over the half / int8 images)");
  rc = fg_check_table(route, filters, n_filters, filter_of_query, nq);
  if (rc != VDB_OK || nq == 0) return rc;
  return search_graph_filters_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, queries, nq, k, ef,
                                     route, max_list, out_ids, out_scores, out_n, out_route);
  });
}

// the same call over the f16 / bf16 image of the rows: a symbol of its own — the two calls above keep refusing the
// half modes, which is their documented contract
int32_t vdb_hip_index_search_graph_filters_half(vdb_hip_index* ix, int32_t mode, void** filters, uint32_t n_filters,
                                                const uint32_t* filter_of_query, const float* queries, uint32_t nq, uint32_t k, uint32_t ef,
                                                int32_t route, uint32_t max_list, uint64_t* out_ids, float* out_scores, uint32_t* out_n,
                                                uint32_t* out_route) {
  return vdb::guarded([&]() -> int32_t {
  int32_t rc = fg_check_handle(ix, fg_table_ok(filters, n_filters, filter_of_query, nq), queries, nq, k, out_ids, out_scores, out_n);
  if (rc != VDB_OK) return rc;
  if (mode != VDB_SEARCH_HNSW_F16 && mode != VDB_SEARCH_HNSW_BF16)
    return fail(VDB_ERR_UNSUPPORTED, "half-precision filtered graph search: VDB_SEARCH_HNSW_F16 or VDB_SEARCH_HNSW_BF16");
  if (ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, "half-precision filtered graph search: Cosine, DotProduct and Euclidean only");
  rc = fg_check_table(route, filters, n_filters, filter_of_query, nq);
  if (rc != VDB_OK || nq == 0) return rc;
  return search_graph_filters_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, queries, nq, k, ef,
                                     route, max_list, out_ids, out_scores, out_n, out_route,
                                     mode == VDB_SEARCH_HNSW_F16 ? kFiltersF16 : kFiltersBF16);
  });
}

// the same call over the u8 codes of DualPrecisionHnsw: the int8 walk with the allow-list inside it, the re-score of the
// k * oversampling_ratio best allowed candidates in f32, the f32 exact pass.  A symbol of its own — the three calls above keep
// refusing mode 4, which is their documented contract
int32_t vdb_hip_index_search_graph_filters_int8(vdb_hip_index* ix, void** filters, uint32_t n_filters, const uint32_t* filter_of_query,
                                                const float* queries, uint32_t nq, uint32_t k, uint32_t ef_search,
                                                uint32_t oversampling_ratio, int32_t route, uint32_t max_list, uint64_t* out_ids,
                                                float* out_scores, uint32_t* out_n, uint32_t* out_route) {
  return vdb::guarded([&]() -> int32_t {
  int32_t rc = fg_check_handle(ix, fg_table_ok(filters, n_filters, filter_of_query, nq), queries, nq, k, out_ids, out_scores, out_n);
  if (rc != VDB_OK) return rc;
  if (ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, "int8 filtered graph search: Cosine, DotProduct and Euclidean only");
  // the bound vdb_hip_set_int8_oversampling holds the handle's option to: k * ratio sizes nbmax, ef and the LDS list of the walk
  if (oversampling_ratio > 64) return fail(VDB_ERR_INVALID_ARG, "int8 filtered graph search: oversampling_ratio 0 (the handle's option) or 1..64");
  rc = fg_check_table(route, filters, n_filters, filter_of_query, nq);
  if (rc != VDB_OK || nq == 0) return rc;
  const uint32_t ratio = oversampling_ratio ? oversampling_ratio : (uint32_t)opt_value(ix, VDB_OPT_INT8_OVERSAMPLING);
  return search_graph_filters_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, queries, nq, k,
                                     ef_search, route, max_list, out_ids, out_scores, out_n, out_route, kFiltersInt8, ratio);
  });
}

// the half call with exact f32 answers: the walk over the f16 / bf16 image with the allow-list inside it at
// ef = max(ef_search, k * ratio), the re-score of the k * ratio best allowed candidates over the f32 rows, the f32 exact pass.
// oversampling_ratio 0 = 4 (DualPrecisionConfig::default; the handle's int8 option is not read)
int32_t vdb_hip_index_search_graph_filters_half_rescore(vdb_hip_index* ix, int32_t mode, void** filters, uint32_t n_filters,
                                                        const uint32_t* filter_of_query, const float* queries, uint32_t nq, uint32_t k,
                                                        uint32_t ef_search, uint32_t oversampling_ratio, int32_t route, uint32_t max_list,
                                                        uint64_t* out_ids, float* out_scores, uint32_t* out_n, uint32_t* out_route) {
  return vdb::guarded([&]() -> int32_t {
  int32_t rc = fg_check_handle(ix, fg_table_ok(filters, n_filters, filter_of_query, nq), queries, nq, k, out_ids, out_scores, out_n);
  if (rc != VDB_OK) return rc;
  if (mode != VDB_SEARCH_HNSW_F16 && mode != VDB_SEARCH_HNSW_BF16)
    return fail(VDB_ERR_UNSUPPORTED, "half-precision filtered graph search with re-score: VDB_SEARCH_HNSW_F16 or VDB_SEARCH_HNSW_BF16");
  if (ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, "half-precision filtered graph search with re-score: Cosine, DotProduct and Euclidean only");
  // k * ratio sizes nbmax, ef and the LDS list of the walk: the int8 call's bound
  if (oversampling_ratio > 64)
    return fail(VDB_ERR_INVALID_ARG, "half-precision filtered graph search with re-score: oversampling_ratio 0 (= 4) or 1..64");
  rc = fg_check_table(route, filters, n_filters, filter_of_query, nq);
  if (rc != VDB_OK || nq == 0) return rc;
  return search_graph_filters_direct(ix, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, queries, nq, k,
                                     ef_search, route, max_list, out_ids, out_scores, out_n, out_route,
                                     mode == VDB_SEARCH_HNSW_F16 ? kFiltersF16Rescore : kFiltersBF16Rescore,
                                     oversampling_ratio ? oversampling_ratio : 4u);
  });
}

// Collection::multi_query_search / multi_query_search_ids (collection/search/batch.rs:206-403) for n_groups user queries: the walks at
// the over-fetched k and FusionStrategy::fuse (fusion/strategy.rs) on the device (include/velesdb_hip.h)
int32_t vdb_hip_index_multi_query_search(vdb_hip_index* ix, const void* filter, const float* queries, const uint32_t* group_sizes,
                                         uint32_t n_groups, uint32_t top_k, int32_t strategy, uint32_t rrf_k, const float* weights,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || (n_groups && (!queries || !group_sizes || !out_n)) || (n_groups && top_k && (!out_ids || !out_scores)))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "multi_query_search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "multi_query_search: not available on a member of a process group");
  float w[3];
  const int32_t rcs = fuse_check_strategy(strategy, weights, w);
  if (rcs != VDB_OK) return rcs;
  const uint64_t kf = fusion::overfetch(top_k);
  uint64_t nq = 0;
  for (uint32_t g = 0; g < n_groups; g++) {
    if (group_sizes[g] == 0)
      return fail(VDB_ERR_INVALID_ARG, "multi_query_search requires at least one vector (group " + std::to_string(g) + ")");
    if (group_sizes[g] > VDB_MAX_FUSED_VECTORS)
      return fail(VDB_ERR_INVALID_ARG, "multi_query_search supports at most " + std::to_string(VDB_MAX_FUSED_VECTORS) + " vectors, got " +
                                           std::to_string(group_sizes[g]) + " (group " + std::to_string(g) + ")");
    if (group_sizes[g] * kf > VDB_FUSE_MAX_RECORDS)
      return fail(VDB_ERR_UNSUPPORTED, "multi_query_search: group " + std::to_string(g) + " would fuse " + std::to_string(group_sizes[g]) + " lists of " +
                                           std::to_string(kf) + " records, more than the " + std::to_string(VDB_FUSE_MAX_RECORDS) + " one block's LDS takes");
    nq += group_sizes[g];
  }
  if (n_groups == 0) return VDB_OK;
  if (nq > 0xFFFFFFFFull) return fail(VDB_ERR_INVALID_ARG, "multi_query_search: more than 2^32 - 1 vectors in one call");
  return multi_query_direct(ix, static_cast<const RowFilter*>(filter), queries, group_sizes, n_groups, (uint32_t)nq, top_k, (uint32_t)kf, strategy,
                            rrf_k, w, out_ids, out_scores, out_n);
  });
}

// Collection::hybrid_search / hybrid_search_with_filter (collection/search/text.rs:113-299) for nq user queries with the text hits the
// caller's BM25 index returned: the walks at k' = 2k (with a filter: max(4k, k + 10), inside the walk) and the weighted rank fusion
// (vdb_hybrid.hpp) on the device (include/velesdb_hip.h)
int32_t vdb_hip_index_hybrid_search(vdb_hip_index* ix, const void* filter, const float* queries, uint32_t nq, uint32_t k, const uint64_t* text_ids,
                                    const uint32_t* text_n, uint32_t text_stride, const float* vector_weights, uint64_t* out_ids,
                                    float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || (nq && (!queries || !text_n || !out_n)) || (nq && k && (!out_ids || !out_scores)) || (nq && text_stride && !text_ids))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  VDB_NO_GROUP(ix, "hybrid_search");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "hybrid_search: not available on a member of a process group");
  // text.rs:137 (k * 2) and 244 (k.saturating_mul(4).max(k + 10)); 64-bit, so that a product past u32 is seen and refused below
  const uint64_t kf = filter ? std::max<uint64_t>((uint64_t)k * 4, (uint64_t)k + 10) : (uint64_t)k * 2;
  // every argument and limit check in one place (hybrid.hip): the vector lists are planned at their bound k' until the walks are back
  std::vector<HybridQuery> table;
  uint32_t most = 0;
  const int32_t rcp = hybrid_plan(nullptr, kf, text_n, text_stride, vector_weights, nq, &table, &most);
  if (rcp != VDB_OK || nq == 0) return rcp;
  return hybrid_direct(ix, static_cast<const RowFilter*>(filter), queries, nq, k, (uint32_t)kf, text_ids, text_n, text_stride, table, out_ids, out_scores,
                       out_n);
  });
}

// The argument checks the two calls below share, in the order of include/velesdb_hip.h: the rows form, the ratio (read for the forms
// that have one), the multi-device handle and the process group, the table; then — behind each call's own argument checks — the metric.
static int32_t fused_filters_check_args(vdb_hip_index* ix, const char* what, int32_t rows, uint32_t ratio, void** filters, uint32_t n_filters,
                                        const uint32_t* filter_of, uint32_t n_units) {
  const std::string w(what);
  if (rows < kFiltersF32 || rows > kFiltersBF16Rescore) return fail(VDB_ERR_INVALID_ARG, w + ": rows is one of enum vdb_walk_rows (0..5)");
  if (rows >= kFiltersInt8 && ratio > 64) return fail(VDB_ERR_INVALID_ARG, w + ": oversampling_ratio 0 (the rows form's default) or 1..64");
  if (ix->group) return fail(VDB_ERR_UNSUPPORTED, w + ": not available on a multi-device handle");
  if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, w + ": not available on a member of a process group");
  for (uint32_t j = 0; j < n_filters; j++)
    if (!filters[j]) return fail(VDB_ERR_INVALID_ARG, w + ": filter " + std::to_string(j) + " of the table is null");
  for (uint32_t i = 0; i < n_units; i++)
    if (filter_of[i] > n_filters)
      return fail(VDB_ERR_INVALID_ARG, w + ": entry " + std::to_string(i) + " names filter " + std::to_string(filter_of[i]) + " of a table of " + std::to_string(n_filters));
  return VDB_OK;
}
static int32_t fused_filters_check_metric(const vdb_hip_index* ix, const char* what, int32_t rows) {
  if (rows != kFiltersF32 && ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, std::string(what) + ": the half and int8 rows forms serve Cosine, DotProduct and Euclidean only");
  return VDB_OK;
}

// vdb_hip_index_hybrid_search with one optional filter per query over any rows form of the walk (include/velesdb_hip.h)
int32_t vdb_hip_index_hybrid_search_filters(vdb_hip_index* ix, int32_t rows, uint32_t oversampling_ratio, void** filters, uint32_t n_filters,
                                            const uint32_t* filter_of_query, const float* queries, uint32_t nq, uint32_t k, const uint64_t* text_ids,
                                            const uint32_t* text_n, uint32_t text_stride, const float* vector_weights, uint64_t* out_ids,
                                            float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || !fg_table_ok(filters, n_filters, filter_of_query, nq) || (nq && (!queries || !text_n || !out_n)) || (nq && k && (!out_ids || !out_scores)) ||
      (nq && text_stride && !text_ids))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  int32_t rc = fused_filters_check_args(ix, "hybrid_search_filters", rows, oversampling_ratio, filters, n_filters, filter_of_query, nq);
  if (rc != VDB_OK) return rc;
  // the weights and the text lists: hybrid_plan's checks and statuses (the vector lists are planned below, phase by phase)
  std::vector<HybridQuery> table;
  uint32_t most = 0;
  rc = hybrid_plan(nullptr, 0, text_n, text_stride, vector_weights, nq, &table, &most);
  if (rc != VDB_OK) return rc;
  if ((rc = fused_filters_check_metric(ix, "hybrid_search_filters", rows)) != VDB_OK) return rc;
  const FusedPhasesPlan plan = fused_phases_plan(
      filter_of_query, nq, n_filters, hybrid_list_len(k, false), hybrid_list_len(k, true), VDB_HYBRID_MAX_RECORDS, [](uint32_t) { return 1u; },
      [&](uint32_t i) { return text_n[i]; });
  if (plan.over >= 0)
    return fail(VDB_ERR_UNSUPPORTED, "hybrid_search_filters: query " + std::to_string(plan.over) + " would fuse a vector list of up to " +
                                         std::to_string(plan.phase[plan.over_phase].list_len) + " ids (" +
                                         (plan.over_phase == kPhaseFiltered ? "filtered" : "unfiltered") + ") and " + std::to_string(text_n[plan.over]) +
                                         " text hits, more than the " + std::to_string(VDB_HYBRID_MAX_RECORDS) + " records one block's LDS takes");
  if (nq == 0) return VDB_OK;
  return hybrid_filters_direct(ix, rows, oversampling_ratio, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_query, queries, nq,
                               k, plan, text_ids, text_n, text_stride, table, out_ids, out_scores, out_n);
  });
}

// vdb_hip_index_multi_query_search with one optional filter per group over any rows form of the walk
int32_t vdb_hip_index_multi_query_search_filters(vdb_hip_index* ix, int32_t rows, uint32_t oversampling_ratio, void** filters, uint32_t n_filters,
                                                 const uint32_t* filter_of_group, const float* queries, const uint32_t* group_sizes,
                                                 uint32_t n_groups, uint32_t top_k, int32_t strategy, uint32_t rrf_k, const float* weights,
                                                 uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || !fg_table_ok(filters, n_filters, filter_of_group, n_groups) || (n_groups && (!queries || !group_sizes || !out_n)) ||
      (n_groups && top_k && (!out_ids || !out_scores)))
    return fail(VDB_ERR_INVALID_ARG, "null argument");
  int32_t rc = fused_filters_check_args(ix, "multi_query_search_filters", rows, oversampling_ratio, filters, n_filters, filter_of_group, n_groups);
  if (rc != VDB_OK) return rc;
  float w[3];
  if ((rc = fuse_check_strategy(strategy, weights, w)) != VDB_OK) return rc;
  const uint64_t kf = fusion::overfetch(top_k);
  uint64_t nq = 0;
  for (uint32_t g = 0; g < n_groups; g++) {
    if (group_sizes[g] == 0)
      return fail(VDB_ERR_INVALID_ARG, "multi_query_search_filters requires at least one vector (group " + std::to_string(g) + ")");
    if (group_sizes[g] > VDB_MAX_FUSED_VECTORS)
      return fail(VDB_ERR_INVALID_ARG, "multi_query_search_filters supports at most " + std::to_string(VDB_MAX_FUSED_VECTORS) + " vectors, got " +
                                           std::to_string(group_sizes[g]) + " (group " + std::to_string(g) + ")");
    nq += group_sizes[g];
  }
  if (nq > 0xFFFFFFFFull) return fail(VDB_ERR_INVALID_ARG, "multi_query_search_filters: more than 2^32 - 1 vectors in one call");
  if ((rc = fused_filters_check_metric(ix, "multi_query_search_filters", rows)) != VDB_OK) return rc;
  const FusedPhasesPlan plan = fused_phases_plan(
      filter_of_group, n_groups, n_filters, kf, kf, VDB_FUSE_MAX_RECORDS, [&](uint32_t g) { return group_sizes[g]; }, [](uint32_t) { return 0u; });
  if (plan.over >= 0)
    return fail(VDB_ERR_UNSUPPORTED, "multi_query_search_filters: group " + std::to_string(plan.over) + " would fuse " + std::to_string(group_sizes[plan.over]) +
                                         " lists of " + std::to_string(kf) + " records, more than the " + std::to_string(VDB_FUSE_MAX_RECORDS) +
                                         " one block's LDS takes");
  if (n_groups == 0) return VDB_OK;
  return multi_query_filters_direct(ix, rows, oversampling_ratio, reinterpret_cast<const RowFilter* const*>(filters), n_filters, filter_of_group, queries,
                                    group_sizes, n_groups, (uint32_t)nq, top_k, plan, strategy, rrf_k, w, out_ids, out_scores, out_n);
  });
}

// HnswIndex::search_with_rerank / search_with_rerank_quality — search.rs:118-160,297-350
int32_t vdb_hip_index_search_rerank(vdb_hip_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t rerank_k,
                                    uint32_t ef, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (rerank_k == 0) return fail(VDB_ERR_INVALID_ARG, "rerank_k must be > 0");
  return search_batch_host(ix, queries, nq, k, ef, VDB_SEARCH_AUTO, rerank_k, out_ids, out_scores, out_n);
  });
}

// DualPrecisionHnsw::is_quantizer_trained — native/dual_precision.rs:117-120
int32_t vdb_hip_index_quantizer_trained(const vdb_hip_index* ix, int32_t* trained) {
  return vdb::guarded([&]() -> int32_t {
    if (!ix || !trained) return fail(VDB_ERR_INVALID_ARG, "null argument");
    // (written under the exclusive lock by train_quantizer — on a replica group by group_for_all once every replica is trained)
    std::shared_lock<IndexMutex> rd(const_cast<vdb_hip_index*>(ix)->mu);
    *trained = ix->quantizer_trained ? 1 : 0;
    return VDB_OK;
  });
}

// DualPrecisionHnsw::search_with_config — native/dual_precision.rs:259-278: the int8 traversal (+ exact f32 re-scoring of the
// k * oversampling_ratio best) only with a trained quantiser, use_int8_traversal and at least min_index_size vectors; otherwise
// the plain f32 graph search.  The configuration travels WITH the call, as in the reference.
int32_t vdb_hip_index_search_with_config(vdb_hip_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t ef_search,
                                         uint32_t oversampling_ratio, int32_t use_int8_traversal, uint64_t min_index_size,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
    if (!ix) return fail(VDB_ERR_INVALID_ARG, "null argument");
    // the same bound vdb_hip_set_int8_oversampling holds the handle's option to: k * ratio sizes nbmax, ef and the LDS list of the walk
    if (oversampling_ratio == 0 || oversampling_ratio > 64)
      return fail(VDB_ERR_INVALID_ARG, "oversampling_ratio must be in 1..64 (DualPrecisionConfig's default is 4)");
    // (n_rows: NativeHnsw::len() counts inserted vectors; the state is read under the shared lock, the search takes its own)
    bool int8;
    {
      std::shared_lock<IndexMutex> rd(ix->mu);
      int8 = ix->quantizer_trained && use_int8_traversal && ix->n_rows >= min_index_size;
    }
    // The f32 branch is NativeHnsw::search with ITS ef_search (dual_precision.rs:269,274 -> graph.rs:251-270: search_layer(ef_search)
    // as given, results cut to k): VDB_SEARCH_HNSW applies HnswIndex's SearchQuality rules on top (0 = Balanced, max(ef, k)).  The
    // two agree whenever 0 < k <= ef_search; the other calls — at most ef_search results, ef_search = 0 acting as 1 — take the
    // NativeHnsw-level entry point with one entry point (no draw from the graph's stream: graph.rs:303).  A device group has no such
    // entry point: its f32 branch keeps the HnswIndex rule.
    if (!int8 && !ix->group && !ix->pcomm && nq && k && (ef_search == 0 || ef_search < k))
      return vdb_hip_index_search_multi_entry(ix, queries, nq, k, ef_search, 1, out_ids, out_scores, out_n);
    return search_batch_host(ix, queries, nq, k, ef_search, int8 ? VDB_SEARCH_HNSW_INT8 : VDB_SEARCH_HNSW, int8 ? oversampling_ratio : 0, out_ids,
                             out_scores, out_n);
  });
}

// VectorIndex::search — index/mod.rs:58; trait_impl.rs:38-42
int32_t vdb_hip_index_search(vdb_hip_index* ix, const float* query, uint32_t query_len, uint32_t k, uint32_t ef,
                             int32_t mode, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || !query) return fail(VDB_ERR_INVALID_ARG, "null argument");
  if (query_len != ix->dim)
    return fail(VDB_ERR_DIM_MISMATCH, "Query dimension mismatch: expected " + std::to_string(ix->dim) + ", got " +
                                          std::to_string(query_len));
  return vdb_hip_index_search_batch(ix, query, 1, k, ef, mode, out_ids, out_scores, out_n);
  });
}

// NativeHnsw::search_multi_entry — index/hnsw/native/graph.rs:288-348.  The extra entry points come out of the graph's own
// xorshift stream (the one that draws insertion levels): the call CHANGES the index (exclusive lock), query i of the batch takes
// draws i (min(num_probes, 4) - 1) .. of it, exactly as nq sequential calls of the reference would.
int32_t vdb_hip_index_search_multi_entry(vdb_hip_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, uint32_t num_probes,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
    if (!ix || (nq && (!queries || !out_n)) || (nq && k && (!out_ids || !out_scores))) return fail(VDB_ERR_INVALID_ARG, "null argument");
    VDB_NO_GROUP(ix, "search_multi_entry");
    if (nq == 0) return VDB_OK;
    if (ix->pcomm) return fail(VDB_ERR_UNSUPPORTED, "search_multi_entry: not available on a member of a process group");
    std::lock_guard<vdb::IndexMutex> g(ix->mu);
    VDB_ENTER(ix);
    if (!ix->graph_valid) return fail(VDB_ERR_STATE, "HNSW graph not built for all rows (use mode BRUTE or build it)");
    // NativeHnsw level: ef_search goes to search_layer AS GIVEN (graph.rs:343) — no SearchQuality rule, no max(ef, k): a call with
    // ef_search < k returns at most ef_search results (more entry points than ef_search: that many, graph.rs:463-468)
    // (ef_search = 0 is legal there and acts as 1: the entry point is pushed uncut and every later push pops one)
    const uint32_t draws = (num_probes > 1 && ix->graph_nodes > 10) ? std::min<uint32_t>(num_probes, 4) - 1 : 0;
    const uint32_t* d_extra = nullptr;
    if (draws) {
      std::vector<uint32_t> extra((size_t)nq * 3, 0xFFFFFFFFu);
      for (uint32_t q = 0; q < nq; q++)
        for (uint32_t p = 0; p < draws; p++) {
          uint64_t s = ix->rng_state;  // graph.rs:320-334 (no zero-state reseed here)
          s ^= s << 13;
          s ^= s >> 7;
          s ^= s << 17;
          ix->rng_state = s;
          extra[(size_t)q * 3 + p] = (uint32_t)(s % ix->graph_nodes);
        }
      if (ix->s_part_cnt.reserve(extra.size() * 4, false, ix->stream) != hipSuccess) return fail(VDB_ERR_OOM, "entry-point scratch");
      VDB_HIP(hipMemcpyAsync(ix->s_part_cnt.p, extra.data(), extra.size() * 4, hipMemcpyHostToDevice, ix->stream));
      VDB_HIP(hipStreamSynchronize(ix->stream));  // `extra` is host memory
      d_extra = ix->s_part_cnt.as<uint32_t>();
    }
    int32_t rc = stage_queries(ix, queries, 0, nq, nq);
    if (rc != VDB_OK) return rc;
    struct RawEf {  // (exclusive lock held: nobody else reads the flag; reset on every way out, an exception caught by guarded() included)
      vdb_hip_index* h;
      explicit RawEf(vdb_hip_index* x) : h(x) { h->raw_ef = true; }
      ~RawEf() { h->raw_ef = false; }
    };
    {
      RawEf raw(ix);
      rc = search_staged(ix, nq, k, ef, VDB_SEARCH_HNSW, 0, d_extra);
    }
    if (rc != VDB_OK) return rc;
    deliver_slice(ix, 0, nq, nq, k, out_ids, out_scores, out_n);
    return VDB_OK;
  });
}

int32_t vdb_hip_index_combine_stats(vdb_hip_index* ix, uint64_t* launches, uint64_t* calls, uint64_t* queries, uint64_t* max_batch) {
  return vdb::guarded([&]() -> int32_t {
    if (!ix) return fail(VDB_ERR_INVALID_ARG, "null argument");
    uint64_t v[4] = {0, 0, 0, 0};
    auto add = [&](vdb_hip_index* h) {
      if (!h->combiner) return;
      std::lock_guard<std::mutex> lk(h->combiner->mu);
      v[0] += h->combiner->launches;
      v[1] += h->combiner->calls;
      v[2] += h->combiner->queries;
      v[3] = std::max(v[3], h->combiner->max_batch);
    };
    if (ix->group)
      for (size_t s = 0; s < group_size(ix); s++) add(group_shard(ix, s));
    else
      add(ix);
    if (launches) *launches = v[0];
    if (calls) *calls = v[1];
    if (queries) *queries = v[2];
    if (max_batch) *max_batch = v[3];
    return VDB_OK;
  });
}

}  // extern "C"
