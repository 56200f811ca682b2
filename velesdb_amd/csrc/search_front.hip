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
