// hybrid.hip — Collection::hybrid_search / hybrid_search_with_filter (collection/search/text.rs:113-299) on the device:
// hybrid_fuse_kernel, its form with one optional filter per query hybrid_fuse_filters_kernel (one body, hybrid_fuse_block),
// their launchers and the stand-alone entry point vdb_hip_hybrid_fuse.  The rule itself is vdb_hybrid.hpp (shared with the host model
// of the CPU tier); DESIGN 4.1p.
//
// One block per user query.  The query's records sit in LDS as 16-byte (list << 13 | position, live, id) entries, as in fusion.hip:
//   1. filtered form only: every thread looks at eight consecutive text hits, a block-wide scan of the kept counts gives every kept
//      hit its rank — a stable compaction, done BEFORE ranks exist;
//   2. the vector list (from the walk's result block, at its stride) and the text hits into LDS;
//   3. bitonic sort over the power-of-two padded count by (64-bit id, list, position) — an id's occurrences become one run, V before T,
//      a list's positions ascending;
//   4. every thread looks at eight consecutive entries; the head of a run folds it through hybrid::fuse_run;
//   5. a block-wide scan of the head counts compacts the fused records to the front of the same LDS array;
//   6. bitonic sort of the padded records by (total-order score descending, id descending);
//   7. unfiltered form on a handle only: of the first min(k, distinct ids) the ones that are not live are compacted away (one more scan);
//   8. the output, padded as every search pads (id ~0, score NaN).
// The dynamic LDS of a launch is sized to the largest query of the call (records padded to a power of two, x 16 B, + one u32 per
// thread for the scans), the block to an eighth of that (64..1024 threads), as fuse_launch sizes fuse_lists_kernel.
// The bitonic network and the scan are vdb_lds_sort.hpp's, shared with fusion.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vdb_hybrid.hpp"
#include "vdb_index.hpp"
#include "vdb_kernels.hpp"
#include "vdb_lds_sort.hpp"

namespace vdb {

using fusion::Rec;

constexpr uint32_t kHybridItems = 8;  // LDS entries (and text hits) per thread

// exclusive prefix sum of v over the block's threads, *total = the block's sum.  Every thread of the block calls it; the barrier in
// front ends whatever the block read from LDS (the records, or scan in an earlier use) before
__device__ __forceinline__ uint32_t hybrid_scan(uint32_t* __restrict__ scan, uint32_t v, uint32_t tid, uint32_t nt, uint32_t* total) {
  __syncthreads();
  lds_scan(scan, v, tid, nt);
  *total = scan[nt - 1];
  return scan[tid] - v;
}

// The body of both kernels below, for one block = one user query.  g: the query's vector list and HybridQuery in the launch's
// arrays; q: its row in the call's text and output arrays (hybrid_fuse_kernel: q = g).  filtered, filter_bits and filter_rows are
// uniform over the block: the launch's (hybrid_fuse_kernel) or the query's own (hybrid_fuse_filters_kernel).  The bitmap pointer is
// typed as a global address, so that the per-hit read is a global load whichever kernel the pointer came from.
typedef const __attribute__((address_space(1))) uint32_t* hybrid_glb_u32_p;
__device__ __forceinline__ void hybrid_fuse_block(const HybridArgs& a, const uint32_t g, const uint32_t q, const bool filtered,
                                                  const hybrid_glb_u32_p filter_bits, const uint32_t filter_rows) {
  extern __shared__ Rec hybrid_recs[];  // [a.lds_records] entries, then [blockDim.x] u32
  Rec* recs = hybrid_recs;
  uint32_t* scan = reinterpret_cast<uint32_t*>(hybrid_recs + a.lds_records);
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const HybridQuery Q = a.queries[g];
  const uint32_t nv = Q.nv, ntx = Q.nt;
  const size_t ob = (size_t)q * (a.k ? a.k : 1u);
  const float nan = fusion::u2f(0x7FC00000u);
  // (nv + ntx > lds_records cannot happen: the host sized the launch by the largest query; then also ntx <= nt * kHybridItems)
  bool nothing = a.k == 0 || nv + ntx == 0 || nv + ntx > a.lds_records;
  uint32_t n = nv + ntx;

  if (!nothing) {
    // the text hits of this thread: [tid * 8, tid * 8 + 8)
    const size_t tb = (size_t)q * a.text_stride;
    uint32_t keep = 0, live = 0, cnt = 0;
#pragma unroll
    for (uint32_t e = 0; e < kHybridItems; e++) {
      const uint32_t i = tid * kHybridItems + e;
      if (i >= ntx) continue;
      uint32_t flags = hybrid::kTextLive | hybrid::kTextAllowed;  // (no row table: caller lists, all live)
      if (a.text_rows) {
        const uint32_t row = a.text_rows[tb + i];  // ~0u: the handle does not know the id
        const bool lv = row < a.n_rows && (!a.alive || a.alive[row] != 0);
        const bool al = lv && filtered && row < filter_rows && ((filter_bits[row >> 5] >> (row & 31u)) & 1u);
        flags = (lv ? hybrid::kTextLive : 0u) | (al ? hybrid::kTextAllowed : 0u);
      }
      if (hybrid::text_ranked(flags, filtered)) {
        keep |= 1u << e;
        cnt++;
      }
      if (flags & hybrid::kTextLive) live |= 1u << e;
    }
    uint32_t pos = tid * kHybridItems, kept = ntx;
    if (filtered) pos = hybrid_scan(scan, cnt, tid, nt, &kept);  // stable compaction: ranks exist only behind it
    n = nv + kept;
    if (n == 0) {
      nothing = true;
    } else {
#pragma unroll
      for (uint32_t e = 0; e < kHybridItems; e++) {
        if (!(keep & (1u << e))) continue;
        const uint32_t p = filtered ? pos++ : pos + e;  // < kept <= ntx
        recs[nv + p] = hybrid::rec_of(1u, p, (live >> e) & 1u, a.text_ids[tb + tid * kHybridItems + e]);
      }
      const size_t vb = (size_t)g * a.vec_stride;
      for (uint32_t p = tid; p < nv; p += nt) recs[p] = hybrid::rec_of(0u, p, true, a.vec_ids[vb + p]);
    }
  }
  if (nothing) {  // (uniform over the block: k, the query's counts and the scan's total)
    for (uint32_t e = tid; e < a.k; e += nt) {
      a.out_ids[ob + e] = ~0ull;
      a.out_scores[ob + e] = nan;
    }
    if (tid == 0) a.out_n[q] = 0;
    return;
  }
  const uint32_t P = lds_pow2(n);  // <= lds_records (a power of two >= the largest nv + ntx)
  for (uint32_t i = n + tid; i < P; i += nt) recs[i] = Rec{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // behind every record, id ~0 included
  __syncthreads();
  lds_bitonic(recs, P, tid, nt, [](const Rec& x, const Rec& y) { return fusion::rec_less<false>(x, y); });

  // heads of the id runs -> fused records in registers
  const float w = Q.w, tw = hybrid::text_weight(Q.w);
  uint32_t fs[kHybridItems], fz[kHybridItems], fw[kHybridItems];
  uint32_t heads = 0, alive_heads = 0, cnt = 0;
#pragma unroll
  for (uint32_t e = 0; e < kHybridItems; e++) {
    const uint32_t i = tid * kHybridItems + e;
    fs[e] = fz[e] = fw[e] = 0;
    if (i < n) {
      const Rec r = recs[i];
      bool head = i == 0;
      if (!head) {
        const Rec q = recs[i - 1];
        head = q.z != r.z || q.w != r.w;
      }
      if (head) {
        uint32_t run, lv;
        const float s = hybrid::fuse_run([&](uint32_t j) { return recs[j]; }, i, n, w, tw, &run, &lv);
        fs[e] = fusion::f2u(s);
        fz[e] = r.z;
        fw[e] = r.w;
        heads |= 1u << e;
        alive_heads |= (lv & 1u) << e;
        cnt++;
      }
    }
  }
  uint32_t D;  // distinct ids, 1 <= D <= n
  uint32_t d = hybrid_scan(scan, cnt, tid, nt, &D);  // (its first barrier: every run has been read, the array may be overwritten)
#pragma unroll
  for (uint32_t e = 0; e < kHybridItems; e++)
    if (heads & (1u << e)) recs[d++] = hybrid::fused_of(fusion::u2f(fs[e]), (alive_heads >> e) & 1u, fz[e], fw[e]);  // d <= tid * 8 + e < n
  const uint32_t P2 = lds_pow2(D);
  for (uint32_t i = D + tid; i < P2; i += nt) recs[i] = hybrid::fused_pad();
  __syncthreads();
  lds_bitonic(recs, P2, tid, nt, [](const Rec& x, const Rec& y) { return hybrid::fused_less(x, y); });

  const uint32_t m = min(a.k, D);  // the cut
  uint32_t written = m;
  if (a.text_rows && !filtered) {
    // the survivors of the cut that are not live leave the output; the others keep their order (m <= D <= nt * 8)
    uint32_t lv = 0, c = 0;
#pragma unroll
    for (uint32_t e = 0; e < kHybridItems; e++) {
      const uint32_t i = tid * kHybridItems + e;
      if (i < m && recs[i].y) {
        lv |= 1u << e;
        c++;
      }
    }
    uint32_t o = hybrid_scan(scan, c, tid, nt, &written);
#pragma unroll
    for (uint32_t e = 0; e < kHybridItems; e++) {
      if (!(lv & (1u << e))) continue;
      const Rec r = recs[tid * kHybridItems + e];
      a.out_ids[ob + o] = fusion::rec_id(r);  // o < written <= m <= k
      a.out_scores[ob + o] = fusion::u2f(hybrid::fused_score_bits(r));
      o++;
    }
  } else {
    for (uint32_t e = tid; e < m; e += nt) {
      const Rec r = recs[e];
      a.out_ids[ob + e] = fusion::rec_id(r);
      a.out_scores[ob + e] = fusion::u2f(hybrid::fused_score_bits(r));
    }
  }
  for (uint32_t e = written + tid; e < a.k; e += nt) {
    a.out_ids[ob + e] = ~0ull;
    a.out_scores[ob + e] = nan;
  }
  if (tid == 0) a.out_n[q] = written;
}

__global__ void __launch_bounds__(1024) hybrid_fuse_kernel(const HybridArgs a) {
  hybrid_fuse_block(a, blockIdx.x, blockIdx.x, a.filtered != 0, (hybrid_glb_u32_p)a.filter_bits, a.filter_rows);
}

// One optional filter PER QUERY (vdb_hip_index_hybrid_search_filters): block b serves slot b of the launch — vector list
// and HybridQuery b, the text hits and the output row of call position slots[b].query, the filter descs[slots[b].filter] (entry
// n_filters: none, the unfiltered form).  The slot and the descriptor are the same for every thread of the block; the descriptor's
// bitmap pointer comes out of memory, so it is made wave-uniform and a global address by hand (as hnsw_filtered.hip's uniform_ptr).
__global__ void __launch_bounds__(1024) hybrid_fuse_filters_kernel(const HybridFiltersArgs fa) {
  const HybridSlot s = fa.slots[blockIdx.x];
  const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.filter);
  const bool filtered = f < fa.n_filters;
  const HybridFilterDesc d = fa.descs[filtered ? f : fa.n_filters];
  const uint64_t bp = (uint64_t)d.bits;
  const hybrid_glb_u32_p bits = (hybrid_glb_u32_p)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bp >> 32)) << 32) |
                                                   (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bp));
  hybrid_fuse_block(fa.h, blockIdx.x, (uint32_t)__builtin_amdgcn_readfirstlane((int)s.query), filtered, bits,
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)d.rows));
}

// The per-query table of a call from the list lengths and weights (host): the ONE validation of both entry points.  weights null =
// 0.5 for every query.  vec_n null: the vector lists do not exist yet (the index entry point, before its walks) — every query is
// planned with the vec_stride ids its walk may return, and the caller sets nv behind the walk.  A NaN weight and a list longer than
// its stride are INVALID, a query past VDB_HYBRID_MAX_RECORDS is UNSUPPORTED: decided here, before anything runs.
int32_t hybrid_plan(const uint32_t* vec_n, uint64_t vec_stride, const uint32_t* text_n, uint32_t text_stride, const float* weights, uint32_t nq,
                    std::vector<HybridQuery>* queries, uint32_t* max_records) {
  queries->assign(nq, HybridQuery{0, 0, 0.0f, 0});
  uint32_t most = 0;
  for (uint32_t i = 0; i < nq; i++) {
    const float w = weights ? weights[i] : hybrid::kDefaultWeight;
    if (!hybrid::weight_valid(w)) return fail(VDB_ERR_INVALID_ARG, "hybrid: vector_weight of query " + std::to_string(i) + " is NaN");
    const uint64_t nv = vec_n ? vec_n[i] : vec_stride;
    if (nv > vec_stride)
      return fail(VDB_ERR_INVALID_ARG, "hybrid: the vector list of query " + std::to_string(i) + " holds " + std::to_string(nv) +
                                           " ids, vec_stride is " + std::to_string(vec_stride));
    if (text_n[i] > text_stride)
      return fail(VDB_ERR_INVALID_ARG, "hybrid: the text list of query " + std::to_string(i) + " holds " + std::to_string(text_n[i]) +
                                           " ids, text_stride is " + std::to_string(text_stride));
    const uint64_t n = nv + text_n[i];
    if (n > VDB_HYBRID_MAX_RECORDS)
      return fail(VDB_ERR_UNSUPPORTED, "hybrid: query " + std::to_string(i) + " would fuse a vector list of " + (vec_n ? "" : "up to ") +
                                           std::to_string(nv) + " ids and " + std::to_string(text_n[i]) + " text hits, more than the " +
                                           std::to_string(VDB_HYBRID_MAX_RECORDS) + " records one block's LDS takes");
    (*queries)[i] = HybridQuery{(uint32_t)nv, text_n[i], hybrid::clamp_weight(w), 0};
    most = std::max(most, (uint32_t)n);
  }
  *max_records = most;
  return VDB_OK;
}

// one launch for nq queries; the LDS array of the launch is sized here (max_records = the largest query's nv + nt,
// <= VDB_HYBRID_MAX_RECORDS: hybrid_plan) and handed to the kernel in args_of(a).lds_records
template <class Args, class Kernel, class ArgsOf>
static int32_t hybrid_launch_of(Kernel kernel, const char* name, Args a, ArgsOf&& args_of, uint32_t nq, uint32_t max_records, hipStream_t st) {
  if (nq == 0) return VDB_OK;
  uint32_t P = 1;
  while (P < max_records) P <<= 1;
  args_of(a).lds_records = P;
  const uint32_t nt = std::min<uint32_t>(1024, std::max<uint32_t>(64, P / kHybridItems));  // nt * kHybridItems >= P
  const size_t lds = (size_t)P * sizeof(Rec) + (size_t)nt * 4;
  static_assert((size_t)VDB_HYBRID_MAX_RECORDS * sizeof(Rec) + 1024 * 4 <= 160 * 1024, "the largest query must fit the CU's LDS");
  static_assert(VDB_HYBRID_MAX_RECORDS <= 1024 * kHybridItems && VDB_HYBRID_MAX_RECORDS <= (1u << fusion::kPosBits), "eight records per thread; 13 position bits");
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string(name) + " LDS attribute: " + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(nq), dim3(nt), lds, st, a);
  VDB_HIP(hipGetLastError());
  return VDB_OK;
}
int32_t hybrid_launch(HybridArgs a, uint32_t nq, uint32_t max_records, hipStream_t st) {
  return hybrid_launch_of(hybrid_fuse_kernel, "hybrid_fuse_kernel", a, [](HybridArgs& x) -> HybridArgs& { return x; }, nq, max_records, st);
}
// the per-query form: nq = the slots of the launch (fa.slots, fa.h.vec_ids and fa.h.queries hold one entry per slot)
int32_t hybrid_filters_launch(HybridFiltersArgs fa, uint32_t nq, uint32_t max_records, hipStream_t st) {
  return hybrid_launch_of(hybrid_fuse_filters_kernel, "hybrid_fuse_filters_kernel", fa, [](HybridFiltersArgs& x) -> HybridArgs& { return x.h; }, nq,
                          max_records, st);
}

namespace {
struct TmpDev {
  void* p = nullptr;
  ~TmpDev() {
    if (p) (void)hipFree(p);
  }
};
}  // namespace

}  // namespace vdb

using namespace vdb;

extern "C" {

// the hybrid rule alone over caller lists, all ids live, no filter; host pointers, one launch (include/velesdb_hip.h)
int32_t vdb_hip_hybrid_fuse(int32_t device, const uint64_t* vec_ids, const uint32_t* vec_n, uint32_t vec_stride, const uint64_t* text_ids,
                            const uint32_t* text_n, uint32_t text_stride, const float* vector_weights, uint32_t nq, uint32_t k,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
    if ((nq && (!vec_n || !text_n || !out_n)) || (nq && k && (!out_ids || !out_scores)) || (nq && vec_stride && !vec_ids) ||
        (nq && text_stride && !text_ids))
      return fail(VDB_ERR_INVALID_ARG, "null argument");
    std::vector<HybridQuery> queries;
    uint32_t most = 0;
    int32_t rc = hybrid_plan(vec_n, vec_stride, text_n, text_stride, vector_weights, nq, &queries, &most);
    if (rc != VDB_OK) return rc;
    if (nq == 0) return VDB_OK;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
      (void)hipGetLastError();
      return fail(VDB_ERR_NO_DEVICE, "no HIP device visible (hipGetDeviceCount)");
    }
    if (device < 0 || device >= n_dev) return fail(VDB_ERR_INVALID_ARG, "bad device ordinal");
    VDB_HIP(hipSetDevice(device));

    // one device block: vector ids | text ids | queries | out ids | out scores | out n (every part 16-byte aligned)
    const size_t kk = std::max<uint32_t>(k, 1);
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t vcells = (size_t)nq * vec_stride, tcells = (size_t)nq * text_stride;
    const size_t o_tx = up16(vcells * 8), o_q = o_tx + up16(tcells * 8), o_oi = o_q + up16((size_t)nq * sizeof(HybridQuery)),
                 o_os = o_oi + up16((size_t)nq * kk * 8), o_on = o_os + up16((size_t)nq * kk * 4), total = o_on + up16((size_t)nq * 4);
    TmpDev blk;
    VDB_HIP(hipMalloc(&blk.p, total));
    unsigned char* b = static_cast<unsigned char*>(blk.p);
    if (vcells) VDB_HIP(hipMemcpy(b, vec_ids, vcells * 8, hipMemcpyHostToDevice));
    if (tcells) VDB_HIP(hipMemcpy(b + o_tx, text_ids, tcells * 8, hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(b + o_q, queries.data(), queries.size() * sizeof(HybridQuery), hipMemcpyHostToDevice));
    HybridArgs a{};
    a.vec_ids = reinterpret_cast<const uint64_t*>(b);
    a.vec_stride = vec_stride;
    a.text_ids = reinterpret_cast<const uint64_t*>(b + o_tx);
    a.text_stride = text_stride;
    a.queries = reinterpret_cast<const HybridQuery*>(b + o_q);
    a.k = k;
    a.out_ids = reinterpret_cast<uint64_t*>(b + o_oi);
    a.out_scores = reinterpret_cast<float*>(b + o_os);
    a.out_n = reinterpret_cast<uint32_t*>(b + o_on);
    rc = hybrid_launch(a, nq, most, nullptr);
    if (rc != VDB_OK) return rc;
    std::vector<unsigned char> h(total - o_oi);  // the outputs are written only once everything has come back
    VDB_HIP(hipMemcpy(h.data(), b + o_oi, h.size(), hipMemcpyDeviceToHost));
    if (k) {
      std::memcpy(out_ids, h.data(), (size_t)nq * k * 8);
      std::memcpy(out_scores, h.data() + (o_os - o_oi), (size_t)nq * k * 4);
    }
    std::memcpy(out_n, h.data() + (o_on - o_oi), (size_t)nq * 4);
    return VDB_OK;
  });
}

}  // extern "C"
