// fusion.hip — FusionStrategy::fuse (fusion/strategy.rs:138-300) on the device: fuse_lists_kernel, its launcher and the stand-alone
// entry point vdb_hip_fuse_results.  The rule itself is vdb_fusion.hpp (shared with the host model of the CPU tier); DESIGN 4.1j.
//
// One block per group of lists.  The group's records sit in LDS as 16-byte (id, list ordinal << 13 | position, score) entries:
//   1. bitonic sort over the power-of-two padded count by (64-bit id, list, position) — an id's occurrences become one run, its lists in
//      ascending order, a list's positions in ascending order;
//   2. every thread looks at eight consecutive entries; the head of a run folds the run through fusion::fuse_run (a run has at most
//      one entry per list plus in-list duplicates) and keeps (fused score, id) in registers;
//   3. a block-wide scan of the head counts compacts the fused pairs to the front of the same LDS array;
//   4. bitonic sort of the padded pairs by (total-order score descending, id ascending), the first min(top_k, distinct ids) go out.
// The dynamic LDS of a launch is sized to the largest group of the call (records padded to a power of two, x 16 B, + one u32 per
// thread for the scan), the block to an eighth of that (64..1024 threads): launches of small groups share a CU.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vdb_fusion.hpp"
#include "vdb_index.hpp"
#include "vdb_kernels.hpp"
#include "vdb_lds_sort.hpp"

namespace vdb {

using fusion::Rec;

constexpr uint32_t kFuseItems = 8;  // LDS entries per thread in step 2

// (the network and the scan: vdb_lds_sort.hpp, shared with hybrid.hip)
template <bool BY_SCORE>
__device__ __forceinline__ void fuse_bitonic(Rec* __restrict__ recs, uint32_t P, uint32_t tid, uint32_t nt) {
  lds_bitonic(recs, P, tid, nt, [](const Rec& a, const Rec& b) { return fusion::rec_less<BY_SCORE>(a, b); });
}

__global__ void __launch_bounds__(1024) fuse_lists_kernel(const FuseArgs a) {
  extern __shared__ Rec fuse_recs[];  // [a.lds_records] entries, then [blockDim.x] u32
  Rec* recs = fuse_recs;
  uint32_t* scan = reinterpret_cast<uint32_t*>(fuse_recs + a.lds_records);
  const uint32_t tid = threadIdx.x, nt = blockDim.x, g = blockIdx.x;
  const FuseGroup G = a.groups[g];
  const uint32_t n = G.n;
  const size_t ob = (size_t)g * (a.top_k ? a.top_k : 1u);
  const float nan = fusion::u2f(0x7FC00000u);
  if (n == 0 || a.top_k == 0 || n > a.lds_records) {  // (n > lds_records cannot happen: the host sized the launch by the largest group)
    for (uint32_t e = tid; e < a.top_k; e += nt) {
      a.out_ids[ob + e] = ~0ull;
      a.out_scores[ob + e] = nan;
    }
    if (tid == 0) a.out_n[g] = 0;
    return;
  }
  const uint32_t P = lds_pow2(n);  // <= lds_records (a power of two >= the largest n)

  // the group's lists into LDS: one wave per list, lanes over its positions
  for (uint32_t l = tid >> 6; l < G.V; l += nt >> 6) {
    const FuseList L = a.lists[G.first + l];
    const size_t base = (size_t)(G.first + l) * a.list_stride;
    for (uint32_t pos = tid & 63u; pos < L.n; pos += 64) {
      const uint64_t id = a.ids[base + pos];
      const uint32_t at = L.off + pos;  // < n by the host's prefix sums
      if (at < n) recs[at] = Rec{(L.ord << fusion::kPosBits) | pos, fusion::f2u(a.scores[base + pos]), (uint32_t)id, (uint32_t)(id >> 32)};
    }
  }
  for (uint32_t i = n + tid; i < P; i += nt) recs[i] = Rec{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // behind every record, id ~0 included
  __syncthreads();
  fuse_bitonic<false>(recs, P, tid, nt);

  // heads of the id runs -> fused pairs in registers
  uint32_t fy[kFuseItems], fz[kFuseItems], fw[kFuseItems];
  uint32_t heads = 0, cnt = 0;
#pragma unroll
  for (uint32_t e = 0; e < kFuseItems; e++) {
    const uint32_t i = tid * kFuseItems + e;
    fy[e] = fz[e] = fw[e] = 0;
    if (i < n) {
      const Rec r = recs[i];
      bool head = i == 0;
      if (!head) {
        const Rec q = recs[i - 1];
        head = q.z != r.z || q.w != r.w;
      }
      if (head) {
        uint32_t run;
        const float s = fusion::fuse_run([&](uint32_t j) { return recs[j]; }, i, n, a.strategy, a.rrf_k, G.V, a.w_avg, a.w_max, a.w_hit, &run);
        fy[e] = fusion::f2u(s);
        fz[e] = r.z;
        fw[e] = r.w;
        heads |= 1u << e;
        cnt++;
      }
    }
  }
  lds_scan(scan, cnt, tid, nt);  // (behind its first barrier every run has been read: the array may be overwritten from here on)
  const uint32_t D = scan[nt - 1];  // distinct ids, 1 <= D <= n
  uint32_t d = scan[tid] - cnt;
#pragma unroll
  for (uint32_t e = 0; e < kFuseItems; e++)
    if (heads & (1u << e)) recs[d++] = Rec{fusion::desc_key(fy[e]), fy[e], fz[e], fw[e]};  // d <= tid * 8 + e < n
  const uint32_t P2 = lds_pow2(D);
  for (uint32_t i = D + tid; i < P2; i += nt) recs[i] = Rec{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  __syncthreads();
  fuse_bitonic<true>(recs, P2, tid, nt);

  const uint32_t m = min(a.top_k, D);
  for (uint32_t e = tid; e < a.top_k; e += nt) {
    if (e < m) {
      const Rec r = recs[e];
      a.out_ids[ob + e] = fusion::rec_id(r);
      a.out_scores[ob + e] = fusion::u2f(r.y);
    } else {
      a.out_ids[ob + e] = ~0ull;
      a.out_scores[ob + e] = nan;
    }
  }
  if (tid == 0) a.out_n[g] = m;
}

// strategy and weights of a call -> w[3]; the messages are FusionError's (strategy.rs:23-34)
int32_t fuse_check_strategy(int32_t strategy, const float* weights, float* w) {
  w[0] = w[1] = w[2] = 0.0f;
  if (strategy < VDB_FUSION_AVERAGE || strategy > VDB_FUSION_WEIGHTED)
    return fail(VDB_ERR_INVALID_ARG, "fusion: strategy " + std::to_string(strategy) + " is none of AVERAGE (0), MAXIMUM (1), RRF (2), WEIGHTED (3)");
  if (strategy != VDB_FUSION_WEIGHTED) return VDB_OK;
  if (!weights) return fail(VDB_ERR_INVALID_ARG, "fusion: VDB_FUSION_WEIGHTED needs weights[3] = avg, max, hit");
  const int e = fusion::weights_error(weights[0], weights[1], weights[2]);
  if (e == 1) return fail(VDB_ERR_INVALID_ARG, "fusion: Weights must be non-negative");
  if (e == 2) return fail(VDB_ERR_INVALID_ARG, "fusion: Weights must sum to 1.0, got " + std::to_string((weights[0] + weights[1]) + weights[2]));
  w[0] = weights[0];
  w[1] = weights[1];
  w[2] = weights[2];
  return VDB_OK;
}

// the per-list and per-group tables of a call from the list lengths (host): where a list's records go in its group's LDS array,
// its ordinal among the group's non-empty lists.  A group past VDB_FUSE_MAX_RECORDS is refused here, before anything runs.
int32_t fuse_plan(const uint32_t* list_n, uint32_t n_lists, uint32_t list_stride, const uint32_t* group_sizes, uint32_t n_groups,
                  std::vector<FuseList>* lists, std::vector<FuseGroup>* groups, uint32_t* max_records) {
  uint64_t sum = 0;
  for (uint32_t g = 0; g < n_groups; g++) sum += group_sizes[g];
  if (sum != n_lists)
    return fail(VDB_ERR_INVALID_ARG, "fusion: group_sizes sum to " + std::to_string(sum) + ", the call holds " + std::to_string(n_lists) + " lists");
  lists->assign(n_lists, FuseList{0, 0, 0, 0});
  groups->assign(n_groups, FuseGroup{0, 0, 0, 0});
  uint32_t first = 0, most = 0;
  for (uint32_t g = 0; g < n_groups; g++) {
    uint64_t off = 0;
    uint32_t ord = 0;
    for (uint32_t l = first; l < first + group_sizes[g]; l++) {
      if (list_n[l] > list_stride)
        return fail(VDB_ERR_INVALID_ARG, "fusion: list " + std::to_string(l) + " holds " + std::to_string(list_n[l]) + " records, list_stride is " +
                                             std::to_string(list_stride));
      (*lists)[l] = FuseList{list_n[l], (uint32_t)off, ord, 0};
      off += list_n[l];
      if (list_n[l]) ord++;
      if (off > VDB_FUSE_MAX_RECORDS)
        return fail(VDB_ERR_UNSUPPORTED, "fusion: group " + std::to_string(g) + " holds more than " + std::to_string(VDB_FUSE_MAX_RECORDS) +
                                             " records (what one block's LDS takes)");
    }
    (*groups)[g] = FuseGroup{first, group_sizes[g], (uint32_t)off, 0};
    most = std::max(most, (uint32_t)off);
    first += group_sizes[g];
  }
  *max_records = most;
  return VDB_OK;
}

// one launch for n_groups groups; a.lds_records is set here (max_records = the largest group's record count, <= VDB_FUSE_MAX_RECORDS)
int32_t fuse_launch(FuseArgs a, uint32_t n_groups, uint32_t max_records, hipStream_t st) {
  if (n_groups == 0) return VDB_OK;
  if (max_records > VDB_FUSE_MAX_RECORDS) return fail(VDB_ERR_UNSUPPORTED, "fusion: a group past the LDS");
  uint32_t P = 1;
  while (P < max_records) P <<= 1;
  a.lds_records = P;
  const uint32_t nt = std::min<uint32_t>(1024, std::max<uint32_t>(64, P / kFuseItems));  // nt * kFuseItems >= P
  const size_t lds = (size_t)P * sizeof(Rec) + (size_t)nt * 4;
  static_assert((size_t)VDB_FUSE_MAX_RECORDS * sizeof(Rec) + 1024 * 4 <= 160 * 1024, "the largest group must fit the CU's LDS");
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fuse_lists_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("fuse_lists_kernel LDS attribute: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(fuse_lists_kernel, dim3(n_groups), dim3(nt), lds, st, a);
  VDB_HIP(hipGetLastError());
  return VDB_OK;
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

// FusionStrategy::fuse for n_groups independent groups of lists, host pointers (include/velesdb_hip.h)
int32_t vdb_hip_fuse_results(int32_t device, int32_t strategy, uint32_t rrf_k, const float* weights, const uint64_t* ids, const float* scores,
                             const uint32_t* list_n, uint32_t n_lists, uint32_t list_stride, const uint32_t* group_sizes, uint32_t n_groups,
                             uint32_t top_k, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
  return vdb::guarded([&]() -> int32_t {
    if ((n_groups && (!group_sizes || !out_n)) || (n_groups && top_k && (!out_ids || !out_scores)) || (n_lists && !list_n) ||
        (n_lists && list_stride && (!ids || !scores)))
      return fail(VDB_ERR_INVALID_ARG, "null argument");
    float w[3];
    int32_t rc = fuse_check_strategy(strategy, weights, w);
    if (rc != VDB_OK) return rc;
    std::vector<FuseList> lists;
    std::vector<FuseGroup> groups;
    uint32_t most = 0;
    rc = fuse_plan(list_n, n_lists, list_stride, group_sizes, n_groups, &lists, &groups, &most);
    if (rc != VDB_OK) return rc;
    if (n_groups == 0) return VDB_OK;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
      (void)hipGetLastError();
      return fail(VDB_ERR_NO_DEVICE, "no HIP device visible (hipGetDeviceCount)");
    }
    if (device < 0 || device >= n_dev) return fail(VDB_ERR_INVALID_ARG, "bad device ordinal");
    VDB_HIP(hipSetDevice(device));

    // one device block: ids | scores | lists | groups | out ids | out scores | out n (every part 16-byte aligned)
    const size_t kk = std::max<uint32_t>(top_k, 1);
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t cells = (size_t)n_lists * list_stride;
    const size_t o_sc = up16(cells * 8), o_li = o_sc + up16(cells * 4), o_gr = o_li + up16(lists.size() * sizeof(FuseList)),
                 o_oi = o_gr + up16(groups.size() * sizeof(FuseGroup)), o_os = o_oi + up16((size_t)n_groups * kk * 8),
                 o_on = o_os + up16((size_t)n_groups * kk * 4), total = o_on + up16((size_t)n_groups * 4);
    TmpDev blk;
    VDB_HIP(hipMalloc(&blk.p, total));
    unsigned char* b = static_cast<unsigned char*>(blk.p);
    if (cells) {
      VDB_HIP(hipMemcpy(b, ids, cells * 8, hipMemcpyHostToDevice));
      VDB_HIP(hipMemcpy(b + o_sc, scores, cells * 4, hipMemcpyHostToDevice));
    }
    if (!lists.empty()) VDB_HIP(hipMemcpy(b + o_li, lists.data(), lists.size() * sizeof(FuseList), hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(b + o_gr, groups.data(), groups.size() * sizeof(FuseGroup), hipMemcpyHostToDevice));
    FuseArgs a{};
    a.ids = reinterpret_cast<const uint64_t*>(b);
    a.scores = reinterpret_cast<const float*>(b + o_sc);
    a.list_stride = list_stride;
    a.lists = reinterpret_cast<const FuseList*>(b + o_li);
    a.groups = reinterpret_cast<const FuseGroup*>(b + o_gr);
    a.strategy = strategy;
    a.rrf_k = rrf_k;
    a.w_avg = w[0];
    a.w_max = w[1];
    a.w_hit = w[2];
    a.top_k = top_k;
    a.out_ids = reinterpret_cast<uint64_t*>(b + o_oi);
    a.out_scores = reinterpret_cast<float*>(b + o_os);
    a.out_n = reinterpret_cast<uint32_t*>(b + o_on);
    rc = fuse_launch(a, n_groups, most, nullptr);
    if (rc != VDB_OK) return rc;
    std::vector<unsigned char> h(total - o_oi);  // the outputs are written only once everything has come back
    VDB_HIP(hipMemcpy(h.data(), b + o_oi, h.size(), hipMemcpyDeviceToHost));
    if (top_k) {
      std::memcpy(out_ids, h.data(), (size_t)n_groups * top_k * 8);
      std::memcpy(out_scores, h.data() + (o_os - o_oi), (size_t)n_groups * top_k * 4);
    }
    std::memcpy(out_n, h.data() + (o_on - o_oi), (size_t)n_groups * 4);
    return VDB_OK;
  });
}

}  // extern "C"
