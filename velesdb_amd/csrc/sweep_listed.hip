// sweep_listed.hip — filtered exact search (vdb_hip_index_search_batch_filtered) and its form with one filter per
// query (vdb_hip_index_search_batch_filters, DESIGN 4.1n: the GROUPED kernels share the arithmetic bodies below).
//
// The caller hands over the set of ids a predicate matched; the filter object holds them as a bitmap and as the ascending list of
// internal rows.  Two routes give the same bits:
//   * the LISTED sweep (this file): the kernels read only the listed rows, gathered whole by index (a row is row_stride floats,
//     16-byte aligned), blocks take contiguous chunks of the list, alive[row] is read where a key would enter a list, block-local
//     top-k lists of 64-bit keys go to part_keys and merge_topk finishes — the cost follows the number of allowed rows;
//   * MASK SUBSTITUTION: filter_mask_kernel writes mask[r] = allowed(r) && alive(r) and the whole exact path runs with that mask
//     in place of the soft-delete flags (index.hip, search_alive).
// The listed sweep has to produce the scores of the unfiltered path bit for bit, so it has the two arithmetic bodies of that path:
//   * mode C (vdb_device.hpp): one wave per row, float4 chunk c on lane c % 64, predicated tails, the xor butterfly — the body of
//     sweep_topk_f32 with the row index taken from the list (Euclidean always; Cosine / DotProduct with the engine off);
//   * mode M (oracle dotM; sweep_topk_mfma_f32): ONE fmaf chain per (row, query) over k = 128 U + 16 m + 4 kk + c in the order
//     U, m, c, kk over the vector zero-padded to a multiple of 128 — a lane owns a (row, query) chain, the rows travel through LDS
//     in steps of 64 elements (split_rerank_verify's scheme, sweep_split.hip), 16 rows in flight per wave.
#include <algorithm>

#include "vdb_device.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

// ---- mode C -------------------------------------------------------------------------------------------------------------
// B queries per pass (1, 4, 8), RPG = 64 / B listed rows per group, CPL = float4 chunks per lane (dim == CPL * 256) or 0 for any
// dim.  Block b owns the groups [b * per_block, (b + 1) * per_block) of the list, its 4 waves take them in turn.
// LDS as sweep_topk_f32: lists[B][k] u64 | cnt[B] | lock[B] | generic-dim query scratch.
// The body is shared by the one-filter kernel and the grouped one: GROUPED says where a block finds its work — query
// b of the pass is row it->q[b] of a.queries and of the partial-list area (else row b), the block sweeps the WHOLE of a.list —
// the item's chunk of the filter's list, handed over as a list of its own — (else its per_block share), and its lists go to slot
// it->slot of the lists_per_q a query owns (else to list blockIdx.x of gridDim.x).  (A sweep that starts at unit 0 keeps the
// register counts of the one-filter kernels; one that started at a unit read from the item, or that derived its end from
// a.count, cost mode M eight more VGPRs.)  What is
// only needed at the end (slot, the query positions) is read there and does not stay live across the sweep.
struct ListedWork {
  const ListedGroupItem* it;
  uint32_t lists_per_q;
};
// a field of the block's item: the same value in every lane, so it belongs in a scalar register
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ ListedWork listed_work_of(const ListedGroupItem* __restrict__ it, uint32_t lists_per_q, ListedArgs* a) {
  const uint64_t lp = reinterpret_cast<uint64_t>(it->list);
  // (a pointer read from memory is a generic one: rebuilt as a GLOBAL pointer, so that the list is read with global_load, not flat_load)
  typedef const __attribute__((address_space(1))) uint32_t* glb_u32_p;
  a->list = (const uint32_t*)(glb_u32_p)(((uint64_t)uniform_u32((uint32_t)(lp >> 32)) << 32) | uniform_u32((uint32_t)lp));
  a->count = uniform_u32(it->count);
  a->nq = uniform_u32(it->nq);
  return ListedWork{it, lists_per_q};
}
// Rows a wave fetches together before it runs their chains (a matter of fetching only: every (row, query) chain is the same
// whatever its companions).  The one-filter kernels take 4.  At 4 rows x CPL float4 next to the 64 accumulators and the B x CPL
// query float4, six instances need more registers than the occupancy the plans size their launches by allows (4 / 3 / 2 blocks
// per CU for B = 1 / 4 / 8): the grouped kernels take 2 rows there (1 in one case), fence the scheduler after each such group
// and ask for the occupancy, and reach it without spilling; the one-filter instances stay as they were.
constexpr bool listed_groups_tight(int metric, int b, int cpl) {
  return (b == 1 && cpl == 4) || (metric == kEuclidean && ((b == 1 && cpl >= 2) || (b == 4 && cpl == 4)));
}
constexpr int listed_rows_in_flight(int metric, int b, int cpl, int rpg, bool grouped) {
  if (!grouped || !listed_groups_tight(metric, b, cpl)) return rpg >= 4 ? 4 : rpg;
  return b == 4 ? 1 : 2;  // (Euclidean, B = 4, CPL = 4: sixteen query float4 stay resident, two rows next to them spilled)
}
// ... and the compiler is told the occupancy there (waves per SIMD = 256-thread blocks per CU); 1 = no request
constexpr int listed_groups_min_waves(int metric, int b, int cpl) { return listed_groups_tight(metric, b, cpl) ? (b == 1 ? 4 : 3) : 1; }
template <int METRIC, int B, int CPL, bool GROUPED>
__device__ __forceinline__ void listed_body_c(const ListedArgs& a, uint32_t per_block, const ListedWork& w) {
  constexpr int OP = (METRIC == kEuclidean) ? kOpL2 : kOpDot;
  constexpr int RPG = 64 / B;
  constexpr bool HIB = higher_is_better(METRIC);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = (int)(threadIdx.x >> 6);
  const uint32_t k = a.k;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(smem + (size_t)B * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(smem + (size_t)B * k * 8 + (size_t)B * 4);
  float* qgen = reinterpret_cast<float*>(smem + ((((size_t)B * k * 8 + (size_t)B * 8) + 15) & ~(size_t)15));  // generic path only
  const uint32_t nq_here = a.nq;
  if (threadIdx.x < B) {
    cnts[threadIdx.x] = 0;
    locks[threadIdx.x] = 0;
  }
  __syncthreads();

  const int d4 = (int)((a.dim + 3) / 4);  // chunks per row
  float4 q[B][CPL > 0 ? CPL : 1];
  float qnorm_mine = 0.0f;  // lane l keeps the norm of query (l % B)
  if (CPL > 0) {
#pragma unroll
    for (int b = 0; b < B; b++) {
      float nacc = 0.0f;
#pragma unroll
      for (int j = 0; j < CPL; j++) {
        q[b][j] = (b < (int)nq_here) ? ld4(a.queries + (GROUPED ? (size_t)w.it->q[b] : (size_t)b) * a.q_stride + (size_t)(j * 64 + lane) * 4)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
        nacc = chain4<kOpDot>(nacc, q[b][j], q[b][j]);
      }
      if (METRIC == kCosine) {
        float n = sqrtf(butterfly_all(nacc));
        if ((lane % B) == b) qnorm_mine = n;
      }
    }
  } else {
    const int qlen = d4 * 4;
    for (int i = threadIdx.x; i < B * qlen; i += 256) {
      int b = i / qlen, e = i % qlen;
      qgen[i] = (b < (int)nq_here && e < (int)a.dim) ? a.queries[(GROUPED ? (size_t)w.it->q[b] : (size_t)b) * a.q_stride + e] : 0.0f;
    }
    __syncthreads();
    if (METRIC == kCosine) {
      for (int b = 0; b < B; b++) {
        float nacc = 0.0f;
        for (int c = lane; c < d4; c += 64) {
          float4 x = ld4(qgen + (size_t)b * qlen + c * 4);
          int nv = (int)a.dim - c * 4;
          nacc = nv >= 4 ? chain4<kOpDot>(nacc, x, x) : chain4_tail<kOpDot>(nacc, x, x, nv);
        }
        float n = sqrtf(butterfly_all(nacc));
        if ((lane % B) == b) qnorm_mine = n;
      }
    }
  }

  const uint32_t ngroups = (a.count + RPG - 1) / RPG;
  const uint32_t g_end = GROUPED ? uniform_u32(w.it->units) : min(ngroups, (blockIdx.x + 1) * per_block);
  for (uint32_t g = (GROUPED ? 0u : blockIdx.x * per_block) + (uint32_t)wib; g < g_end; g += 4) {
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; i++) acc[i] = 0.0f;
    const uint32_t pos0 = g * RPG;
    if (CPL > 0) {
      constexpr int RB = listed_rows_in_flight(METRIC, B, CPL, RPG, GROUPED);  // rows in flight together
#pragma unroll
      for (int r = 0; r < RPG; r += RB) {
        float4 v[RB][CPL > 0 ? CPL : 1];
#pragma unroll
        for (int rr = 0; rr < RB; rr++) {
          uint32_t pos = pos0 + r + rr;
          pos = pos < a.count ? pos : a.count - 1;  // tail of the list: re-read its last row, masked later
          const float* p = a.rows + (size_t)a.list[pos] * a.row_stride + (size_t)lane * 4;
#pragma unroll
          for (int j = 0; j < CPL; j++) v[rr][j] = ld4(p + j * 256);
        }
#pragma unroll
        for (int rr = 0; rr < RB; rr++)
#pragma unroll
          for (int b = 0; b < B; b++) {
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < CPL; j++) s = chain4<OP>(s, q[b][j], v[rr][j]);
            acc[(r + rr) * B + b] = s;
          }
        // (the loops are unrolled into one block: without a fence the scheduler fetches far more rows ahead than RB)
        if (GROUPED && listed_groups_tight(METRIC, B, CPL)) __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      const int qlen = d4 * 4;
#pragma unroll
      for (int r = 0; r < RPG; r++) {
        uint32_t pos = pos0 + r;
        pos = pos < a.count ? pos : a.count - 1;
        const float* p = a.rows + (size_t)a.list[pos] * a.row_stride;
        for (int c = lane; c < d4; c += 64) {
          float4 x = ld4(p + c * 4);
          int nv = (int)a.dim - c * 4;
#pragma unroll
          for (int b = 0; b < B; b++) {
            float4 qq = ld4(qgen + (size_t)b * qlen + c * 4);
            acc[r * B + b] = nv >= 4 ? chain4<OP>(acc[r * B + b], qq, x) : chain4_tail<OP>(acc[r * B + b], qq, x, nv);
          }
        }
      }
    }
    treduce64(acc, lane);
    // lane l now owns pair l: list position pos0 + l / B, query l % B
    const int b = lane % B;
    const uint32_t pos = pos0 + lane / B;
    const bool valid = pos < a.count && b < (int)nq_here;
    const uint32_t row = valid ? a.list[pos] : 0u;
    float vnorm = 1.0f;
    if (METRIC == kCosine && valid) vnorm = a.norms[row];
    const float score = finish_score<METRIC>(acc[0], qnorm_mine, vnorm);
    const uint64_t key = valid ? make_key<HIB>(score, row) : kKeyInvalid;
    const uint32_t c_b = cnts[b];
    const uint64_t tau = (c_b == k) ? lists[(size_t)b * k + (k - 1)] : kKeyInvalid;
    uint64_t mask = __ballot(key < tau);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const uint64_t kk = readlane64(key, src);
      if (a.alive && a.alive[key_row(kk)] == 0) continue;  // soft-deleted since the filter was made
      const int bb = src % B;
      shared_list_offer(lists + (size_t)bb * k, cnts + bb, locks + bb, k, kk, lane);
    }
  }
  // ---- one list per query per block goes to HBM, padded with invalid keys ----
  __syncthreads();
  for (int b = wib; b < (int)nq_here && b < B; b += 4) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + (GROUPED ? (size_t)w.it->q[b] * w.lists_per_q + uniform_u32(w.it->slot) : (size_t)b * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}
template <int METRIC, int B, int CPL>
__global__ __launch_bounds__(256) void sweep_topk_listed(ListedArgs a, uint32_t per_block) {
  listed_body_c<METRIC, B, CPL, false>(a, per_block, ListedWork{});
}
// One filter per query (vdb_hip_index_search_batch_filters): block b does work item b — one chunk of one pass of one
// filter's list (listed_groups_plan, vdb_filter_route.hpp).  The item is read with uniform loads; a.list / count / nq come from it.
template <int METRIC, int B, int CPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(listed_groups_min_waves(METRIC, B, CPL))))
void sweep_topk_listed_groups(ListedArgs a, const ListedGroupItem* __restrict__ items, uint32_t lists_per_q) {
  const ListedWork w = listed_work_of(items + blockIdx.x, lists_per_q, &a);
  listed_body_c<METRIC, B, CPL, true>(a, 0, w);
}

// ---- mode M -------------------------------------------------------------------------------------------------------------
// A block takes 64-row tiles of the list; thread t owns row t % 64 of the tile and the queries t / 64, t / 64 + 4, ... (up to 4 of
// the <= 16 queries of a pass).  LDS: q[nq][dim_pad] f32 | row stage [2][64][68] f32 | lists[nq][k] u64 | cnt[16] | lock[16] |
// query norms [16] | tile rows [64].
constexpr uint32_t kListedMQueries = 16, kListedMTile = 64, kListedMStep = 64, kListedMStride = kListedMStep + 4;
static size_t listed_m_lds_bytes(uint32_t nq, uint32_t k, uint32_t dim) {
  const size_t dim_pad = ((size_t)dim + 127) / 128 * 128;
  return (size_t)nq * dim_pad * 4 + 2 * (size_t)kListedMTile * kListedMStride * 4 + (size_t)nq * k * 8 + 3 * (size_t)kListedMQueries * 4 +
         (size_t)kListedMTile * 4;
}
template <int METRIC, bool GROUPED>
__device__ __forceinline__ void listed_body_m(const ListedArgs& a, uint32_t dim_pad, uint32_t per_block, const ListedWork& w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, k = a.k, nq = a.nq;
  const int lane = lane_id();
  const uint32_t wib = tid >> 6;
  float* qs = reinterpret_cast<float*>(smem);
  float* stage = qs + (size_t)nq * dim_pad;
  unsigned char* after = reinterpret_cast<unsigned char*>(stage + 2 * (size_t)kListedMTile * kListedMStride);
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(after);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(after + (size_t)nq * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(after + (size_t)nq * k * 8 + (size_t)kListedMQueries * 4);
  float* qn = reinterpret_cast<float*>(after + (size_t)nq * k * 8 + 2 * (size_t)kListedMQueries * 4);
  uint32_t* crow = reinterpret_cast<uint32_t*>(after + (size_t)nq * k * 8 + 3 * (size_t)kListedMQueries * 4);
  if (tid < kListedMQueries) {
    cnts[tid] = 0;
    locks[tid] = 0;
  }
  for (uint32_t i = tid; i < nq * dim_pad; i += 256) {
    const uint32_t b = i / dim_pad, e = i % dim_pad;
    qs[i] = e < a.dim ? a.queries[(GROUPED ? (size_t)w.it->q[b] : (size_t)b) * a.q_stride + e] : 0.0f;
  }
  __syncthreads();
  if (METRIC == kCosine) {  // the query norms are the canonical ones (mode C), as in sweep_topk_mfma_f32
    const int d4 = (int)((a.dim + 3) / 4);
    for (uint32_t b = wib; b < nq; b += 4) {
      float nacc = 0.0f;
      for (int c = lane; c < d4; c += 64) {
        const float4 x = ld4(qs + (size_t)b * dim_pad + c * 4);
        const int nv = (int)a.dim - c * 4;
        nacc = nv >= 4 ? chain4<kOpDot>(nacc, x, x) : chain4_tail<kOpDot>(nacc, x, x, nv);
      }
      const float n = sqrtf(butterfly_all(nacc));
      if (lane == 0) qn[b] = n;
    }
    __syncthreads();
  }
  const uint32_t ntiles = (a.count + kListedMTile - 1) / kListedMTile;
  // (GROUPED: an item holds at least one tile — listed_groups_plan emits no empty chunk; saying so keeps the Dot instance at the
  // one-filter kernel's 98 VGPRs, it took 108 without)
  const uint32_t t_end = GROUPED ? max(1u, uniform_u32(w.it->units)) : min(ntiles, (blockIdx.x + 1) * per_block);
  const uint32_t r = tid & 63u;
  float4 v[4];  // 64 rows x 16 float4 per step: 4 per thread, 16 consecutive threads read one row's 256 bytes
  auto fetch = [&](uint32_t U) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t f = tid + 256u * (uint32_t)i;
      const uint32_t fr = f / (kListedMStep / 4), e0 = U + 4 * (f % (kListedMStep / 4));
      float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (e0 < a.dim) {
        w = ld4(a.rows + (size_t)crow[fr] * a.row_stride + e0);
        if (e0 + 4 > a.dim) {  // the vector ends inside this chunk: what follows is the chain's zero padding
          if (e0 + 1 >= a.dim) w.y = 0.0f;
          if (e0 + 2 >= a.dim) w.z = 0.0f;
          w.w = 0.0f;
        }
      }
      v[i] = w;
    }
  };
  auto park = [&](uint32_t buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t f = tid + 256u * (uint32_t)i;
      const uint32_t fr = f / (kListedMStep / 4), c4 = f % (kListedMStep / 4);
      *reinterpret_cast<float4*>(stage + ((size_t)buf * kListedMTile + fr) * kListedMStride + 4 * c4) = v[i];
    }
  };
  for (uint32_t t = GROUPED ? 0u : blockIdx.x * per_block; t < t_end; t++) {
    if (tid < kListedMTile) {
      const uint32_t pos = t * kListedMTile + tid;
      crow[tid] = a.list[pos < a.count ? pos : a.count - 1];  // tail of the list: its last row again, masked below
    }
    __syncthreads();
    fetch(0);
    park(0);
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t U = 0, buf = 0; U < dim_pad; U += kListedMStep, buf ^= 1u) {
      const bool more = U + kListedMStep < dim_pad;
      if (more) fetch(U + kListedMStep);
      const float* x = stage + ((size_t)buf * kListedMTile + r) * kListedMStride;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        float xr[16];
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
          const float4 w = *reinterpret_cast<const float4*>(x + 16 * m + e);
          xr[e] = w.x; xr[e + 1] = w.y; xr[e + 2] = w.z; xr[e + 3] = w.w;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t qi = wib + 4u * (uint32_t)j;
          if (qi < nq) {  // (uniform per wave)
            const float* qq = qs + (size_t)qi * dim_pad + U + 16 * m;
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
              for (int kk = 0; kk < 4; kk++) acc[j] = __builtin_fmaf(xr[4 * kk + c], qq[4 * kk + c], acc[j]);
          }
        }
      }
      if (more) park(buf ^ 1u);
      __syncthreads();
    }
    const bool valid = t * kListedMTile + r < a.count;
    const uint32_t row = crow[r];
    const float vnorm = (METRIC == kCosine && valid) ? a.norms[row] : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t qi = wib + 4u * (uint32_t)j;
      if (qi >= nq) continue;
      const float score = finish_score<METRIC>(acc[j], METRIC == kCosine ? qn[qi] : 0.0f, vnorm);
      const uint64_t key = valid ? make_key<true>(score, row) : kKeyInvalid;
      const uint32_t c_b = cnts[qi];
      const uint64_t tau = (c_b == k) ? lists[(size_t)qi * k + (k - 1)] : kKeyInvalid;
      uint64_t mask = __ballot(key < tau);
      while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t kk = readlane64(key, src);
        if (a.alive && a.alive[key_row(kk)] == 0) continue;  // soft-deleted since the filter was made
        shared_list_offer(lists + (size_t)qi * k, cnts + qi, locks + qi, k, kk, lane);
      }
    }
    __syncthreads();  // the tile's rows (crow) and the stage are rewritten next
  }
  __syncthreads();
  for (uint32_t b = wib; b < nq; b += 4) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + (GROUPED ? (size_t)w.it->q[b] * w.lists_per_q + uniform_u32(w.it->slot) : (size_t)b * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = (uint32_t)lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}
template <int METRIC>
__global__ __launch_bounds__(256) void sweep_topk_listed_m(ListedArgs a, uint32_t dim_pad, uint32_t per_block) {
  listed_body_m<METRIC, false>(a, dim_pad, per_block, ListedWork{});
}
// the grouped form: as sweep_topk_listed_groups, the chunk counted in 64-row tiles; the LDS layout follows the item's nq
template <int METRIC>
__global__ __launch_bounds__(256) void sweep_topk_listed_groups_m(ListedArgs a, uint32_t dim_pad, const ListedGroupItem* __restrict__ items,
                                                                  uint32_t lists_per_q) {
  const ListedWork w = listed_work_of(items + blockIdx.x, lists_per_q, &a);
  listed_body_m<METRIC, true>(a, dim_pad, 0, w);
}

// ---- the row mask of the mask-substitution route: 4 rows per thread, one 32-bit store -----------------------------------------
__global__ __launch_bounds__(256) void filter_mask_kernel(const uint32_t* bitmap, uint32_t f_rows, const uint8_t* alive, uint8_t* mask,
                                                          uint32_t n_rows) {
  const uint32_t r0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (r0 >= n_rows) return;
  const uint32_t w = r0 < f_rows ? bitmap[r0 >> 5] >> (r0 & 31u) : 0u;  // (r0 % 4 == 0: the four bits sit in one word)
  uint32_t out = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) {
    const uint32_t r = r0 + i;
    const bool on = r < n_rows && r < f_rows && ((w >> i) & 1u) && (!alive || alive[r] != 0);
    out |= on ? (1u << (8 * i)) : 0u;
  }
  *reinterpret_cast<uint32_t*>(mask + r0) = out;  // (the buffer is sized to a multiple of 4 past n_rows)
}
void launch_filter_mask(const uint32_t* bitmap, uint32_t f_rows, const uint8_t* alive, uint8_t* mask, uint32_t n_rows, hipStream_t st) {
  const uint32_t quads = (n_rows + 3) / 4;
  hipLaunchKernelGGL(filter_mask_kernel, dim3((quads + 255) / 256), dim3(256), 0, st, bitmap, f_rows, alive, mask, n_rows);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
void sweep_listed_plan(bool mode_m, uint32_t dim, uint32_t k, uint32_t count, uint32_t nq_left, int n_cus, ListedPlan* p) {
  *p = ListedPlan{};
  if (count == 0 || k == 0 || nq_left == 0) return;
  if (mode_m) {
    uint32_t nqp = std::min<uint32_t>(nq_left, kListedMQueries);
    while (nqp > 1 && listed_m_lds_bytes(nqp, k, dim) > 160 * 1024) nqp = (nqp + 1) / 2;
    const size_t lds = listed_m_lds_bytes(nqp, k, dim);
    if (lds > 160 * 1024) return;
    const uint32_t ntiles = (count + kListedMTile - 1) / kListedMTile;
    const int per_cu = listed_occupancy(true, 0, lds);
    const uint32_t want = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)n_cus * per_cu);
    p->per_block = (ntiles + want - 1) / want;
    p->blocks = (int)((ntiles + p->per_block - 1) / p->per_block);
    p->nq_pass = nqp;
    p->lds = lds;
    return;
  }
  const int cpl = sweep_cpl_for_dim(dim);
  int B = nq_left >= 5 ? 8 : (nq_left >= 2 ? 4 : 1);
  while (B > 1 && sweep_lds_bytes(B, k, dim, cpl) > 60 * 1024) B = B == 8 ? 4 : 1;
  if (sweep_lds_bytes(B, k, dim, cpl) > 60 * 1024) return;
  const uint32_t rpg = 64u / (uint32_t)B;
  const uint32_t ngroups = (count + rpg - 1) / rpg;
  const int occ = listed_occupancy(false, B, 0);
  const uint32_t want = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)ngroups + 3) / 4, (uint64_t)n_cus * occ));
  p->per_block = (ngroups + want - 1) / want;
  p->blocks = (int)((ngroups + p->per_block - 1) / p->per_block);
  p->nq_pass = std::min<uint32_t>(nq_left, (uint32_t)B);
  p->lds = sweep_lds_bytes(B, k, dim, cpl);
  p->B = B;
}

template <int METRIC, int B, int CPL>
static hipError_t launch_listed_t(const ListedPlan& p, const ListedArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((sweep_topk_listed<METRIC, B, CPL>), dim3(p.blocks), dim3(256), p.lds, st, a, p.per_block);
  return hipGetLastError();
}
template <int METRIC, int B>
static hipError_t launch_listed_cpl(const ListedPlan& p, const ListedArgs& a, hipStream_t st) {
  switch (sweep_cpl_for_dim(a.dim)) {
    case 1: return launch_listed_t<METRIC, B, 1>(p, a, st);
    case 2: return launch_listed_t<METRIC, B, 2>(p, a, st);
    case 3: return launch_listed_t<METRIC, B, 3>(p, a, st);
    case 4: return launch_listed_t<METRIC, B, 4>(p, a, st);
    default: return launch_listed_t<METRIC, B, 0>(p, a, st);
  }
}
template <int METRIC>
static hipError_t launch_listed_b(const ListedPlan& p, const ListedArgs& a, hipStream_t st) {
  switch (p.B) {
    case 1: return launch_listed_cpl<METRIC, 1>(p, a, st);
    case 4: return launch_listed_cpl<METRIC, 4>(p, a, st);
    default: return launch_listed_cpl<METRIC, 8>(p, a, st);
  }
}
template <int METRIC>
static hipError_t launch_listed_m(const ListedPlan& p, const ListedArgs& a, hipStream_t st) {
  static bool done = false;
  if (p.lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_listed_m<METRIC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  const uint32_t dim_pad = (a.dim + 127) / 128 * 128;
  hipLaunchKernelGGL((sweep_topk_listed_m<METRIC>), dim3(p.blocks), dim3(256), p.lds, st, a, dim_pad, p.per_block);
  return hipGetLastError();
}

hipError_t launch_sweep_listed(int metric, bool mode_m, const ListedPlan& p, const ListedArgs& a, hipStream_t st) {
  if (mode_m) return metric == kCosine ? launch_listed_m<kCosine>(p, a, st) : launch_listed_m<kDot>(p, a, st);
  switch (metric) {
    case kCosine: return launch_listed_b<kCosine>(p, a, st);
    case kEuclidean: return launch_listed_b<kEuclidean>(p, a, st);
    default: return launch_listed_b<kDot>(p, a, st);
  }
}

// ---- the grouped launches: one block per work item, the same dispatch by metric, B and CPL ----
int listed_occupancy(bool mode_m, int B, size_t lds) {
  if (mode_m) return (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / std::max<size_t>(lds, 1), 4));
  return (B == 1) ? 4 : (B == 8 ? 2 : 3);  // resident 256-thread blocks per CU (VGPR-limited, as sweep_topk_f32)
}
template <int METRIC, int B, int CPL>
static hipError_t launch_groups_t(const ListedArgs& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q, hipStream_t st) {
  const size_t lds = sweep_lds_bytes(B, a.k, a.dim, CPL);
  hipLaunchKernelGGL((sweep_topk_listed_groups<METRIC, B, CPL>), dim3(n_items), dim3(256), lds, st, a, items, lists_per_q);
  return hipGetLastError();
}
template <int METRIC, int B>
static hipError_t launch_groups_cpl(const ListedArgs& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q, hipStream_t st) {
  switch (sweep_cpl_for_dim(a.dim)) {
    case 1: return launch_groups_t<METRIC, B, 1>(a, items, n_items, lists_per_q, st);
    case 2: return launch_groups_t<METRIC, B, 2>(a, items, n_items, lists_per_q, st);
    case 3: return launch_groups_t<METRIC, B, 3>(a, items, n_items, lists_per_q, st);
    case 4: return launch_groups_t<METRIC, B, 4>(a, items, n_items, lists_per_q, st);
    default: return launch_groups_t<METRIC, B, 0>(a, items, n_items, lists_per_q, st);
  }
}
template <int METRIC>
static hipError_t launch_groups_b(int B, const ListedArgs& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q, hipStream_t st) {
  switch (B) {
    case 1: return launch_groups_cpl<METRIC, 1>(a, items, n_items, lists_per_q, st);
    case 4: return launch_groups_cpl<METRIC, 4>(a, items, n_items, lists_per_q, st);
    default: return launch_groups_cpl<METRIC, 8>(a, items, n_items, lists_per_q, st);
  }
}
template <int METRIC>
static hipError_t launch_groups_m(const ListedArgs& a, const ListedGroupItem* items, uint32_t n_items, uint32_t nq_max, uint32_t lists_per_q,
                                  hipStream_t st) {
  const size_t lds = listed_m_lds_bytes(nq_max, a.k, a.dim);
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_listed_groups_m<METRIC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  const uint32_t dim_pad = (a.dim + 127) / 128 * 128;
  hipLaunchKernelGGL((sweep_topk_listed_groups_m<METRIC>), dim3(n_items), dim3(256), lds, st, a, dim_pad, items, lists_per_q);
  return hipGetLastError();
}
// a: rows / norms / alive / queries / part_keys / strides / dim / k (list, count and nq travel in the items); B: the launch's class
// (mode C), nq_max: the largest pass of the launch (mode M: it sizes the LDS)
hipError_t launch_sweep_listed_groups(int metric, bool mode_m, int B, const ListedArgs& a, const ListedGroupItem* items, uint32_t n_items,
                                      uint32_t nq_max, uint32_t lists_per_q, hipStream_t st) {
  if (n_items == 0) return hipSuccess;
  if (mode_m)
    return metric == kCosine ? launch_groups_m<kCosine>(a, items, n_items, nq_max, lists_per_q, st)
                             : launch_groups_m<kDot>(a, items, n_items, nq_max, lists_per_q, st);
  switch (metric) {
    case kCosine: return launch_groups_b<kCosine>(B, a, items, n_items, lists_per_q, st);
    case kEuclidean: return launch_groups_b<kEuclidean>(B, a, items, n_items, lists_per_q, st);
    default: return launch_groups_b<kDot>(B, a, items, n_items, lists_per_q, st);
  }
}

}  // namespace vdb
