// sweep_half_l2.hip — Euclidean distance over the half-precision copies of the rows: half_precision::euclidean_distance
// (crates/velesdb-core/src/half_precision.rs:257-287) on VectorData::F16 (:274-279: sqrt of the f32 sum of (x - y)^2, the difference
// taken in f32) and on VectorData::BF16 (:281-285: the same over the values converted back to f32), as an exact sweep with fused
// top-k (VDB_SEARCH_BRUTE_F16 / VDB_SEARCH_BRUTE_BF16 on a Euclidean handle).
//
// Why a difference-form chain and not |q|^2 + |v|^2 - 2 q.v on the matrix cores: for a row close to the query the expanded form
// cancels — measured on f16-rounded N(0,1) data, rows at distance 0.06 .. 0.4 come out 1.3e-3 .. 2.7e-3 off (relative), a chain of
// (q - v)^2 stays within 1.5e-6 of float64.  The reported score therefore always comes from the chain below.
//
// DECLARED SUMMATION ORDER (the "mode C" order of vdb_device.hpp, with 8-element chunks): for a rounded query q and a rounded row v,
// both converted back to f32 (exact),
//   * element i belongs to the 16-byte chunk c = i / 8 of the half row; chunk c belongs to lane c % 64;
//   * every lane runs ONE chain from +0.0f over its elements in increasing i: d = q[i] - v[i] (f32 subtraction, exact for two half
//     values unless their exponents are > 24 apart), acc = fmaf(d, d, acc);
//   * elements i >= dim are zero in both images (the copies are zero-padded to a multiple of 8): fmaf(0, 0, acc) == acc, bit for bit;
//   * the 64 lanes are combined with the xor butterfly 32, 16, 8, 4, 2, 1 (transposed: 64 (row, query) pairs per lane in, one
//     finished sum per lane out — same bits), then sqrtf (correctly rounded); any NaN -> +qNaN (canon_nan).
// Every product and partial sum exact in f32  =>  the result equals the reference's sequential chain bit for bit (tests).
//
// Shape: as sweep_topk_f32 — one wave owns RPG = 64 / B whole rows x B queries per step, a row is read ONCE as 16-byte loads
// (8 half values per lane, 1 KiB per load instruction), converted in registers; the B rounded queries live in LDS as f32 (converted
// once per block) and are read back as ds_read_b128; block-shared sorted top-k lists, one per query (vdb_device.hpp); one list
// per query and block goes to HBM and merge_topk* finishes.  Algorithmic HBM bytes per corpus pass: n_rows * stride * 2.
// LDS: q[B][stride] f32 | lists[B][k] u64 | cnt[B] | lock[B].
#include <algorithm>

#include "vdb_device.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

struct HalfL2Args {
  const uint16_t* rows;  // [n_rows][row_stride] f16 / bf16, row_stride % 8 == 0, zero behind dim
  const uint8_t* alive;
  const float* queries;  // f32, rounded to the half format while staging
  uint64_t* part_keys;
  uint64_t row_stride, q_stride;
  uint32_t n_rows, dim, nq, k;
};

template <bool F16>
__device__ __forceinline__ float half_round(float x) {  // the value a half copy holds, back in f32
  if (F16) return (float)(_Float16)x;  // v_cvt_f16_f32 (round to nearest even, overflow to inf, subnormals kept) and back
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return __uint_as_float(((u >> 16) | 0x0040u) << 16);  // NaN stays NaN (quiet)
  u += 0x7FFFu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xFFFF0000u);
}
// the two half values of one dword, lower address first
template <bool F16>
__device__ __forceinline__ void unpack2(uint32_t w, float& lo, float& hi) {
  if (F16) {
    lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
    hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
  } else {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xFFFF0000u);
  }
}

// The body is shared by the sweep over all rows and the LISTED one (filtered search over a half image): there position p of
// the filter's ascending row list stands where row p stood — the row pointer comes through the list, positions past `count` re-read the
// list's last row and are masked, the key carries the real row — and block b takes the groups [b * per_block, (b + 1) * per_block) of
// the list.  The declared summation order above is per (row, query): the same bits wherever the row sits.
// GROUPED (one filter per query; implies LISTED): the block does ONE work item — `list` / `count` are the item's chunk of
// its filter's list, handed over as a list of its own and swept whole from unit 0 (`per_block` = its units), a.nq the item's pass;
// query b of the pass is row it->q[b] of a.queries and of the partial-list area [call's queries][lists_per_q][k], and the block's
// lists go to slot it->slot.  What is only needed at the end (slot, the positions) is read there.
template <bool F16, int B, bool LISTED, bool GROUPED = false>
__device__ __forceinline__ void half_l2_sweep_body(const HalfL2Args& a, const uint32_t* __restrict__ list, uint32_t count, uint32_t per_block,
                                                   const ListedGroupItem* __restrict__ it = nullptr, uint32_t lists_per_q = 0u) {
  constexpr int RPG = 64 / B;                // rows per group: 64 (row, query) pairs per lane
  constexpr int RB = RPG < 4 ? RPG : (B == 1 ? 8 : 4);  // rows in flight together
  constexpr bool HIB = false;                // a distance: smaller is better
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t wave = blockIdx.x * 4 + wib;
  const uint32_t nwaves = gridDim.x * 4;
  const uint32_t k = a.k;
  const uint32_t qlen = (uint32_t)a.row_stride;  // floats per staged query
  const uint32_t d8 = qlen / 8;                  // 16-byte chunks per row
  float* qs = reinterpret_cast<float*>(smem);
  unsigned char* lbase = smem + (size_t)B * qlen * 4;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(lbase);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(lbase + (size_t)B * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(lbase + (size_t)B * k * 8 + (size_t)B * 4);
  if (threadIdx.x < B) {
    cnts[threadIdx.x] = 0;
    locks[threadIdx.x] = 0;
  }
  for (uint32_t i = threadIdx.x; i < (uint32_t)B * qlen; i += 256) {
    const uint32_t b = i / qlen, e = i % qlen;
    qs[i] = (b < a.nq && e < a.dim) ? half_round<F16>(a.queries[(GROUPED ? (size_t)it->q[b] : (size_t)b) * a.q_stride + e]) : 0.0f;
  }
  __syncthreads();

  const uint32_t n_here = LISTED ? count : a.n_rows;  // rows of the sweep: positions of the list, or rows of the index
  const uint32_t ngroups = (n_here + RPG - 1) / RPG;
  const uint32_t g_end = GROUPED ? per_block : (LISTED ? min(ngroups, (blockIdx.x + 1) * per_block) : ngroups);  // listed: the block's chunk of the list
  for (uint32_t g = GROUPED ? (uint32_t)wib : (LISTED ? blockIdx.x * per_block + (uint32_t)wib : wave); g < g_end; g += LISTED ? 4u : nwaves) {
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; i++) acc[i] = 0.0f;
    const uint32_t row0 = g * RPG;
#pragma unroll
    for (int r0 = 0; r0 < RPG; r0 += RB) {
      const uint16_t* rp[RB];
#pragma unroll
      for (int rr = 0; rr < RB; rr++) {
        uint32_t row = row0 + r0 + rr;
        row = row < n_here ? row : n_here - 1;  // tail rows: re-read the last row, masked later
        if constexpr (LISTED) row = list[row];
        rp[rr] = a.rows + (size_t)row * a.row_stride;
      }
      for (uint32_t c = lane; c < d8; c += 64) {
        uint4 v[RB];
#pragma unroll
        for (int rr = 0; rr < RB; rr++) v[rr] = *reinterpret_cast<const uint4*>(rp[rr] + (size_t)c * 8);
#pragma unroll
        for (int rr = 0; rr < RB; rr++) {
          float x[8];
          unpack2<F16>(v[rr].x, x[0], x[1]);
          unpack2<F16>(v[rr].y, x[2], x[3]);
          unpack2<F16>(v[rr].z, x[4], x[5]);
          unpack2<F16>(v[rr].w, x[6], x[7]);
          const float4 x0 = make_float4(x[0], x[1], x[2], x[3]), x1 = make_float4(x[4], x[5], x[6], x[7]);
#pragma unroll
          for (int b = 0; b < B; b++) {
            const float* qp = qs + (size_t)b * qlen + (size_t)c * 8;
            float s = acc[(r0 + rr) * B + b];
            s = chain4<kOpL2>(s, ld4(qp), x0);
            s = chain4<kOpL2>(s, ld4(qp + 4), x1);
            acc[(r0 + rr) * B + b] = s;
            if (B > 1 && (b & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (keeps the query reads of a step from being hoisted together)
          }
        }
      }
    }
    treduce64(acc, lane);
    // lane l now owns pair idx = l: row r = l / B, query b = l % B
    const int b = lane % B;
    const uint32_t pos = row0 + lane / B;
    const bool valid = pos < n_here && b < (int)a.nq;
    const uint32_t row = LISTED ? (valid ? list[pos] : 0u) : pos;
    const float score = finish_score<kEuclidean>(acc[0], 0.0f, 0.0f);
    const uint64_t key = valid ? make_key<HIB>(score, row) : kKeyInvalid;
    const uint32_t c_b = cnts[b];
    const uint64_t tau = (c_b == k) ? lists[(size_t)b * k + (k - 1)] : kKeyInvalid;
    uint64_t mask = __ballot(key < tau);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const uint64_t kk = readlane64(key, src);
      if (a.alive && a.alive[key_row(kk)] == 0) continue;  // soft-deleted rows are filtered where it is rare
      const int bb = src % B;
      shared_list_offer(lists + (size_t)bb * k, cnts + bb, locks + bb, k, kk, lane);
    }
  }
  __syncthreads();
  for (int b = wib; b < (int)a.nq && b < B; b += 4) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + (GROUPED ? (size_t)it->q[b] * lists_per_q + (uint32_t)__builtin_amdgcn_readfirstlane((int)it->slot)
                                           : (size_t)b * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}
template <bool F16, int B>
__global__ __launch_bounds__(256, 3) void sweep_topk_half_l2(HalfL2Args a) {
  half_l2_sweep_body<F16, B, false>(a, nullptr, 0u, 0u);
}
// the sweep over a filter's ascending row list; a.n_rows is not read
struct HalfL2ListedArgs {
  HalfL2Args a;
  const uint32_t* list;   // [count] ascending internal rows (device memory)
  uint32_t count;
  uint32_t per_block;     // row groups (64 / B rows) of the list per block
};
template <bool F16, int B>
__global__ __launch_bounds__(256, 3) void sweep_topk_half_l2_listed(HalfL2ListedArgs la) {
  half_l2_sweep_body<F16, B, true>(la.a, la.list, la.count, la.per_block);
}

// One filter per query over a half image (vdb_hip_index_search_batch_filters_mode): block b does work item b — one chunk
// of one pass of one filter's list (mode_groups_plan, vdb_filter_route.hpp), as sweep_topk_listed_groups does over the f32 rows.  The
// item is read with uniform loads; the list pointer is rebuilt as a GLOBAL one, so the list is read with global_load, not flat_load.
template <bool F16, int B>
__global__ __launch_bounds__(256, 3) void sweep_topk_half_l2_listed_groups(HalfL2Args a, const ListedGroupItem* __restrict__ items,
                                                                           uint32_t lists_per_q) {
  const ListedGroupItem* __restrict__ it = items + blockIdx.x;
  typedef const __attribute__((address_space(1))) uint32_t* glb_u32_p;
  const uint64_t lp = reinterpret_cast<uint64_t>(it->list);
  const uint32_t* list = (const uint32_t*)(glb_u32_p)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lp >> 32)) << 32) |
                                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lp));
  a.nq = (uint32_t)__builtin_amdgcn_readfirstlane((int)it->nq);
  half_l2_sweep_body<F16, B, true, true>(a, list, (uint32_t)__builtin_amdgcn_readfirstlane((int)it->count),
                                         (uint32_t)__builtin_amdgcn_readfirstlane((int)it->units), it, lists_per_q);
}

size_t sweep_half_l2_lds_bytes(int B, uint32_t k, uint32_t dim) { return (size_t)fm_half_l2_lds_bytes(B, k, dim); }

template <bool F16, int B>
static hipError_t launch_half_l2_t(const HalfL2Args& a, int blocks, size_t lds, hipStream_t st) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_half_l2<F16, B>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_half_l2<F16, B>), dim3(blocks), dim3(256), lds, st, a);
  return hipGetLastError();
}
template <bool F16>
static hipError_t launch_half_l2_b(int B, const HalfL2Args& a, int blocks, size_t lds, hipStream_t st) {
  switch (B) {
    case 16: return launch_half_l2_t<F16, 16>(a, blocks, lds, st);
    case 4: return launch_half_l2_t<F16, 4>(a, blocks, lds, st);
    case 1: return launch_half_l2_t<F16, 1>(a, blocks, lds, st);
    default: return hipErrorInvalidValue;
  }
}
// rows: the half copy (stride = dim rounded up to 8, zero-padded); queries: nq <= B f32 rows; part_keys: [nq][blocks][k]
hipError_t launch_sweep_half_l2(bool f16, int B, const uint16_t* rows, uint64_t row_stride, const uint8_t* alive, const float* queries,
                                uint64_t q_stride, uint64_t* part_keys, uint32_t n_rows, uint32_t dim, uint32_t nq, uint32_t k, int blocks,
                                hipStream_t st) {
  if (row_stride % 8 != 0 || row_stride < dim || nq > (uint32_t)B) return hipErrorInvalidValue;
  HalfL2Args a{rows, alive, queries, part_keys, row_stride, q_stride, n_rows, dim, nq, k};
  const size_t lds = sweep_half_l2_lds_bytes(B, k, dim);
  return f16 ? launch_half_l2_b<true>(B, a, blocks, lds, st) : launch_half_l2_b<false>(B, a, blocks, lds, st);
}

template <bool F16, int B>
static hipError_t launch_half_l2_listed_t(const HalfL2ListedArgs& la, int blocks, size_t lds, hipStream_t st) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_half_l2_listed<F16, B>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_half_l2_listed<F16, B>), dim3(blocks), dim3(256), lds, st, la);
  return hipGetLastError();
}
template <bool F16>
static hipError_t launch_half_l2_listed_b(int B, const HalfL2ListedArgs& la, int blocks, size_t lds, hipStream_t st) {
  switch (B) {
    case 16: return launch_half_l2_listed_t<F16, 16>(la, blocks, lds, st);
    case 4: return launch_half_l2_listed_t<F16, 4>(la, blocks, lds, st);
    case 1: return launch_half_l2_listed_t<F16, 1>(la, blocks, lds, st);
    default: return hipErrorInvalidValue;
  }
}
// the same over `count` listed rows (ascending internal rows, device memory): blocks x per_block row groups cover the list
// (mode_listed_plan, vdb_filter_route.hpp); part_keys: [nq][blocks][k]
hipError_t launch_sweep_half_l2_listed(bool f16, int B, const uint16_t* rows, uint64_t row_stride, const uint8_t* alive, const uint32_t* list,
                                       uint32_t count, uint32_t per_block, const float* queries, uint64_t q_stride, uint64_t* part_keys,
                                       uint32_t n_rows, uint32_t dim, uint32_t nq, uint32_t k, int blocks, hipStream_t st) {
  if (row_stride % 8 != 0 || row_stride < dim || nq > (uint32_t)B || count == 0 || per_block == 0 || !list) return hipErrorInvalidValue;
  if ((uint64_t)blocks * per_block * (64u / (uint32_t)B) < count) return hipErrorInvalidValue;  // (the chunks must cover the list)
  HalfL2ListedArgs la{{rows, alive, queries, part_keys, row_stride, q_stride, n_rows, dim, nq, k}, list, count, per_block};
  const size_t lds = sweep_half_l2_lds_bytes(B, k, dim);
  return f16 ? launch_half_l2_listed_b<true>(B, la, blocks, lds, st) : launch_half_l2_listed_b<false>(B, la, blocks, lds, st);
}

template <bool F16, int B>
static hipError_t launch_half_l2_listed_groups_t(const HalfL2Args& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q,
                                                 size_t lds, hipStream_t st) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_half_l2_listed_groups<F16, B>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_half_l2_listed_groups<F16, B>), dim3(n_items), dim3(256), lds, st, a, items, lists_per_q);
  return hipGetLastError();
}
template <bool F16>
static hipError_t launch_half_l2_listed_groups_b(int B, const HalfL2Args& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q,
                                                 size_t lds, hipStream_t st) {
  switch (B) {
    case 16: return launch_half_l2_listed_groups_t<F16, 16>(a, items, n_items, lists_per_q, lds, st);
    case 4: return launch_half_l2_listed_groups_t<F16, 4>(a, items, n_items, lists_per_q, lds, st);
    case 1: return launch_half_l2_listed_groups_t<F16, 1>(a, items, n_items, lists_per_q, lds, st);
    default: return hipErrorInvalidValue;
  }
}
// one grouped launch of a call with one filter per query: block b does items[b] (device memory; mode_groups_plan); a
// query is addressed by its position in `queries`; part_keys: [call's queries][lists_per_q][k], pre-filled with invalid keys
hipError_t launch_sweep_half_l2_listed_groups(bool f16, int B, const uint16_t* rows, uint64_t row_stride, const uint8_t* alive, const float* queries,
                                              uint64_t q_stride, uint64_t* part_keys, uint32_t dim, uint32_t k, const ListedGroupItem* items,
                                              uint32_t n_items, uint32_t lists_per_q, hipStream_t st) {
  if (row_stride % 8 != 0 || row_stride < dim || !items || n_items == 0 || lists_per_q == 0) return hipErrorInvalidValue;
  HalfL2Args a{rows, alive, queries, part_keys, row_stride, q_stride, 0u, dim, 0u, k};  // (n_rows is not read; nq comes from the item)
  const size_t lds = sweep_half_l2_lds_bytes(B, k, dim);
  return f16 ? launch_half_l2_listed_groups_b<true>(B, a, items, n_items, lists_per_q, lds, st)
             : launch_half_l2_listed_groups_b<false>(B, a, items, n_items, lists_per_q, lds, st);
}

}  // namespace vdb
