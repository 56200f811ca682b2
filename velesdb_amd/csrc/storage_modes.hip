// storage_modes.hip — the storage modes of core/quantization.rs on the GPU: SQ8 (QuantizedVector: one byte per
// dimension + per-vector min/max, :204-316) and Binary (BinaryQuantizedVector: one sign bit per dimension, :48-202),
// the quantisers, and exact top-k searches of f32 queries over the quantised corpus with the reference's asymmetric
// distances dot_product_quantized_simd / euclidean_squared_quantized_simd / cosine_similarity_quantized_simd
// (:410-554) and BinaryQuantizedVector::hamming_distance (:123-135).  crud.rs:66-82 builds exactly these codes on
// upsert when a collection's StorageMode is SQ8 / Binary.
//
// Arithmetic: the reference's functions are plain scalar Rust — every sum is one left-to-right chain over the
// dimensions, nothing is fused (Rust never contracts a*b+c).  That order is reproduced exactly: ONE LANE OWNS ONE
// ROW and walks its dimensions in order with separately rounded multiplies and adds (__fmul_rn / __fadd_rn = plain
// * and + under -ffp-contract=off; sqrtf and / are correctly rounded; NOT __fsqrt_rn, which is the native
// approximation in this toolchain), so
// scores are bit-identical to the oracle's restatement (oracle/vdb_oracle.cpp vo_sq8_*), and — the reference's
// functions being deterministic scalar code — to the reference itself.
//
// sweep_topk_sq8<METRIC,B>: a wave takes 64 rows; their codes arrive through an LDS tile (16 rows x 64 B per load
// instruction, coalesced; each lane then reads its own row's 64 bytes with 4 conflict-free ds_read_b128), the B
// queries sit in LDS dimension-major so one broadcast ds_read_b128 feeds 4 queries; per element 3 VALU ops of
// dequantisation shared by the B queries + 2 per query.  Bound: HBM for B <= 4 (N*(dim+16) bytes per pass: 784 MB
// at 1 M x 768), the vector ALUs beyond.  Top-k: block-shared locked lists (vdb_device.hpp) + merge_topk.
#include <algorithm>
#include <cstring>
#include <memory>

#include "vdb_device.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_index.hpp"
#include "vdb_kernels.hpp"
#include "vdb_sweep_pass.hpp"

namespace vdb {

constexpr float kF32Eps = 1.1920929e-07f;  // f32::EPSILON

// ---- quantisers ---------------------------------------------------------------------------------------------
// QuantizedVector::from_f32 (:229-255), one wave per row: min / max are order-independent, the codes elementwise.
// Also keeps quantized_norm_sq of cosine_similarity_quantized_simd (:531-546) — a left-to-right chain, so it is
// computed by sq8_norms below, one lane per row.
__global__ __launch_bounds__(256) void sq8_quantize_rows(const float* rows, uint64_t row_stride, uint8_t* codes,
                                                         uint64_t code_stride, float* vmin, float* vmax, uint32_t row0,
                                                         uint32_t n_rows, uint32_t dim) {
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t r = wave; r < n_rows; r += nwaves) {
    const uint32_t row = row0 + r;
    const float* p = rows + (size_t)row * row_stride;
    float mn = __uint_as_float(0x7F800000u), mx = __uint_as_float(0xFF800000u);
    for (uint32_t i = lane; i < dim; i += 64) {
      mn = fminf(mn, p[i]);  // f32::min / f32::max semantics: a NaN operand yields the other one
      mx = fmaxf(mx, p[i]);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, s, 64));
      mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    }
    const float range = __fsub_rn(mx, mn);
    uint8_t* c = codes + (size_t)row * code_stride;
    if (range < kF32Eps) {
      for (uint32_t i = lane; i < code_stride; i += 64) c[i] = i < dim ? 128 : 0;
    } else {
      const float scale = __fdiv_rn(255.0f, range);
      for (uint32_t i = lane; i < code_stride; i += 64) {
        uint8_t q = 0;
        if (i < dim) {
          const float normalized = __fmul_rn(__fsub_rn(p[i], mn), scale);
          float rr = roundf(normalized);  // half away from zero, like f32::round
          rr = rr < 0.0f ? 0.0f : (rr > 255.0f ? 255.0f : rr);
          q = (rr != rr) ? (uint8_t)0 : (uint8_t)rr;  // NaN `as u8` saturates to 0
        }
        c[i] = q;
      }
    }
    if (lane == 0) {
      vmin[row] = mn;
      vmax[row] = mx;
    }
  }
}

__global__ __launch_bounds__(256) void sq8_norms(const uint8_t* codes, uint64_t code_stride, const float* vmin,
                                                 const float* vmax, float* nsq, uint32_t row0, uint32_t n_rows,
                                                 uint32_t dim) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t row = row0 + r;
  const float mn = vmin[row], range = __fsub_rn(vmax[row], mn);
  const float scale = range < kF32Eps ? 0.0f : __fdiv_rn(range, 255.0f);
  const uint32_t* c = reinterpret_cast<const uint32_t*>(codes + (size_t)row * code_stride);
  float s = 0.0f;
  for (uint32_t i = 0; i < dim; i += 4) {
    const uint32_t w = c[i / 4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (i + e < dim) {
        const float dq = __fadd_rn(__fmul_rn((float)((w >> (8 * e)) & 0xFFu), scale), mn);
        s = __fadd_rn(s, __fmul_rn(dq, dq));
      }
    }
  }
  nsq[row] = s;
}

// BinaryQuantizedVector::from_f32 (:68-86): bit i = (v[i] >= 0.0), LSB-first in bytes = bit i%32 of word i/32.
// One wave per row: a ballot over 64 consecutive dimensions IS eight of the reference's bytes.
__global__ __launch_bounds__(256) void sign_bits_rows(const float* rows, uint64_t row_stride, uint32_t* bits, uint32_t words,
                                                      uint32_t row0, uint32_t n_rows, uint32_t dim) {
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t r = wave; r < n_rows; r += nwaves) {
    const uint32_t row = row0 + r;
    const float* p = rows + (size_t)row * row_stride;
    uint32_t* dst = bits + (size_t)row * words;
    for (uint32_t e0 = 0; e0 < words * 32; e0 += 64) {
      const uint32_t e = e0 + lane;
      const bool bit = e < dim && p[e] >= 0.0f;  // NaN >= 0 is false, -0.0 >= 0 is true, as on the CPU
      const uint64_t m = __ballot(bit);
      if (lane == 0) {
        dst[e0 / 32] = (uint32_t)m;
        if (e0 / 32 + 1 < words) dst[e0 / 32 + 1] = (uint32_t)(m >> 32);
      }
    }
  }
}

// ---- SQ8 sweep ------------------------------------------------------------------------------------------------
struct Sq8Args {
  const uint8_t* codes;   // [n_rows][code_stride], code_stride % 16 == 0, padding bytes 0
  const float* vmin;
  const float* vmax;
  const float* nsq;       // quantized_norm_sq per row (cosine)
  const uint8_t* alive;
  const float* queries;   // [nq][q_stride] f32
  uint64_t* part_keys;    // [nq][n_blocks][k]
  uint64_t code_stride, q_stride;
  uint32_t n_rows, dim, nq, k;
  // gathered variant (the exact pass over the queries a selection stage could not prove): block row blockIdx.y serves the
  // queries qmap[B y .. B y + B - 1] of the *qcount listed ones and exits when there are none; part_keys slots follow the list
  const uint32_t* qmap;
  const uint32_t* qcount;
};

constexpr int kSq8TileStride = 80;  // bytes per row of the staging tile: 64 + 16 padding (conflict-free b128 reads)

typedef float sq8_f32x4 __attribute__((ext_vector_type(4)));
// One broadcast read of four queries' element (16 bytes at a wave-uniform LDS address), WRITTEN AS AN INSTRUCTION.  Left to the
// compiler the unrolled 64-code chunk came out as [one ds_read, s_waitcnt lgkmcnt(0), four vector instructions] x 128: every LDS
// round trip exposed, half of every wave's time in s_waitcnt (round 5 counters, profiles/r05k_*: vector ALU busy 0.54, LDS array
// 0.43, SQ_WAIT_ANY 0.51 of the wave cycles).  Here the reads of a whole code word (4 codes x B queries) are issued together, ONE
// WORD AHEAD of the arithmetic that uses them (two register sets), and one wait per word follows the arithmetic of the word before.
// (Measured and dropped in the same round: the queries' elements through scalar loads from a transposed global copy — no gain, the
// wait was the cost, not the broadcast's 64-fold write; plain instead of packed multiplies / adds — 18 % slower.)
template <int OFF>
__device__ __forceinline__ void sq8_lds_read4(sq8_f32x4& d, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
// (the wait names the values it makes valid: a use cannot be scheduled in front of it)
__device__ __forceinline__ void sq8_lds_wait(sq8_f32x4 (&q)[4][1]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q[0][0]), "+v"(q[1][0]), "+v"(q[2][0]), "+v"(q[3][0])::"memory");
}
__device__ __forceinline__ void sq8_lds_wait(sq8_f32x4 (&q)[4][2]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(q[0][0]), "+v"(q[0][1]), "+v"(q[1][0]), "+v"(q[1][1]), "+v"(q[2][0]), "+v"(q[2][1]), "+v"(q[3][0]), "+v"(q[3][1])::"memory");
}
template <int B, int WI>
__device__ __forceinline__ void sq8_read_word(sq8_f32x4 (&q)[4][B / 4], uint32_t qaddr) {
  // element e of the word, queries 4 j .. 4 j + 3: byte offset ((4 WI + e) B + 4 j) 4 behind the chunk's first element
  sq8_lds_read4<((4 * WI + 0) * B + 0) * 4>(q[0][0], qaddr);
  sq8_lds_read4<((4 * WI + 1) * B + 0) * 4>(q[1][0], qaddr);
  sq8_lds_read4<((4 * WI + 2) * B + 0) * 4>(q[2][0], qaddr);
  sq8_lds_read4<((4 * WI + 3) * B + 0) * 4>(q[3][0], qaddr);
  if constexpr (B == 8) {
    sq8_lds_read4<((4 * WI + 0) * B + 4) * 4>(q[0][1], qaddr);
    sq8_lds_read4<((4 * WI + 1) * B + 4) * 4>(q[1][1], qaddr);
    sq8_lds_read4<((4 * WI + 2) * B + 4) * 4>(q[2][1], qaddr);
    sq8_lds_read4<((4 * WI + 3) * B + 4) * 4>(q[3][1], qaddr);
  }
}
// one code word (4 codes of the lane's row) against the B queries: the reference's chains, element by element in order
// (dot: quantization.rs:452-466; squared L2: :495-507 — sum += ((f0^2 + f1^2) + f2^2) + f3^2 per group of four)
template <int METRIC, int B>
__device__ __forceinline__ void sq8_word_math(float (&acc)[B], uint32_t w, float scale, float mn, const sq8_f32x4 (&q)[4][B / 4]) {
  float dq[4];
#pragma unroll
  for (int e = 0; e < 4; e++) dq[e] = __fadd_rn(__fmul_rn((float)((w >> (8 * e)) & 0xFFu), scale), mn);
  constexpr int P = B / 2;  // query pairs: v_pk_mul_f32 / v_pk_add_f32 — each half is the same IEEE operation as the scalar form
  if (METRIC == kEuclidean) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      f32x2 t = {0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const f32x2 f = f32x2{q[e][p / 2][2 * (p & 1)], q[e][p / 2][2 * (p & 1) + 1]} - f32x2{dq[e], dq[e]};
        t = e == 0 ? f * f : t + f * f;
      }
      acc[2 * p] = __fadd_rn(acc[2 * p], t.x);
      acc[2 * p + 1] = __fadd_rn(acc[2 * p + 1], t.y);
    }
  } else {
    // the products of TWO codes first, then their additions in the reference's order (code e before code e + 1 on every chain): an
    // addition then stands four to eight instructions behind the multiply it needs, instead of directly behind it
#pragma unroll
    for (int e0 = 0; e0 < 4; e0 += 2) {
      f32x2 pr[2][P];
#pragma unroll
      for (int e = 0; e < 2; e++)
#pragma unroll
        for (int p = 0; p < P; p++) pr[e][p] = f32x2{q[e0 + e][p / 2][2 * (p & 1)], q[e0 + e][p / 2][2 * (p & 1) + 1]} * f32x2{dq[e0 + e], dq[e0 + e]};
#pragma unroll
      for (int e = 0; e < 2; e++)
#pragma unroll
        for (int p = 0; p < P; p++) {
          const f32x2 r = f32x2{acc[2 * p], acc[2 * p + 1]} + pr[e][p];
          acc[2 * p] = r.x;
          acc[2 * p + 1] = r.y;
        }
    }
  }
}
// words WI, WI + 1 of a chunk: q0 holds word WI's elements (valid), q1 receives word WI + 1's while word WI is multiplied, and so on
template <int METRIC, int B, int WI>
__device__ __forceinline__ void sq8_word_pair(float (&acc)[B], const uint32_t (&wds)[16], float scale, float mn, uint32_t qaddr,
                                              sq8_f32x4 (&q0)[4][B / 4], sq8_f32x4 (&q1)[4][B / 4]) {
  sq8_read_word<B, WI + 1>(q1, qaddr);
  sq8_word_math<METRIC, B>(acc, wds[WI], scale, mn, q0);
  sq8_lds_wait(q1);
  if constexpr (WI + 2 < 16) sq8_read_word<B, WI + 2>(q0, qaddr);
  sq8_word_math<METRIC, B>(acc, wds[WI + 1], scale, mn, q1);
  if constexpr (WI + 2 < 16) sq8_lds_wait(q0);
}

// The body (sq8_sweep_body.inc) is shared by the sweep over all rows and the LISTED one (filtered search over the codes):
// there lane l of group g owns row list[g * 64 + l] — the staging loads gather their 16-byte pieces by that row, vmin / vmax / nsq are
// read through the list, positions past `count` are clamped to count - 1 and masked, the key carries the real row — and block b takes
// the groups [b * per_block, (b + 1) * per_block) of the list.  Every (row, query) chain is one lane's sequential chain over the row's
// own codes: the bits do not depend on where the row sits or which rows share its group.
// (Shared as TEXT, not as an inlined __device__ function: behind a function call — even an always-inlined one with nothing else
// changed — the Euclidean instances of sweep_topk_sq8 came out with other registers, 150 -> 138 and 211 -> 213 VGPRs; included into the
// kernel itself, every instance of sweep_topk_sq8 keeps the instructions it had.)
template <int METRIC, int B>
__global__ __launch_bounds__(256) void sweep_topk_sq8(Sq8Args a) {
  constexpr bool LISTED = false;
  constexpr bool GROUPED = false;
  const uint32_t* const list = nullptr;
  const uint32_t count = 0u, per_block = 0u;
  const ListedGroupItem* const it = nullptr;
  const uint32_t nq_item = 0u, lists_per_q = 0u;
#include "sq8_sweep_body.inc"
}
// the sweep over a filter's ascending row list; a.n_rows / qmap / qcount are not read
struct Sq8ListedArgs {
  Sq8Args a;
  const uint32_t* list;   // [count] ascending internal rows (device memory)
  uint32_t count;
  uint32_t per_block;     // 64-row groups of the list per block
};
template <int METRIC, int B>
__global__ __launch_bounds__(256) void sweep_topk_sq8_listed(Sq8ListedArgs la) {
  constexpr bool LISTED = true;
  constexpr bool GROUPED = false;
  const Sq8Args& a = la.a;
  const uint32_t* const list = la.list;
  const uint32_t count = la.count, per_block = la.per_block;
  const ListedGroupItem* const it = nullptr;
  const uint32_t nq_item = 0u, lists_per_q = 0u;
#include "sq8_sweep_body.inc"
}
// One filter per query over the codes (vdb_hip_index_search_batch_filters_mode): block b does work item b — one chunk of
// one pass of one filter's list (mode_groups_plan, vdb_filter_route.hpp), as sweep_topk_listed_groups does over the f32 rows.  The item
// is read with uniform loads: the chunk is a list of its own (pointer rebuilt as a GLOBAL one, so the list is read with global_load,
// not flat_load) swept whole from unit 0, query b of the pass is row it->q[b] of a.queries and of the partial-list area
// [call's queries][lists_per_q][k], and the block's lists go to slot it->slot.  a.nq / n_rows / qmap / qcount are not read.
// (Dot, B = 8: the twin sits at 128 VGPRs, four waves per SIMD — what mode_groups_plan sizes the launch by; with the item's scalars
// next to the sweep's the instance came out one register above it.  The compiler is told the occupancy there; 1 = no request.)
constexpr int sq8_groups_min_waves(int metric, int b) { return metric == kDot && b == 8 ? 4 : 1; }
template <int METRIC, int B>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sq8_groups_min_waves(METRIC, B)))) void sweep_topk_sq8_listed_groups(Sq8Args a, const ListedGroupItem* __restrict__ items, uint32_t lists_per_q) {
  constexpr bool LISTED = true;
  constexpr bool GROUPED = true;
  const ListedGroupItem* const it = items + blockIdx.x;
  typedef const __attribute__((address_space(1))) uint32_t* glb_u32_p;
  const uint64_t lp = reinterpret_cast<uint64_t>(it->list);
  const uint32_t* const list = (const uint32_t*)(glb_u32_p)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lp >> 32)) << 32) |
                                                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lp));
  const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)it->count), per_block = 0u;
  const uint32_t nq_item = (uint32_t)__builtin_amdgcn_readfirstlane((int)it->nq);
#include "sq8_sweep_body.inc"
}

static_assert(kSq8TileStride == 80, "fm_sq8_lds_bytes (vdb_filter_route.hpp) states the staging tile's stride");
static size_t sq8_lds_bytes(int B, uint32_t k, uint32_t dim) { return (size_t)fm_sq8_lds_bytes(B, k, dim); }

template <int METRIC, int B>
static hipError_t launch_sq8_t(const Sq8Args& a, int blocks, size_t lds, hipStream_t st, int groups = 1) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_sq8<METRIC, B>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_sq8<METRIC, B>), dim3(blocks, groups), dim3(256), lds, st, a);
  return hipGetLastError();
}
template <int B>
static hipError_t launch_sq8_m(int metric, const Sq8Args& a, int blocks, size_t lds, hipStream_t st, int groups = 1) {
  if (metric == kCosine) return launch_sq8_t<kCosine, B>(a, blocks, lds, st, groups);
  if (metric == kEuclidean) return launch_sq8_t<kEuclidean, B>(a, blocks, lds, st, groups);
  return launch_sq8_t<kDot, B>(a, blocks, lds, st, groups);
}

template <int METRIC, int B>
static hipError_t launch_sq8_listed_t(const Sq8ListedArgs& la, int blocks, size_t lds, hipStream_t st) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_sq8_listed<METRIC, B>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_sq8_listed<METRIC, B>), dim3(blocks), dim3(256), lds, st, la);
  return hipGetLastError();
}
template <int B>
static hipError_t launch_sq8_listed_m(int metric, const Sq8ListedArgs& la, int blocks, size_t lds, hipStream_t st) {
  if (metric == kCosine) return launch_sq8_listed_t<kCosine, B>(la, blocks, lds, st);
  if (metric == kEuclidean) return launch_sq8_listed_t<kEuclidean, B>(la, blocks, lds, st);
  return launch_sq8_listed_t<kDot, B>(la, blocks, lds, st);
}

template <int METRIC, int B>
static hipError_t launch_sq8_listed_groups_t(const Sq8Args& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q, size_t lds,
                                             hipStream_t st) {
  static bool done = false;
  if (lds > 64 * 1024 && !done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_sq8_listed_groups<METRIC, B>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    done = true;
  }
  hipLaunchKernelGGL((sweep_topk_sq8_listed_groups<METRIC, B>), dim3(n_items), dim3(256), lds, st, a, items, lists_per_q);
  return hipGetLastError();
}
template <int B>
static hipError_t launch_sq8_listed_groups_m(int metric, const Sq8Args& a, const ListedGroupItem* items, uint32_t n_items, uint32_t lists_per_q,
                                             size_t lds, hipStream_t st) {
  if (metric == kCosine) return launch_sq8_listed_groups_t<kCosine, B>(a, items, n_items, lists_per_q, lds, st);
  if (metric == kEuclidean) return launch_sq8_listed_groups_t<kEuclidean, B>(a, items, n_items, lists_per_q, lds, st);
  return launch_sq8_listed_groups_t<kDot, B>(a, items, n_items, lists_per_q, lds, st);
}

// ---- selection stage over the SQ8 storage mode (select_stage.hip brute_split_dev, level 3) -------------------------------------
// The dequantised rows d = code * scale + min as a bf16 image (what the matrix cores select on), their norms sqrt(nsq), and
// the first kSplitSeedRows dequantised rows in f32 (what the exact matrix-core kernel seeds the thresholds from).
// Euclidean (aug): the augmented form of sweep_split.hip — image rows of dim + 64 (slots dim, dim + 1 = hi / lo of -nsq / 2), seed
// rows of dim + 4 (slot dim = -nsq / 2)
__global__ __launch_bounds__(256) void sq8_dequant_rows(const uint8_t* codes, uint64_t code_stride, const float* vmin, const float* vmax,
                                                        const float* nsq, uint16_t* img, float* nrm, float* seed, uint32_t seed_rows,
                                                        uint32_t row0, uint32_t n_rows, uint32_t dim, uint32_t dim_a, uint32_t dim_s,
                                                        uint32_t* rho_max_bits) {
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t r = wave; r < n_rows; r += nwaves) {
    const uint32_t row = row0 + r;
    double se = 0.0, sx = 0.0;  // the dequantised row's bf16 rounding residual ratio (sweep_split.hip select_eps_q)
    const float mn = vmin[row], range = __fsub_rn(vmax[row], mn);
    const bool flat = range < kF32Eps;
    const float scale = __fdiv_rn(range, 255.0f);
    const uint8_t* c = codes + (size_t)row * code_stride;
    for (uint32_t i = lane * 4; i < dim; i += 256) {  // dim % 4 == 0 (selection needs dim % 64 == 0)
      const uint32_t w = *reinterpret_cast<const uint32_t*>(c + i);
      float d[4];
#pragma unroll
      for (int e = 0; e < 4; e++) d[e] = flat ? mn : __fadd_rn(__fmul_rn((float)((w >> (8 * e)) & 0xFFu), scale), mn);
      uint32_t h[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {  // round to nearest even; NaN stays NaN
        uint32_t u = __float_as_uint(d[e]);
        h[e] = (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x0040u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
        const float de = d[e] - __uint_as_float(h[e] << 16);  // exact in f32
        se += (double)de * (double)de;
        sx += (double)d[e] * (double)d[e];
      }
      *reinterpret_cast<uint2*>(img + (size_t)row * dim_a + i) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
      if (row < seed_rows) *reinterpret_cast<float4*>(seed + (size_t)row * dim_s + i) = make_float4(d[0], d[1], d[2], d[3]);
    }
    if (dim_a > dim) {
      const float hh = -0.5f * nsq[row];
      uint32_t u = __float_as_uint(hh);
      const uint32_t hi = (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x0040u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
      u = __float_as_uint(hh - __uint_as_float(hi << 16));
      const uint32_t lo = (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x0040u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
      if (dim + lane < dim_a) img[(size_t)row * dim_a + dim + lane] = lane == 0 ? (uint16_t)hi : (lane == 1 ? (uint16_t)lo : (uint16_t)0);
      if (row < seed_rows && lane < 4 && dim + lane < dim_s) seed[(size_t)row * dim_s + dim + lane] = lane == 0 ? hh : 0.0f;
    }
    if (lane == 0) nrm[row] = sqrtf(nsq[row]);
    if (rho_max_bits) {
#pragma unroll
      for (int s2 = 32; s2 > 0; s2 >>= 1) {
        se += __shfl_xor(se, s2, 64);
        sx += __shfl_xor(sx, s2, 64);
      }
      if (lane == 0 && sx > 0.0) {
        const float rho = (float)(sqrt(se / sx) * 1.0000002);
        if (rho == rho && rho < __uint_as_float(0x7F800000u)) atomicMax(rho_max_bits, __float_as_uint(rho));
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static void quantize_range(vdb_hip_index* ix, uint64_t first, uint64_t n) {
  if (n == 0) return;
  const int blocks = (int)std::min<uint64_t>((n + 3) / 4, 4096);
  if (ix->storage_mode == VDB_STORAGE_SQ8) {
    hipLaunchKernelGGL(sq8_quantize_rows, dim3(blocks), dim3(256), 0, ix->stream, ix->rows.as<float>(), ix->row_stride,
                       ix->sq8_codes.as<uint8_t>(), ix->sq8_stride, ix->sq8_min.as<float>(), ix->sq8_max.as<float>(),
                       (uint32_t)first, (uint32_t)n, ix->dim);
    hipLaunchKernelGGL(sq8_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, ix->sq8_codes.as<uint8_t>(),
                       ix->sq8_stride, ix->sq8_min.as<float>(), ix->sq8_max.as<float>(), ix->sq8_nsq.as<float>(),
                       (uint32_t)first, (uint32_t)n, ix->dim);
  } else if (ix->storage_mode == VDB_STORAGE_BINARY) {
    hipLaunchKernelGGL(sign_bits_rows, dim3(blocks), dim3(256), 0, ix->stream, ix->rows.as<float>(), ix->row_stride,
                       ix->sign_bits.as<uint32_t>(), ix->words, (uint32_t)first, (uint32_t)n, ix->dim);
  }
}

// grows the quantised arrays with the index and encodes rows [first, first + n)
int32_t storage_mode_append(vdb_hip_index* ix, uint64_t first, uint64_t n) {
  if (ix->storage_mode == VDB_STORAGE_FULL) return VDB_OK;
  const uint64_t cap = std::max<uint64_t>(ix->capacity, 1);
  hipError_t e = hipSuccess;
  if (ix->storage_mode == VDB_STORAGE_SQ8) {
    if ((e = ix->sq8_codes.reserve(cap * ix->sq8_stride, true, ix->stream)) != hipSuccess ||
        (e = ix->sq8_min.reserve(cap * 4, true, ix->stream)) != hipSuccess ||
        (e = ix->sq8_max.reserve(cap * 4, true, ix->stream)) != hipSuccess ||
        (e = ix->sq8_nsq.reserve(cap * 4, true, ix->stream)) != hipSuccess)
      return fail(VDB_ERR_OOM, std::string("SQ8 codes: ") + hipGetErrorString(e));
  } else {
    if ((e = ix->sign_bits.reserve(cap * ix->words * 4, true, ix->stream)) != hipSuccess)
      return fail(VDB_ERR_OOM, std::string("sign bits: ") + hipGetErrorString(e));
  }
  quantize_range(ix, first, n);
  if (first < ix->sq8_img_rows) ix->sq8_img_rows = first;  // codes rebuilt from `first`: the selection image follows at next use
  VDB_HIP(hipGetLastError());
  return VDB_OK;
}

// selection stage (level 3): bf16 image of the dequantised rows, their norms, the f32 seed prefix — built at first use,
// kept current by storage_mode_append
static int32_t ensure_sq8_select_impl(vdb_hip_index* ix, hipStream_t st);
int32_t ensure_sq8_select(vdb_hip_index* cx, hipStream_t st) {  // (inside a search: see select_stage.hip build_image_on_primary)
  vdb_hip_index* p = primary_of(cx);
  {
    std::lock_guard<std::mutex> il(p->img_mu);
    const bool stale = p->sq8_img.cap == 0 || p->sq8_img_rows < p->n_rows;
    const int32_t rc = ensure_sq8_select_impl(p, st);
    if (rc != VDB_OK) return rc;
    if (stale) VDB_HIP(hipStreamSynchronize(st));  // complete before another context may take the image over (index.hip)
    if (cx != p) copy_image_fields(cx, p);
  }
  if (!cx->sel_stats) {
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocDefault) != hipSuccess) return fail(VDB_ERR_OOM, "pinned selection statistics");
    memset(h, 0, 64);
    cx->sel_stats = static_cast<volatile uint32_t*>(h);
  }
  return VDB_OK;
}
static int32_t ensure_sq8_select_impl(vdb_hip_index* ix, hipStream_t st) {
  const uint64_t cap = std::max<uint64_t>(ix->capacity, 1) + kRowSlack;
  const bool aug = ix->metric == VDB_EUCLIDEAN;
  const uint32_t dim_a = aug ? ix->dim + 64 : ix->dim, dim_s = aug ? ix->dim + 4 : ix->dim;
  hipError_t e;
  if ((e = ix->sq8_img.reserve(cap * (size_t)dim_a * 2, true, st)) != hipSuccess ||
      (e = ix->sq8_nrm.reserve(cap * 4, true, st)) != hipSuccess ||
      (e = ix->sq8_seed.reserve((size_t)kSplitSeedRows * dim_s * 4, true, st)) != hipSuccess)
    return fail(VDB_ERR_OOM, std::string("SQ8 selection image: ") + hipGetErrorString(e));
  if (!ix->sq8_rho.p) {  // (the image is built from row 0 behind this: every row contributes)
    if ((e = ix->sq8_rho.reserve(256, false, st)) != hipSuccess || (e = hipMemsetAsync(ix->sq8_rho.p, 0, 256, st)) != hipSuccess)
      return fail(VDB_ERR_OOM, std::string("SQ8 residual bound: ") + hipGetErrorString(e));
    ix->sq8_img_rows = 0;
  }
  if (ix->sq8_img_rows < ix->n_rows) {
    const uint64_t first = ix->sq8_img_rows, n = ix->n_rows - first;
    const int blocks = (int)std::min<uint64_t>((n + 3) / 4, 4096);
    hipLaunchKernelGGL(sq8_dequant_rows, dim3(blocks), dim3(256), 0, st, ix->sq8_codes.as<uint8_t>(), ix->sq8_stride,
                       ix->sq8_min.as<float>(), ix->sq8_max.as<float>(), ix->sq8_nsq.as<float>(), ix->sq8_img.as<uint16_t>(),
                       ix->sq8_nrm.as<float>(), ix->sq8_seed.as<float>(), kSplitSeedRows, (uint32_t)first, (uint32_t)n, ix->dim, dim_a, dim_s,
                       ix->sq8_rho.as<uint32_t>());
    ix->sq8_img_rows = ix->n_rows;
    VDB_HIP(hipGetLastError());
  }
  return VDB_OK;
}

// the reference chain for the queries flagged by a selection batch, decided on the device: list them, one gathered launch of
// the exact SQ8 sweep (block rows without a listed query exit at once), merge per listed query, scatter.  qmap / fin.qcount / fin.qslot:
// the list the re-scoring launch made (sweep_split.hip list_unproven); fin: the batch's last launch, completed and issued here
int32_t sq8_fallback_flagged(vdb_hip_index* ix, const float* d_q, uint64_t q_stride, uint32_t nqg, uint32_t k, const uint32_t* qmap,
                             const SelectFinishArgs& fin_in, hipStream_t st) {
  SelectFinishArgs fin = fin_in;
  const uint32_t* qcount = fin.qcount;
  const uint8_t* alive = search_alive(ix);  // (a filtered call's row mask: the exact pass must not let disallowed rows back in)
  int B = 8;
  if (sq8_lds_bytes(8, k, ix->dim) > 160 * 1024) B = 4;
  if (B == 4 && sq8_lds_bytes(4, k, ix->dim) > 160 * 1024) B = 1;
  const size_t lds = sq8_lds_bytes(B, k, ix->dim);
  if (lds > 160 * 1024) return fail(VDB_ERR_UNSUPPORTED, "SQ8 search: dim / k too large for the LDS query tile");
  const uint32_t ngroups = (uint32_t)((ix->n_rows + 63) / 64);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds, 4));
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ngroups + 3) / 4, (int64_t)ix->n_cus * per_cu));
  const int qgroups = (int)((nqg + (uint32_t)B - 1) / (uint32_t)B);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 15) & ~(size_t)15;
    return o;
  };
  const size_t o_keys = take((size_t)nqg * blocks * k * 8), o_ids = take((size_t)nqg * k * 8), o_sc = take((size_t)nqg * k * 4),
               o_n = take((size_t)nqg * 4);
  hipError_t e;
  if ((e = ix->s_fb_keys.reserve(off, false, st)) != hipSuccess) return fail(VDB_ERR_OOM, "SQ8 fallback scratch");
  unsigned char* sd = ix->s_fb_keys.as<unsigned char>();
  Sq8Args a{};
  a.codes = ix->sq8_codes.as<uint8_t>();
  a.vmin = ix->sq8_min.as<float>();
  a.vmax = ix->sq8_max.as<float>();
  a.nsq = ix->sq8_nsq.as<float>();
  a.alive = alive;
  a.queries = d_q;
  a.part_keys = reinterpret_cast<uint64_t*>(sd + o_keys);
  a.code_stride = ix->sq8_stride;
  a.q_stride = q_stride;
  a.n_rows = (uint32_t)ix->n_rows;
  a.dim = ix->dim;
  a.nq = (uint32_t)B;
  a.k = k;
  a.qmap = qmap;
  a.qcount = qcount;
  e = B == 8 ? launch_sq8_m<8>(ix->metric, a, blocks, lds, st, qgroups)
             : (B == 4 ? launch_sq8_m<4>(ix->metric, a, blocks, lds, st, qgroups) : launch_sq8_m<1>(ix->metric, a, blocks, lds, st, qgroups));
  if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("SQ8 fallback sweep launch: ") + hipGetErrorString(e));
  MergeArgs m{};
  m.part_keys = a.part_keys;
  m.ext_ids = ix->ext_ids.as<uint64_t>();
  m.out_ids = reinterpret_cast<uint64_t*>(sd + o_ids);
  m.out_scores = reinterpret_cast<float*>(sd + o_sc);
  m.out_n = reinterpret_cast<uint32_t*>(sd + o_n);
  m.n_lists = (uint32_t)blocks;
  m.k = k;
  m.active = qcount;
  launch_merge(ix->metric != VDB_EUCLIDEAN, m, nqg, st);
  fin.g_ids = m.out_ids;
  fin.g_scores = m.out_scores;
  fin.g_n = m.out_n;
  launch_select_finish(fin, st);
  VDB_HIP(hipGetLastError());
  return VDB_OK;
}

// the SQ8 codes of the handle and the slice's queries; the caller sets alive and part_keys (nq and k: the slice's)
static Sq8Args sq8_args(const vdb_hip_index* ix, const QuerySlice& c) {
  Sq8Args a{};
  a.codes = ix->sq8_codes.as<uint8_t>();
  a.vmin = ix->sq8_min.as<float>();
  a.vmax = ix->sq8_max.as<float>();
  a.nsq = ix->sq8_nsq.as<float>();
  a.queries = c.d_q;
  a.code_stride = ix->sq8_stride;
  a.q_stride = c.q_stride;
  a.n_rows = (uint32_t)ix->n_rows;
  a.dim = ix->dim;
  a.nq = c.nq;
  a.k = c.k;
  return a;
}

int32_t brute_sq8_dev(vdb_hip_index* ix, const QuerySlice& s, hipStream_t st) {
  if (ix->storage_mode != VDB_STORAGE_SQ8) return fail(VDB_ERR_STATE, "SQ8 search: set the storage mode to SQ8 first");
  if (ix->metric != VDB_COSINE && ix->metric != VDB_EUCLIDEAN && ix->metric != VDB_DOT)
    return fail(VDB_ERR_UNSUPPORTED, "SQ8 search: Cosine, Euclidean and DotProduct only");
  if (s.nq == 0) return VDB_OK;
  if (s.k == 0 || ix->n_rows == 0) return zero_results(s, st);
  const uint32_t k = s.k;
  for (uint32_t q0 = 0; q0 < s.nq;) {
    int B = s.nq - q0 >= 8 ? 8 : (s.nq - q0 >= 4 ? 4 : 1);
    if (B == 8 && sq8_lds_bytes(8, k, ix->dim) > 160 * 1024) B = 4;
    if (B == 4 && sq8_lds_bytes(4, k, ix->dim) > 160 * 1024) B = 1;
    const size_t lds = sq8_lds_bytes(B, k, ix->dim);
    if (lds > 160 * 1024) return fail(VDB_ERR_UNSUPPORTED, "SQ8 search: dim / k too large for the LDS query tile");
    const QuerySlice c = s.sub(q0, std::min<uint32_t>((uint32_t)B, s.nq - q0));
    const uint32_t ngroups = (uint32_t)((ix->n_rows + 63) / 64);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds, 4));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ngroups + 3) / 4, (int64_t)ix->n_cus * per_cu));
    if (ix->s_part_keys.reserve((size_t)B * blocks * k * 8, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "top-k scratch");
    Sq8Args a = sq8_args(ix, c);
    a.alive = search_alive(ix);
    a.part_keys = ix->s_part_keys.as<uint64_t>();
    const int32_t rc = timed_launch(ix, 0, st, "SQ8 sweep launch", [&] {  // (VDB_KERNEL_SQ8: the caller's)
      return B == 8 ? launch_sq8_m<8>(ix->metric, a, blocks, lds, st)
                    : (B == 4 ? launch_sq8_m<4>(ix->metric, a, blocks, lds, st) : launch_sq8_m<1>(ix->metric, a, blocks, lds, st));
    });
    if (rc != VDB_OK) return rc;
    merge_pass(ix, ix->metric != VDB_EUCLIDEAN, a.part_keys, nullptr, (uint32_t)blocks, c, st);
    q0 += c.nq;
  }
  VDB_HIP(hipGetLastError());
  return VDB_OK;
}

// The listed route of a filtered SQ8 call (vdb_hip_index_search_batch_filtered_mode): sweep_topk_sq8_listed over the
// filter's ascending row list, pass by pass (mode_listed_plan, vdb_filter_route.hpp), merge_topk behind every pass.  The caller has
// checked the storage mode, the metric, k > 0 and count > 0, and that the plan of the first pass fits.
int32_t brute_sq8_listed_dev(vdb_hip_index* ix, const uint32_t* list, uint32_t count, const QuerySlice& s, hipStream_t st) {
  const uint32_t k = s.k;
  for (uint32_t q0 = 0; q0 < s.nq;) {
    const ModeListedPlan lp = mode_listed_plan(false, ix->dim, k, count, s.nq - q0, ix->n_cus);
    if (lp.blocks == 0) return fail(VDB_ERR_UNSUPPORTED, "SQ8 search: dim / k too large for the LDS query tile");
    if (ix->s_part_keys.reserve((size_t)lp.B * lp.blocks * k * 8, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "top-k scratch");
    const QuerySlice c = s.sub(q0, lp.nq_pass);
    Sq8ListedArgs la{};
    la.a = sq8_args(ix, c);
    la.a.alive = ix->any_dead ? ix->alive.as<uint8_t>() : nullptr;  // rows removed since the filter was made
    la.a.part_keys = ix->s_part_keys.as<uint64_t>();
    la.list = list;
    la.count = count;
    la.per_block = lp.per_block;
    const int32_t rc = timed_launch(ix, VDB_KERNEL_SWEEP_LISTED, st, "listed SQ8 sweep launch", [&] {
      return lp.B == 8 ? launch_sq8_listed_m<8>(ix->metric, la, lp.blocks, (size_t)lp.lds, st)
                       : (lp.B == 4 ? launch_sq8_listed_m<4>(ix->metric, la, lp.blocks, (size_t)lp.lds, st)
                                    : launch_sq8_listed_m<1>(ix->metric, la, lp.blocks, (size_t)lp.lds, st));
    });
    if (rc != VDB_OK) return rc;
    merge_pass(ix, ix->metric != VDB_EUCLIDEAN, la.a.part_keys, nullptr, (uint32_t)lp.blocks, c, st);
    q0 += c.nq;
  }
  VDB_HIP(hipGetLastError());
  return VDB_OK;
}

// One grouped launch of a call with one filter per query (vdb_hip_index_search_batch_filters_mode): block b does items[b]
// (device memory; mode_groups_plan).  s: the staged queries of the call — a query is addressed by its position in it; part_keys:
// [call's queries][lists_per_q][k], pre-filled with invalid keys.  The caller has checked the storage mode, the metric and k > 0.
int32_t sq8_listed_groups_launch(vdb_hip_index* ix, int B, const QuerySlice& s, uint64_t* part_keys, const ListedGroupItem* items, uint32_t n_items,
                                 uint32_t lists_per_q, hipStream_t st) {
  if ((B != 8 && B != 4 && B != 1) || n_items == 0 || lists_per_q == 0) return fail(VDB_ERR_INVALID_ARG, "grouped listed SQ8 sweep: bad launch");
  const size_t lds = sq8_lds_bytes(B, s.k, ix->dim);
  if (lds > 160 * 1024) return fail(VDB_ERR_UNSUPPORTED, "SQ8 search: dim / k too large for the LDS query tile");
  Sq8Args a = sq8_args(ix, s);
  a.alive = ix->any_dead ? ix->alive.as<uint8_t>() : nullptr;  // rows removed since the filters were made
  a.part_keys = part_keys;
  return timed_launch(ix, VDB_KERNEL_SWEEP_LISTED_GROUPS, st, "grouped listed SQ8 sweep launch", [&] {
    return B == 8 ? launch_sq8_listed_groups_m<8>(ix->metric, a, items, n_items, lists_per_q, lds, st)
                  : (B == 4 ? launch_sq8_listed_groups_m<4>(ix->metric, a, items, n_items, lists_per_q, lds, st)
                            : launch_sq8_listed_groups_m<1>(ix->metric, a, items, n_items, lists_per_q, lds, st));
  });
}

// the four-bit image of the sign-bit codes (bits_gemm.hip: batches of >= 32 queries run on the matrix cores), in the storage mode's
// image buffers (vdb_index.hpp); built at first use, extended lazily behind inserts — inside a search: see index.hip
// build_image_on_primary for why a build is complete before the image is handed on
static int32_t ensure_sign_image(vdb_hip_index* cx, hipStream_t st) {
  vdb_hip_index* p = primary_of(cx);
  std::lock_guard<std::mutex> il(p->img_mu);
  const bool stale = p->sq8_img.cap == 0 || p->sq8_img_rows < p->n_rows;
  const uint64_t cap = std::max<uint64_t>(p->capacity, 1) + kRowSlack;
  const uint32_t stride = bits_image_stride(p->dim);
  hipError_t e;
  if ((e = p->sq8_img.reserve(cap * (size_t)stride, true, st)) != hipSuccess || (e = p->sq8_nrm.reserve(cap * 4, true, st)) != hipSuccess)
    return fail(VDB_ERR_OOM, std::string("sign-bit image: ") + hipGetErrorString(e));
  if (p->sq8_img_rows < p->n_rows) {
    launch_bits_expand(VDB_HAMMING, p->sign_bits.as<uint32_t>(), p->words, p->sq8_img.as<uint8_t>(), stride, p->sq8_nrm.as<float>(), (uint32_t)p->sq8_img_rows,
                       (uint32_t)(p->n_rows - p->sq8_img_rows), p->dim, 0.0f, st);
    p->sq8_img_rows = p->n_rows;
    VDB_HIP(hipGetLastError());
  }
  if (stale) VDB_HIP(hipStreamSynchronize(st));
  if (cx != p) copy_image_fields(cx, p);
  return VDB_OK;
}

// the queries' sign bits, by the kernel that encodes rows
static void pack_queries_as_signs(const vdb_hip_index* ix, const QuerySlice& s, uint32_t* qbits, hipStream_t st) {
  hipLaunchKernelGGL(sign_bits_rows, dim3((unsigned)std::min<uint32_t>((s.nq + 3) / 4, 4096)), dim3(256), 0, st, s.d_q, s.q_stride, qbits, ix->words, 0u,
                     s.nq, ix->dim);
}

// BinaryQuantizedVector::hamming_distance between the sign bits of the queries and of every row: the packed-bit path of index.hip
// (brute_bits_dev: one-launch kernel, four-bit GEMM on the matrix cores, vector-ALU plan) over the sign-bit array — scores = distance
// as f32, smallest first
int32_t brute_binary_dev(vdb_hip_index* ix, const QuerySlice& s, hipStream_t st) {
  if (ix->storage_mode != VDB_STORAGE_BINARY) return fail(VDB_ERR_STATE, "Binary search: set the storage mode to Binary first");
  if (s.nq == 0) return VDB_OK;
  if (s.k == 0 || ix->n_rows == 0) return zero_results(s, st);
  const BitsSource src{ix->sign_bits.as<uint32_t>(), pack_queries_as_signs, VDB_HAMMING, ensure_sign_image, &vdb_hip_index::sq8_img, &vdb_hip_index::sq8_nrm,
                       /*sign_rule=*/1u, /*higher_is_better=*/false, "one-launch sign-bit search", "sign-bit sweep launch"};
  return brute_bits_dev(ix, src, s, st);
}


}  // namespace vdb

using namespace vdb;

extern "C" {

// StorageMode of a collection (quantization.rs:17-29; crud.rs:66-82 encodes every upserted vector accordingly)
int32_t vdb_hip_index_set_storage_mode(vdb_hip_index* ix, int32_t mode) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix) return fail(VDB_ERR_INVALID_ARG, "null argument");
  if (mode != VDB_STORAGE_FULL && mode != VDB_STORAGE_SQ8 && mode != VDB_STORAGE_BINARY)
    return fail(VDB_ERR_INVALID_ARG, "bad storage mode");
  if (ix->group) return group_for_all(ix, 2, (uint32_t)mode);
  std::lock_guard<vdb::IndexMutex> g(ix->mu);
  if (ix->storage_mode == mode) return VDB_OK;
  VDB_ENTER(ix);
  for (DevBuf* b : {&ix->sq8_codes, &ix->sq8_min, &ix->sq8_max, &ix->sq8_nsq, &ix->sign_bits, &ix->sq8_img, &ix->sq8_nrm, &ix->sq8_seed})
    b->release();
  ix->sq8_img_rows = 0;
  ix->storage_mode = mode;
  ix->sq8_stride = ((uint64_t)ix->dim + 15) / 16 * 16;
  int32_t rc = storage_mode_append(ix, 0, ix->n_rows);
  if (rc != VDB_OK) {
    ix->storage_mode = VDB_STORAGE_FULL;
    return rc;
  }
  VDB_HIP(hipStreamSynchronize(ix->stream));
  return VDB_OK;
  });
}

// The stored code of one vector in the reference's byte format: QuantizedVector::to_bytes (min f32, max f32, dim
// bytes; quantization.rs:289-295) or BinaryQuantizedVector::to_bytes (dimension u32, ceil(dim/8) bytes; :155-169).
int32_t vdb_hip_index_get_quantized(vdb_hip_index* ix, uint64_t id, uint8_t* out, size_t cap, size_t* len) {
  return vdb::guarded([&]() -> int32_t {
  if (!ix || !len) return fail(VDB_ERR_INVALID_ARG, "null argument");
  if (ix->group) {  // every shard that holds the id holds the same code
    for (size_t s = 0; s < group_size(ix); s++) {
      int32_t rc = vdb_hip_index_get_quantized(group_shard(ix, s), id, out, cap, len);
      if (rc == VDB_OK || s + 1 == group_size(ix)) return rc;
    }
  }
  std::lock_guard<vdb::IndexMutex> g(ix->mu);
  if (ix->storage_mode == VDB_STORAGE_FULL) return fail(VDB_ERR_STATE, "storage mode is Full: nothing is quantised");
  auto it = ix->id_to_idx.find(id);
  if (it == ix->id_to_idx.end()) return fail(VDB_ERR_INVALID_ARG, "unknown id");
  const uint64_t row = it->second;
  const size_t need = ix->storage_mode == VDB_STORAGE_SQ8 ? 8 + (size_t)ix->dim : 4 + ((size_t)ix->dim + 7) / 8;
  *len = need;
  if (!out || cap < need) return fail(VDB_ERR_INVALID_ARG, "buffer too small");
  VDB_ENTER(ix);
  if (ix->storage_mode == VDB_STORAGE_SQ8) {
    VDB_HIP(hipMemcpyAsync(out, ix->sq8_min.as<float>() + row, 4, hipMemcpyDeviceToHost, ix->stream));
    VDB_HIP(hipMemcpyAsync(out + 4, ix->sq8_max.as<float>() + row, 4, hipMemcpyDeviceToHost, ix->stream));
    VDB_HIP(hipMemcpyAsync(out + 8, ix->sq8_codes.as<uint8_t>() + row * ix->sq8_stride, ix->dim, hipMemcpyDeviceToHost, ix->stream));
  } else {
    const uint32_t d = ix->dim;
    std::memcpy(out, &d, 4);
    VDB_HIP(hipMemcpyAsync(out + 4, ix->sign_bits.as<uint32_t>() + row * ix->words, need - 4, hipMemcpyDeviceToHost, ix->stream));
  }
  VDB_HIP(hipStreamSynchronize(ix->stream));
  return VDB_OK;
  });
}

}  // extern "C"
