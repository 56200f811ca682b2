// sweep_bits_gathered.hip — the GATHERED four-bit matrix-core tier of a filtered search over packed bits: Hamming / Jaccard indexes
// (vdb_hip_index_search_batch_filtered) and the Binary storage mode (vdb_hip_index_search_batch_filtered_mode with
// VDB_SEARCH_BRUTE_BINARY), both under VDB_OPT_FILTER_ROUTE = 3; DESIGN 4.1t.
//
// A GEMM of (the filter's ascending row list) x (the batch's queries) over dim on v_mfma_scale_f32_16x16x128_f8f6f4 with a fused
// top-k.  The streaming four-bit kernel (sweep_topk_gemm_bf16_pp<.., FP4>, bits_gemm.hip) reads a prebuilt image of 4 bits per value
// of EVERY row by LDS-DMA; this one reads the PACKED rows (dim / 8 bytes each) of the listed rows only and expands them to E2M1
// nibbles on the way into LDS.  No image of the rows is built or read.
//
// Work split (that of sweep_half_gathered.hip, DESIGN 4.1s: the plan is shared).  256 threads = four waves.  A block owns ONE query
// tile of TN queries (blockIdx.y; TN = 128 for chunks of >= 64 queries, 16 below) and ONE contiguous span of per_block tiles of 64
// listed rows (blockIdx.x); the TN k-lists stay in LDS for the whole span.  Wave w owns rows 16 w .. 16 w + 15 of every tile across
// the query tile: TN / 16 accumulator tiles.
//
// Operands.  K-SLICES of 256 values: one 128-B line of nibbles per row / query = 8 packed words of a row = two MFMA steps of 128
// values, double-buffered, ONE barrier per slice.  A 16-byte slot of a line is one packed word expanded, and it is exactly what one
// lane of a fragment holds: lane (i = lane & 15, kk = lane >> 4) of step m takes slot 4 m + kk of line i.
//   rows: thread -> (line tid >> 3 (+ 32), slot tid & 7) loads ONE word bits[row * words + 8 ks + slot] (zero at or past `words`), the
//   row taken from the tile's index list; the word waits in a register while the current slice is multiplied, is spread to nibbles by
//   shifts and masks (bits_spread8, four times) and written to the other buffer behind the products.  Jaccard {0, +1}: nibble = 0x2
//   per set bit.  Hamming {-1, +1}: 0x2 per set bit, 0xA per clear bit of a column < dim, 0x0 for the columns at or past dim.  Value
//   i of a word sits in nibble i of its 16 bytes — bits_expand_kernel's order, which the query image was written in.
//   queries: 16-byte pieces of the query image (launch_bits_expand over the packed queries, once per chunk); queries past the batch
//   and pieces past the image's stride are zeros.
// Bank conflicts: hg_slot's swizzle — logical slot s of line r lives in physical slot s ^ ((r >> 1) & 7).  A fragment read has lanes
// 0-15 on slot s of lines r0 .. r0 + 15: eight line pairs on eight physical slots, the two lines of a pair 128 B apart — sixteen
// different 16-byte columns of the 256-B bank row.  A staging write has eight lanes on the eight slots of one line.
//
// Row bit counts (Jaccard): popcount of the words as they are loaded, summed over the slices in a register, over the eight lanes of
// a line by three lane exchanges, one f32 per row of the tile in LDS when the tile's last slice has been loaded.
// Arithmetic: f32 accumulators hold exact integers; the finish of seed_scores_fp4 / g16_protocol.inc.  Hamming 0.5f * (dim - x),
// smallest first; Jaccard uni = qn + cnt - x, uni == 0 ? 1.0f : x / uni, largest first.
// Epilogue: scores are exact, so the quick reject is the FINISHED key against the list's k-th key, no margin: first against the
// bound read once per tile (list_tau_relaxed), then against the fresh one; `alive` is read where a key would enter a list;
// shared_list_offer.  Positions past the list's end were loaded as its last row and are never offered.  Partial lists [nq][spans][k].
#include <algorithm>

#include "vdb_device.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

typedef float f32x4_bg __attribute__((ext_vector_type(4)));
typedef int i32x8_bg __attribute__((ext_vector_type(8)));

constexpr int kBgRows = 64;      // listed rows per tile
constexpr int kBgSlice = 256;    // values of dim per slice: 128 B of nibbles per line, 8 packed words of a row
constexpr int kBgThreads = 256;
static_assert(kBgRows == (int)kHgTileRows && kBgThreads / 64 * 16 == kBgRows, "four waves, a 16-row strip each; the plan counts 64-row tiles");

struct BitsGatherArgs {
  const uint32_t* bits;     // [n_rows][words] packed rows
  const uint8_t* alive;     // nullable
  const uint32_t* list;     // [count] ascending rows
  const uint8_t* qimg;      // [nq][q_stride] nibble image of the queries (launch_bits_expand)
  const float* qcnt;        // [nq] Jaccard: the queries' bit counts; Hamming: dim
  uint64_t* part_keys;      // [nq][spans][k]
  uint32_t words, q_stride; // words of a packed row; bytes of a query's image (a multiple of 128)
  uint32_t count, dim, nq, k;
  uint32_t per_block;       // row tiles per span
};

// byte offset of logical 16-byte slot `slot` of line `line` in a slab of 128-B lines (sweep_half_gathered.hip hg_slot)
__device__ __forceinline__ uint32_t bg_slot(uint32_t line, uint32_t slot) { return line * 128u + ((slot ^ ((line >> 1) & 7u)) << 4); }

// bit i of the low byte of b -> bit 4 i (the low bit of nibble i)
__device__ __forceinline__ uint32_t bits_spread8(uint32_t b) {
  b &= 0xFFu;
  b = (b | (b << 12)) & 0x000F000Fu;
  b = (b | (b << 6)) & 0x03030303u;
  return (b | (b << 3)) & 0x11111111u;
}
// one packed word -> 32 E2M1 nibbles.  valid: the word's columns below dim (Hamming; unused for Jaccard)
template <int METRIC>
__device__ __forceinline__ uint4 bits_to_nibbles(uint32_t h, uint32_t valid) {
  uint32_t o[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const uint32_t s = bits_spread8(h >> (8 * g));
    if (METRIC == kHamming) {
      const uint32_t n = bits_spread8(valid >> (8 * g)) & ~s;  // clear bits of real columns: -1.0 = 0xA
      o[g] = ((s | n) << 1) | (n << 3);
    } else {
      o[g] = s << 1;                                           // +1.0 = 0x2
    }
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int METRIC, int TN>
__global__ __launch_bounds__(kBgThreads, 2) void sweep_topk_bits_gathered(BitsGatherArgs a) {
  constexpr bool HIB = METRIC != kHamming;
  constexpr int NT = TN / 16;                                  // accumulator tiles of a wave
  constexpr int BP = TN * 8 / kBgThreads > 0 ? TN * 8 / kBgThreads : 1;  // 16-byte query pieces per thread and slice (4, or 1 for threads < 128)
  constexpr uint32_t A_BYTES = kBgRows * 128, B_BYTES = TN * 128, BUF = A_BYTES + B_BYTES;
  static_assert(BUF == hg_slab_bytes(TN) / 2, "the plan's LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS: two slab buffers (rows | queries) | lists [TN][k] | cnts [TN] | locks [TN] | tile rows [3][64] | tile bit counts [3][64]
  const uint32_t k = a.k;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem + 2 * BUF);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(smem + 2 * BUF + (size_t)TN * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 4);
  uint32_t* trow = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 8);  // row of every tile position
  float* tcnt = reinterpret_cast<float*>(trow + 3 * kBgRows);

  const uint32_t tid = threadIdx.x;
  const int lane = lane_id();
  const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t q0 = blockIdx.y * (uint32_t)TN;
  const uint32_t ntiles = (a.count + kBgRows - 1) / kBgRows;
  const uint32_t tile0 = blockIdx.x * a.per_block;             // (the plan leaves no block without a tile)
  const uint32_t my_tiles = tile0 < ntiles ? min(a.per_block, ntiles - tile0) : 0u;
  const uint32_t KS = (a.dim + kBgSlice - 1) / kBgSlice;
  const uint32_t total = my_tiles * KS;

  if (tid < (uint32_t)TN) {
    cnts[tid] = 0;
    locks[tid] = 0;
  }
  // the tile's rows: positions past the end take the list's last row (never offered)
  auto stage_meta = [&](uint32_t t) {
    if (tid < (uint32_t)kBgRows) {
      const uint64_t pos = (uint64_t)(tile0 + t) * kBgRows + tid;
      trow[(t % 3u) * kBgRows + tid] = a.list[pos < a.count ? pos : (uint64_t)a.count - 1];
    }
  };
  // staging: thread -> line tid >> 3 (+ 32 per piece), slot tid & 7: eight lanes fetch the eight words / the 128-B line of a slice
  const uint32_t st_line = tid >> 3, st_slot = tid & 7u;
  uint32_t ra[2], ra_word = 0, pop[2] = {0u, 0u};
  uint4 rb[BP];
  auto load_step = [&](uint32_t t, uint32_t ks) {
    ra_word = ks * 8u + st_slot;                               // this thread's word of the row
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t row = trow[(t % 3u) * kBgRows + st_line + 32u * j];
      ra[j] = ra_word < a.words ? a.bits[(size_t)row * a.words + ra_word] : 0u;
      if (METRIC == kJaccard) {
        pop[j] = (ks == 0 ? 0u : pop[j]) + (uint32_t)__popc(ra[j]);
        if (ks + 1 == KS) {                                    // the row's last slice: its bit count, over the eight lanes of the line
          uint32_t c = pop[j];
          c += (uint32_t)__shfl_xor((int)c, 1);
          c += (uint32_t)__shfl_xor((int)c, 2);
          c += (uint32_t)__shfl_xor((int)c, 4);
          if (st_slot == 0) tcnt[(t % 3u) * kBgRows + st_line + 32u * j] = (float)c;
        }
      }
    }
    const uint32_t col = ks * 128u + st_slot * 16u;            // first byte of this thread's pieces of the query image
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      const bool live = b < (uint32_t)TN && q0 + b < a.nq && col < a.q_stride;
      rb[j] = live ? *reinterpret_cast<const uint4*>(a.qimg + (size_t)(q0 + b) * a.q_stride + col) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_step = [&](uint32_t buf) {
    unsigned char* base = smem + buf * BUF;
    const uint32_t c0 = ra_word * 32u;                         // the word's first column
    const uint32_t valid = c0 + 32u <= a.dim ? 0xFFFFFFFFu : (c0 >= a.dim ? 0u : (1u << (a.dim - c0)) - 1u);
#pragma unroll
    for (int j = 0; j < 2; j++) *reinterpret_cast<uint4*>(base + bg_slot(st_line + 32u * j, st_slot)) = bits_to_nibbles<METRIC>(ra[j], valid);
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      if (b < (uint32_t)TN) *reinterpret_cast<uint4*>(base + A_BYTES + bg_slot(b, st_slot)) = rb[j];
    }
  };

  if (my_tiles) stage_meta(0);
  __syncthreads();
  if (total) {
    load_step(0, 0);
    store_step(0);
  }
  float qn_t[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const uint32_t b = q0 + t * 16 + (lane & 15);
    qn_t[t] = b < a.nq ? a.qcnt[b] : 0.0f;
  }
  __syncthreads();

  // fragment reads: lane (i = lane & 15, kk = lane >> 4) takes values 128 m + 32 kk .. + 31 = logical slot 4 m + kk of line i
  const uint32_t fi = (uint32_t)lane & 15u, fkk = (uint32_t)lane >> 4;
  uint32_t step = 0;
  for (uint32_t t = 0; t < my_tiles; t++) {
    f32x4_bg acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = f32x4_bg{0.f, 0.f, 0.f, 0.f};
    for (uint32_t ks = 0; ks < KS; ks++, step++) {
      if (ks == 0 && t + 1 < my_tiles) {  // the next tile's rows: slot (t + 1) % 3 last held tile t - 2, whose epilogue every wave has left
        stage_meta(t + 1);
        if (KS == 1) __syncthreads();     // (otherwise this slice's closing barrier publishes them in time)
      }
      const bool more = step + 1 < total;
      if (more) {
        if (ks + 1 < KS) load_step(t, ks + 1); else load_step(t + 1, 0);
      }
      const unsigned char* base = smem + (step & 1u) * BUF;
#pragma unroll
      for (uint32_t m = 0; m < 2; m++) {
        const uint4 av = *reinterpret_cast<const uint4*>(base + bg_slot(wib * 16u + fi, 4u * m + fkk));
        const i32x8_bg a8 = {(int)av.x, (int)av.y, (int)av.z, (int)av.w, 0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < NT; n++) {
          const uint4 bv = *reinterpret_cast<const uint4*>(base + A_BYTES + bg_slot((uint32_t)n * 16u + fi, 4u * m + fkk));
          const i32x8_bg b8 = {(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w, 0, 0, 0, 0};
          // (four-bit operands use the first four of the builtin's eight registers; unit block scales, as seed_scores_fp4)
          acc[n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc[n], 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        }
      }
      if (more) store_step((step + 1u) & 1u);  // the other buffer: its last readers left it before the previous barrier
      __syncthreads();
    }
    // ---- epilogue of the tile: acc[n][r] = row 16 wib + 4 (lane >> 4) + r of the tile x query q0 + 16 n + (lane & 15) ----
    const uint32_t* rows_t = trow + (t % 3u) * kBgRows;
    const float* cnt_t = tcnt + (t % 3u) * kBgRows;
    uint64_t tau_t[NT];
    asm volatile("" ::: "memory");  // (fresh, plain LDS reads issued together: vdb_device.hpp list_tau_relaxed)
#pragma unroll
    for (int n = 0; n < NT; n++) tau_t[n] = list_tau_relaxed(lists, cnts, (uint32_t)n * 16u + fi, k);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t rl = wib * 16u + 4u * fkk + (uint32_t)r;
      const bool in_list = (uint64_t)(tile0 + t) * kBgRows + rl < a.count;
      const uint32_t row = rows_t[rl];
      const float vc = METRIC == kJaccard ? cnt_t[rl] : 0.0f;
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const uint32_t b = (uint32_t)n * 16u + fi;
        const float x = acc[n][r];
        float score;
        if (METRIC == kHamming) {
          score = 0.5f * (qn_t[n] - x);  // (the finish of the selection kernel: g16_protocol.inc)
        } else {
          const float uni = qn_t[n] + vc - x;
          score = uni == 0.0f ? 1.0f : x / uni;
        }
        const uint64_t key = (in_list && q0 + b < a.nq) ? make_key<HIB>(score, row) : kKeyInvalid;
        uint64_t mask = __ballot(key < tau_t[n]);
        if (mask == 0) continue;
        const uint64_t tau = (cnts[b] == k) ? lists[(size_t)b * k + (k - 1)] : kKeyInvalid;
        mask = __ballot(key < tau);
        while (mask) {
          const int src = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const uint64_t kk = readlane64(key, src);
          if (a.alive && a.alive[key_row(kk)] == 0) continue;
          const int bb = n * 16 + (src & 15);
          shared_list_offer(lists + (size_t)bb * k, cnts + bb, locks + bb, k, kk, lane);
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t b = wib; b < (uint32_t)TN && q0 + b < a.nq; b += kBgThreads / 64) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + ((size_t)(q0 + b) * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = (uint32_t)lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}

template <int METRIC, int TN>
static hipError_t launch_bg_t(const BitsGatherArgs& a, const HalfGatherPlan& p, hipStream_t st) {
  static bool attr_done = false;
  if (p.lds > 64 * 1024 && !attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_topk_bits_gathered<METRIC, TN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFmLdsBudget);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  hipLaunchKernelGGL((sweep_topk_bits_gathered<METRIC, TN>), dim3(p.spans, p.qtiles), dim3(kBgThreads), (size_t)p.lds, st, a);
  return hipGetLastError();
}
template <int METRIC>
static hipError_t launch_bg_m(const BitsGatherArgs& a, const HalfGatherPlan& p, hipStream_t st) {
  return p.TN == 128 ? launch_bg_t<METRIC, 128>(a, p, st) : launch_bg_t<METRIC, 16>(a, p, st);
}

hipError_t launch_sweep_bits_gathered(int metric, const HalfGatherPlan& p, const uint32_t* bits, uint32_t words, const uint8_t* alive,
                                      const uint32_t* list, uint32_t count, const uint8_t* qimg, uint32_t q_stride, const float* qcnt,
                                      uint64_t* part_keys, uint32_t dim, uint32_t nq, uint32_t k, hipStream_t st) {
  if (p.blocks == 0 || (p.TN != 128 && p.TN != 16) || (metric != kHamming && metric != kJaccard) || count == 0 || nq == 0 || nq > p.qtiles * (uint32_t)p.TN ||
      (uint64_t)p.spans * p.per_block * kBgRows < count || p.lds != hg_lds_bytes(p.TN, k) || p.lds > kFmLdsBudget || q_stride % 128u != 0 ||
      (uint64_t)words * 32u < dim)
    return hipErrorInvalidValue;  // (a plan that does not cover the call: nothing is launched)
  BitsGatherArgs a{bits, alive, list, qimg, qcnt, part_keys, words, q_stride, count, dim, nq, k, p.per_block};
  return metric == kHamming ? launch_bg_m<kHamming>(a, p, st) : launch_bg_m<kJaccard>(a, p, st);
}

}  // namespace vdb
