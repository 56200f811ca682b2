// sweep_gathered.hip — the GATHERED matrix-core tiers of filtered exact search (VDB_OPT_FILTER_ROUTE = 3), all three in this file:
//   half: Cosine / DotProduct over the f16 / bf16 row image (vdb_hip_index_search_batch_filtered_mode with
//   VDB_SEARCH_BRUTE_F16 / _BF16), v_mfma_f32_16x16x32_f16 / _bf16 — sweep_topk_half_gathered;
//   four-bit: Hamming / Jaccard indexes (vdb_hip_index_search_batch_filtered) and the Binary storage mode
//   (VDB_SEARCH_BRUTE_BINARY) over PACKED bits, v_mfma_scale_f32_16x16x128_f8f6f4 — sweep_topk_bits_gathered;
//   f32: Cosine / DotProduct over the f32 rows of a handle that answers in mode M (vdb_hip_index_search_batch_filtered),
//   v_mfma_f32_16x16x4_f32 in the chain's own order — sweep_topk_f32_gathered.
// The three kernels share the plan, the constants, the slot swizzle, the launch helper and the plan check below.  Their BODIES are
// written three times, the same pipeline statement for statement: folding them into one forced-inline body with an operand policy
// was tried and changed the register allocation of most instances, so a fix to the pipeline is made in all of them.
//
// The pipeline.  A GEMM of (the filter's ascending row list) x (the batch's queries) over dim with a fused top-k: only the listed rows
// are read.  The streaming kernels of these modes keep the queries x the WHOLE dim in LDS (sweep.hip sweep_topk_mfma_bf16: dim
// classes, 96 queries per pass of the rows) or read a prebuilt image of EVERY row (bits_gemm.hip); this one slices dim, so its LDS
// footprint does not depend on dim and one launch serves every query of a chunk of <= 1 024.
//
// Work split.  256 threads = four waves.  A block owns ONE query tile of TN queries (blockIdx.y; TN = 128 for chunks of >= 64
// queries, 16 below) and ONE contiguous span of the list, per_block row tiles of 64 listed rows (blockIdx.x); it walks the span tile
// by tile while the TN k-lists stay in LDS.  Wave w owns rows 16 w .. 16 w + 15 of every tile across the whole query tile: TN / 16
// accumulator tiles (32 registers at TN = 128).
//
// Operands.  Both go through LDS in K-SLICES of one 128-B line per row / query (64 half elements, 256 four-bit values, 32 f32), double-
// buffered: while slice s is multiplied the pieces of slice s + 1 are in flight in registers (the row taken from the tile's index
// list), written to the other buffer behind the products, ONE barrier per slice.  A line is eight 16-byte slots, and a slot is exactly
// what one lane of a fragment holds: lane (i = lane & 15, kk = lane >> 4) of MFMA step m takes slot 4 m + kk of line i, two steps per
// slice.  Staging: thread -> (line tid >> 3 (+ 32), slot tid & 7): eight lanes fetch one line.  Query pieces behind the image's stride
// and queries behind the batch are zeros (the image holds nq rows, nothing behind them is read).
// Bank conflicts.  Logical slot s of line r lives in physical slot s ^ ((r >> 1) & 7) (gt_slot).  A fragment read (ds_read_b128) has
// lanes 0-15 on logical slot s of lines r0 .. r0 + 15: the eight line pairs take eight different physical slots, the two lines of a
// pair sit 128 B apart, so sixteen lanes cover sixteen different 16-byte columns of the 256-B bank row — no conflict.  A staging write
// (ds_write_b128) has eight lanes on the eight slots of one line: two lines = 256 contiguous bytes.
// Tile rows.  The row index (and the per-row scalar) of every tile position lives in a ring of three slots: tile t + 1 is staged
// during slice 0 of tile t into slot (t + 1) % 3, which last held tile t - 2, whose epilogue every wave has left; the slice's closing
// barrier publishes it before the first load that needs it, except where a tile is ONE slice — then an extra barrier does.  Positions
// past the list's end take the list's last row and are never offered.
// Arithmetic.  A (row, query) pair is accumulated in ONE accumulator over dim in ascending slices, two MFMA steps per slice (f32: two
// steps of four instructions), whatever the instance, the tile or the position in the list.  A pair's score bits depend on the row,
// the query and dim only.
// Epilogue.  The bound of every list is read once per tile (list_tau_relaxed); a pair that the quick test lets pass is keyed, held
// against the list's fresh k-th key, and offered (shared_list_offer); `alive` is read where a key would enter a list (a listed row may
// have been soft-deleted since the filter was made).  Partial lists: [nq][spans][k].
//
// Half.  A row piece is 16 bytes of rows16 + row * stride, loaded as they are (global_load_dwordx4); pieces that start at or behind
// the stride are zeros (the image's pad columns inside the stride are zeros already), so every dim is served.  Per-row scalar: the norm
// of the rounded row, staged with the tile's rows; per-query: the norm of the rounded query (query_norms_bf16_kernel).  Quick test: the
// approximate score against the bound with sweep_topk_mfma_bf16's margin; finish_score_half with its kHalfNormEps rule.
// Four-bit.  A row piece is ONE packed word bits[row * words + 8 ks + slot] (zero at or past `words`); it waits in a register while
// the current slice is multiplied and is spread to 32 E2M1 nibbles by shifts and masks on its way into LDS (bits_spread8, four times)
// — no image of the rows is built or read.  Jaccard {0, +1}: nibble = 0x2 per set bit.  Hamming {-1, +1}: 0x2 per set bit, 0xA per
// clear bit of a column < dim, 0x0 for the columns at or past dim.  Value i of a word sits in nibble i of its 16 bytes —
// bits_expand_kernel's order, which the query image was written in (launch_bits_expand over the packed queries, once per chunk).
// Per-row scalar (Jaccard): the row's bit count — popcount of the words as they are loaded, summed over the slices in a register, over
// the eight lanes of a line by three lane exchanges, written when the tile's last slice has been loaded; per-query: the query's bit
// count (Hamming: dim).  f32 accumulators hold exact integers; the finish of seed_scores_fp4 / g16_protocol.inc: Hamming
// 0.5f * (dim - x), smallest first; Jaccard uni = qn + cnt - x, uni == 0 ? 1.0f : x / uni, largest first.  Scores are exact, so the
// quick test is the FINISHED key against the bound, no margin.
// f32.  A slice is 32 f32 elements of a row / query, a slot is one float4: a row piece is 16 bytes of rows + row * row_stride, a query
// piece 16 bytes of the caller's block; an element at or past dim is a zero in BOTH operands whatever the pad columns hold (the
// mask of listed_body_m's fetch; a query's last piece is read element by element).  Lane (i, kk) takes logical slot 4 m' + kk of
// line i for m' = 0, 1: elements 32 s + 16 m' + 4 kk .. + 3, and issues four v_mfma_f32_16x16x4_f32, component c = 0 .. 3 of the row
// piece with component c of the query piece.  One instruction adds a pair's four products in the order kk = 0 .. 3, so a pair's
// accumulator runs ONE chain over k = 32 s + 16 m' + 4 kk + c in the order s, m', c, kk = oracle mode M's U, m, c, kk (a 128-block
// is four slices): the score bits of sweep_topk_mfma_f32 and sweep_topk_listed_m.  The chain's zero padding up to a multiple of 128
// is executed inside the last slice and SKIPPED behind it: a padded step adds +0 * +0 = +0 to the accumulator, which changes no
// bit of it — x + (+0) = x for every x but -0, NaN and inf included, and the accumulator is never -0: it starts at +0 and a
// round-to-nearest sum is -0 only when both terms are.  Per-row scalar: norms[row] (Cosine), staged with the tile's rows; per-query:
// the mode-C norm (query_norms_f32_kernel: the chain of listed_body_m's prologue).  finish_score; scores are exact, so the quick test
// is the finished key against the bound, no margin (the four-bit tier's form).
#include <algorithm>

#include "vdb_device.hpp"
#include "vdb_filter_route.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kGtRows = 64;       // listed rows per tile
constexpr int kHgSlice = 64;      // half: elements of dim per slice (128 B per line)
constexpr int kBgSlice = 256;     // four-bit: values of dim per slice: 128 B of nibbles per line, 8 packed words of a row
constexpr int kGtThreads = 256;
static_assert(kGtRows == (int)kHgTileRows && kGtThreads / 64 * 16 == kGtRows, "four waves, a 16-row strip each; the plan counts 64-row tiles");

// byte offset of logical 16-byte slot `slot` of line `line` in a slab of 128-B lines
__device__ __forceinline__ uint32_t gt_slot(uint32_t line, uint32_t slot) { return line * 128u + ((slot ^ ((line >> 1) & 7u)) << 4); }

// ---- half ----
struct HalfGatherArgs {
  const uint16_t* rows;     // [n_rows + slack][row_stride] f16 / bf16, row_stride % 8 == 0
  const float* norms;       // [n_rows] norms of the rounded rows (Cosine)
  const uint8_t* alive;     // nullable
  const uint32_t* list;     // [count] ascending rows
  const uint16_t* queries;  // [nq][q_stride] rounded queries (round_queries_bf16)
  const float* qnorms;      // [nq] norms of the rounded queries (Cosine)
  uint64_t* part_keys;      // [nq][spans][k]
  uint64_t row_stride, q_stride;  // elements
  uint32_t count, dim, nq, k;
  uint32_t per_block;       // row tiles per span
};

template <int METRIC, bool F16, int TN>
__global__ __launch_bounds__(kGtThreads, 2) void sweep_topk_half_gathered(HalfGatherArgs a) {
  constexpr bool HIB = true;
  constexpr int NT = TN / 16;                                  // accumulator tiles of a wave
  constexpr int BP = TN * 8 / kGtThreads > 0 ? TN * 8 / kGtThreads : 1;  // 16-byte query pieces per thread and slice (4, or 1 for threads < 128)
  constexpr uint32_t A_BYTES = kGtRows * 128, B_BYTES = TN * 128, BUF = A_BYTES + B_BYTES;
  static_assert(BUF == hg_slab_bytes(TN) / 2, "the plan's LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS: two slab buffers (rows | queries) | lists [TN][k] | cnts [TN] | locks [TN] | tile rows [3][64] | tile norms [3][64]
  const uint32_t k = a.k;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem + 2 * BUF);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(smem + 2 * BUF + (size_t)TN * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 4);
  uint32_t* trow = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 8);  // row of every tile position
  float* tvn = reinterpret_cast<float*>(trow + 3 * kGtRows);

  const uint32_t tid = threadIdx.x;
  const int lane = lane_id();
  const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t q0 = blockIdx.y * (uint32_t)TN;
  const uint32_t ntiles = (a.count + kGtRows - 1) / kGtRows;
  const uint32_t tile0 = blockIdx.x * a.per_block;             // (the plan leaves no block without a tile)
  const uint32_t my_tiles = tile0 < ntiles ? min(a.per_block, ntiles - tile0) : 0u;
  const uint32_t KS = (a.dim + kHgSlice - 1) / kHgSlice;
  const uint32_t total = my_tiles * KS;

  if (tid < (uint32_t)TN) {
    cnts[tid] = 0;
    locks[tid] = 0;
  }
  // the tile's rows and their norms: positions past the end take the list's last row (masked in the epilogue)
  auto stage_meta = [&](uint32_t t) {
    if (tid < (uint32_t)kGtRows) {
      const uint64_t pos = (uint64_t)(tile0 + t) * kGtRows + tid;
      const uint32_t row = a.list[pos < a.count ? pos : (uint64_t)a.count - 1];
      trow[(t % 3u) * kGtRows + tid] = row;
      tvn[(t % 3u) * kGtRows + tid] = METRIC == kCosine ? a.norms[row] : 1.0f;
    }
  };
  // staging: thread -> line tid >> 3 (+ 32 per piece), slot tid & 7: eight lanes fetch one 128-B line
  const uint32_t st_line = tid >> 3, st_slot = tid & 7u;
  uint4 ra[2], rb[BP];
  auto load_step = [&](uint32_t t, uint32_t ks) {
    const uint32_t col = ks * kHgSlice + st_slot * 8;          // first element of this thread's pieces
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t row = trow[(t % 3u) * kGtRows + st_line + 32u * j];
      ra[j] = col < (uint32_t)a.row_stride ? *reinterpret_cast<const uint4*>(a.rows + (size_t)row * a.row_stride + col) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      const bool live = b < (uint32_t)TN && q0 + b < a.nq && col < (uint32_t)a.q_stride;
      rb[j] = live ? *reinterpret_cast<const uint4*>(a.queries + (size_t)(q0 + b) * a.q_stride + col) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_step = [&](uint32_t buf) {
    unsigned char* base = smem + buf * BUF;
#pragma unroll
    for (int j = 0; j < 2; j++) *reinterpret_cast<uint4*>(base + gt_slot(st_line + 32u * j, st_slot)) = ra[j];
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      if (b < (uint32_t)TN) *reinterpret_cast<uint4*>(base + A_BYTES + gt_slot(b, st_slot)) = rb[j];
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
    qn_t[t] = (METRIC == kCosine && b < a.nq) ? a.qnorms[b] : 0.0f;
  }
  __syncthreads();

  // fragment reads: lane (i = lane & 15, kk = lane >> 4) takes elements 32 m + 8 kk .. + 7 = logical slot 4 m + kk of line i
  const uint32_t fi = (uint32_t)lane & 15u, fkk = (uint32_t)lane >> 4;
  uint32_t step = 0;
  for (uint32_t t = 0; t < my_tiles; t++) {
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        const uint4 av = *reinterpret_cast<const uint4*>(base + gt_slot(wib * 16u + fi, 4u * m + fkk));
#pragma unroll
        for (int n = 0; n < NT; n++) {
          const uint4 bv = *reinterpret_cast<const uint4*>(base + A_BYTES + gt_slot((uint32_t)n * 16u + fi, 4u * m + fkk));
          if (F16)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), acc[n], 0, 0, 0);
          else
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc[n], 0, 0, 0);
        }
      }
      if (more) store_step((step + 1u) & 1u);  // the other buffer: its last readers left it before the previous barrier
      __syncthreads();
    }
    // ---- epilogue of the tile: acc[n][r] = row 16 wib + 4 (lane >> 4) + r of the tile x query q0 + 16 n + (lane & 15) ----
    const uint32_t* rows_t = trow + (t % 3u) * kGtRows;
    const float* vn_t = tvn + (t % 3u) * kGtRows;
    float tau_f[NT];
    asm volatile("" ::: "memory");  // (fresh, plain LDS reads issued together: vdb_device.hpp list_tau_relaxed)
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const uint64_t tk = list_tau_relaxed(lists, cnts, (uint32_t)n * 16u + fi, k);
      tau_f[n] = tk != kKeyInvalid ? key_score<HIB>(tk) : __uint_as_float(0xFF800000u);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t rl = wib * 16u + 4u * fkk + (uint32_t)r;
      const bool in_list = (uint64_t)(tile0 + t) * kGtRows + rl < a.count;
      const uint32_t row = rows_t[rl];
      const float vn = vn_t[rl];
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const uint32_t b = (uint32_t)n * 16u + fi;
        const float dotv = acc[n][r];
        const float rq = (METRIC == kCosine) ? __builtin_amdgcn_rcpf(qn_t[n] * vn) : 1.0f;
        const float approx = dotv * rq;
        const float margin = fabsf(tau_f[n]) * 1.9073486e-6f + 1e-37f;
        // (a norm below f32::EPSILON makes the score 0.0 whatever the dot product: never filtered by the approximation)
        const bool tiny = METRIC == kCosine && (qn_t[n] < kHalfNormEps || vn < kHalfNormEps);
        const bool maybe = (tiny || !(approx < tau_f[n] - margin)) && in_list && q0 + b < a.nq;
        uint64_t mask = __ballot(maybe);
        if (mask == 0) continue;
        const float score = finish_score_half<METRIC>(dotv, qn_t[n], vn);
        const uint64_t key = maybe ? make_key<HIB>(score, row) : kKeyInvalid;
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
  for (uint32_t b = wib; b < (uint32_t)TN && q0 + b < a.nq; b += kGtThreads / 64) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + ((size_t)(q0 + b) * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = (uint32_t)lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}

// ---- four-bit ----
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
__global__ __launch_bounds__(kGtThreads, 2) void sweep_topk_bits_gathered(BitsGatherArgs a) {
  constexpr bool HIB = METRIC != kHamming;
  constexpr int NT = TN / 16;                                  // accumulator tiles of a wave
  constexpr int BP = TN * 8 / kGtThreads > 0 ? TN * 8 / kGtThreads : 1;  // 16-byte query pieces per thread and slice (4, or 1 for threads < 128)
  constexpr uint32_t A_BYTES = kGtRows * 128, B_BYTES = TN * 128, BUF = A_BYTES + B_BYTES;
  static_assert(BUF == hg_slab_bytes(TN) / 2, "the plan's LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS: two slab buffers (rows | queries) | lists [TN][k] | cnts [TN] | locks [TN] | tile rows [3][64] | tile bit counts [3][64]
  const uint32_t k = a.k;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem + 2 * BUF);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(smem + 2 * BUF + (size_t)TN * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 4);
  uint32_t* trow = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 8);  // row of every tile position
  float* tcnt = reinterpret_cast<float*>(trow + 3 * kGtRows);

  const uint32_t tid = threadIdx.x;
  const int lane = lane_id();
  const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t q0 = blockIdx.y * (uint32_t)TN;
  const uint32_t ntiles = (a.count + kGtRows - 1) / kGtRows;
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
    if (tid < (uint32_t)kGtRows) {
      const uint64_t pos = (uint64_t)(tile0 + t) * kGtRows + tid;
      trow[(t % 3u) * kGtRows + tid] = a.list[pos < a.count ? pos : (uint64_t)a.count - 1];
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
      const uint32_t row = trow[(t % 3u) * kGtRows + st_line + 32u * j];
      ra[j] = ra_word < a.words ? a.bits[(size_t)row * a.words + ra_word] : 0u;
      if (METRIC == kJaccard) {
        pop[j] = (ks == 0 ? 0u : pop[j]) + (uint32_t)__popc(ra[j]);
        if (ks + 1 == KS) {                                    // the row's last slice: its bit count, over the eight lanes of the line
          uint32_t c = pop[j];
          c += (uint32_t)__shfl_xor((int)c, 1);
          c += (uint32_t)__shfl_xor((int)c, 2);
          c += (uint32_t)__shfl_xor((int)c, 4);
          if (st_slot == 0) tcnt[(t % 3u) * kGtRows + st_line + 32u * j] = (float)c;
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
    for (int j = 0; j < 2; j++) *reinterpret_cast<uint4*>(base + gt_slot(st_line + 32u * j, st_slot)) = bits_to_nibbles<METRIC>(ra[j], valid);
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      if (b < (uint32_t)TN) *reinterpret_cast<uint4*>(base + A_BYTES + gt_slot(b, st_slot)) = rb[j];
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
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        const uint4 av = *reinterpret_cast<const uint4*>(base + gt_slot(wib * 16u + fi, 4u * m + fkk));
        const i32x8 a8 = {(int)av.x, (int)av.y, (int)av.z, (int)av.w, 0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < NT; n++) {
          const uint4 bv = *reinterpret_cast<const uint4*>(base + A_BYTES + gt_slot((uint32_t)n * 16u + fi, 4u * m + fkk));
          const i32x8 b8 = {(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w, 0, 0, 0, 0};
          // (four-bit operands use the first four of the builtin's eight registers; unit block scales, as seed_scores_fp4)
          acc[n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc[n], 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        }
      }
      if (more) store_step((step + 1u) & 1u);  // the other buffer: its last readers left it before the previous barrier
      __syncthreads();
    }
    // ---- epilogue of the tile: acc[n][r] = row 16 wib + 4 (lane >> 4) + r of the tile x query q0 + 16 n + (lane & 15) ----
    const uint32_t* rows_t = trow + (t % 3u) * kGtRows;
    const float* cnt_t = tcnt + (t % 3u) * kGtRows;
    uint64_t tau_t[NT];
    asm volatile("" ::: "memory");  // (fresh, plain LDS reads issued together: vdb_device.hpp list_tau_relaxed)
#pragma unroll
    for (int n = 0; n < NT; n++) tau_t[n] = list_tau_relaxed(lists, cnts, (uint32_t)n * 16u + fi, k);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t rl = wib * 16u + 4u * fkk + (uint32_t)r;
      const bool in_list = (uint64_t)(tile0 + t) * kGtRows + rl < a.count;
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
  for (uint32_t b = wib; b < (uint32_t)TN && q0 + b < a.nq; b += kGtThreads / 64) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + ((size_t)(q0 + b) * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = (uint32_t)lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}

// ---- f32 ----
constexpr int kFgSlice = 32;      // f32: elements of dim per slice (128 B per line)
struct F32GatherArgs {
  const float* rows;        // [n_rows + slack][row_stride] f32, 16-byte aligned rows
  const float* norms;       // [n_rows] mode-C norms of the rows (Cosine)
  const uint8_t* alive;     // nullable
  const uint32_t* list;     // [count] ascending rows
  const float* queries;     // [nq][q_stride] the chunk's queries, 16-byte aligned
  const float* qnorms;      // [nq] mode-C norms of the queries (Cosine; query_norms_f32_kernel)
  uint64_t* part_keys;      // [nq][spans][k]
  uint64_t row_stride, q_stride;  // elements
  uint32_t count, dim, nq, k;
  uint32_t per_block;       // row tiles per span
};

// the canonical (mode C) norm of every query of a chunk, one wave per query: float4 chunk c on lane c % 64, predicated tail, the xor
// butterfly, the root — the bits listed_body_m and sweep_topk_mfma_f32 compute in their prologues
__global__ __launch_bounds__(256) void query_norms_f32_kernel(const float* queries, uint64_t q_stride, float* out, uint32_t nq, uint32_t dim) {
  const int lane = lane_id();
  const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= nq) return;
  const float* qp = queries + (size_t)b * q_stride;
  float nacc = 0.0f;
  for (uint32_t c = (uint32_t)lane; c * 4u < dim; c += 64u)
#pragma unroll
    for (uint32_t e = 0; e < 4; e++)
      if (c * 4u + e < dim) nacc = __builtin_fmaf(qp[c * 4u + e], qp[c * 4u + e], nacc);
  const float n = sqrtf(butterfly_all(nacc));
  if (lane == 0) out[b] = n;
}

template <int METRIC, int TN>
__global__ __launch_bounds__(kGtThreads, 2) void sweep_topk_f32_gathered(F32GatherArgs a) {
  constexpr bool HIB = true;
  constexpr int NT = TN / 16;                                  // accumulator tiles of a wave
  constexpr int BP = TN * 8 / kGtThreads > 0 ? TN * 8 / kGtThreads : 1;  // 16-byte query pieces per thread and slice (4, or 1 for threads < 128)
  constexpr uint32_t A_BYTES = kGtRows * 128, B_BYTES = TN * 128, BUF = A_BYTES + B_BYTES;
  static_assert(BUF == hg_slab_bytes(TN) / 2, "the plan's LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS: two slab buffers (rows | queries) | lists [TN][k] | cnts [TN] | locks [TN] | tile rows [3][64] | tile norms [3][64]
  const uint32_t k = a.k;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem + 2 * BUF);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(smem + 2 * BUF + (size_t)TN * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 4);
  uint32_t* trow = reinterpret_cast<uint32_t*>(smem + 2 * BUF + (size_t)TN * k * 8 + (size_t)TN * 8);  // row of every tile position
  float* tvn = reinterpret_cast<float*>(trow + 3 * kGtRows);

  const uint32_t tid = threadIdx.x;
  const int lane = lane_id();
  const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t q0 = blockIdx.y * (uint32_t)TN;
  const uint32_t ntiles = (a.count + kGtRows - 1) / kGtRows;
  const uint32_t tile0 = blockIdx.x * a.per_block;             // (the plan leaves no block without a tile)
  const uint32_t my_tiles = tile0 < ntiles ? min(a.per_block, ntiles - tile0) : 0u;
  const uint32_t KS = (a.dim + kFgSlice - 1) / kFgSlice;      // (the chain's all-zero slices behind it are skipped: the head comment)
  const uint32_t total = my_tiles * KS;

  if (tid < (uint32_t)TN) {
    cnts[tid] = 0;
    locks[tid] = 0;
  }
  // the tile's rows and their norms: positions past the end take the list's last row (masked in the epilogue)
  auto stage_meta = [&](uint32_t t) {
    if (tid < (uint32_t)kGtRows) {
      const uint64_t pos = (uint64_t)(tile0 + t) * kGtRows + tid;
      const uint32_t row = a.list[pos < a.count ? pos : (uint64_t)a.count - 1];
      trow[(t % 3u) * kGtRows + tid] = row;
      tvn[(t % 3u) * kGtRows + tid] = METRIC == kCosine ? a.norms[row] : 1.0f;
    }
  };
  // staging: thread -> line tid >> 3 (+ 32 per piece), slot tid & 7: eight lanes fetch one 128-B line
  const uint32_t st_line = tid >> 3, st_slot = tid & 7u;
  float4 ra[2], rb[BP];
  auto load_step = [&](uint32_t t, uint32_t ks) {
    const uint32_t e0 = ks * kFgSlice + st_slot * 4;           // first element of this thread's pieces
    const bool whole = e0 + 4 <= a.dim;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t row = trow[(t % 3u) * kGtRows + st_line + 32u * j];
      float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (e0 < a.dim) {
        w = ld4(a.rows + (size_t)row * a.row_stride + e0);
        if (!whole) {  // the vector ends inside this piece: what follows is the chain's zero padding, whatever the pad columns hold
          if (e0 + 1 >= a.dim) w.y = 0.0f;
          if (e0 + 2 >= a.dim) w.z = 0.0f;
          w.w = 0.0f;
        }
      }
      ra[j] = w;
    }
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (b < (uint32_t)TN && q0 + b < a.nq && e0 < a.dim) {
        const float* qp = a.queries + (size_t)(q0 + b) * a.q_stride + e0;
        if (whole) {
          w = ld4(qp);
        } else {       // (nothing at or past dim is read from the caller's block)
          w.x = qp[0];
          if (e0 + 1 < a.dim) w.y = qp[1];
          if (e0 + 2 < a.dim) w.z = qp[2];
        }
      }
      rb[j] = w;
    }
  };
  auto store_step = [&](uint32_t buf) {
    unsigned char* base = smem + buf * BUF;
#pragma unroll
    for (int j = 0; j < 2; j++) *reinterpret_cast<float4*>(base + gt_slot(st_line + 32u * j, st_slot)) = ra[j];
#pragma unroll
    for (int j = 0; j < BP; j++) {
      const uint32_t b = st_line + 32u * j;
      if (b < (uint32_t)TN) *reinterpret_cast<float4*>(base + A_BYTES + gt_slot(b, st_slot)) = rb[j];
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
    qn_t[t] = (METRIC == kCosine && b < a.nq) ? a.qnorms[b] : 0.0f;
  }
  __syncthreads();

  // fragment reads: lane (i = lane & 15, kk = lane >> 4) takes elements 16 m + 4 kk .. + 3 = logical slot 4 m + kk of line i
  const uint32_t fi = (uint32_t)lane & 15u, fkk = (uint32_t)lane >> 4;
  uint32_t step = 0;
  for (uint32_t t = 0; t < my_tiles; t++) {
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        const f32x4 av = *reinterpret_cast<const f32x4*>(base + gt_slot(wib * 16u + fi, 4u * m + fkk));
        f32x4 bv[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) bv[n] = *reinterpret_cast<const f32x4*>(base + A_BYTES + gt_slot((uint32_t)n * 16u + fi, 4u * m + fkk));
        // (c outside, the tiles inside: every accumulator's chain keeps the order c = 0 .. 3, and neighbouring instructions are independent)
#pragma unroll
        for (int c = 0; c < 4; c++) {
#pragma unroll
          for (int n = 0; n < NT; n++) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[n][c], acc[n], 0, 0, 0);
        }
      }
      if (more) store_step((step + 1u) & 1u);  // the other buffer: its last readers left it before the previous barrier
      __syncthreads();
    }
    // ---- epilogue of the tile: acc[n][r] = row 16 wib + 4 (lane >> 4) + r of the tile x query q0 + 16 n + (lane & 15) ----
    const uint32_t* rows_t = trow + (t % 3u) * kGtRows;
    const float* vn_t = tvn + (t % 3u) * kGtRows;
    uint64_t tau_t[NT];
    asm volatile("" ::: "memory");  // (fresh, plain LDS reads issued together: vdb_device.hpp list_tau_relaxed)
#pragma unroll
    for (int n = 0; n < NT; n++) tau_t[n] = list_tau_relaxed(lists, cnts, (uint32_t)n * 16u + fi, k);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t rl = wib * 16u + 4u * fkk + (uint32_t)r;
      const bool in_list = (uint64_t)(tile0 + t) * kGtRows + rl < a.count;
      const uint32_t row = rows_t[rl];
      const float vn = vn_t[rl];
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const uint32_t b = (uint32_t)n * 16u + fi;
        const float score = finish_score<METRIC>(acc[n][r], qn_t[n], vn);
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
  for (uint32_t b = wib; b < (uint32_t)TN && q0 + b < a.nq; b += kGtThreads / 64) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + ((size_t)(q0 + b) * gridDim.x + blockIdx.x) * k;
    for (uint32_t e = (uint32_t)lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
}

// ---- launching, once for the sixteen instances ----
// one instance: the opt-in above 64 KiB of dynamic LDS once, grid = spans x qtiles
template <class Args, void (*KERNEL)(Args)>
static hipError_t launch_gathered(const Args& a, const HalfGatherPlan& p, hipStream_t st) {
  static bool attr_done = false;
  if (p.lds > 64 * 1024 && !attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFmLdsBudget);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(p.spans, p.qtiles), dim3(kGtThreads), (size_t)p.lds, st, a);
  return hipGetLastError();
}
template <int METRIC, bool F16>
static hipError_t launch_half_tn(const HalfGatherArgs& a, const HalfGatherPlan& p, hipStream_t st) {
  return p.TN == 128 ? launch_gathered<HalfGatherArgs, sweep_topk_half_gathered<METRIC, F16, 128>>(a, p, st)
                     : launch_gathered<HalfGatherArgs, sweep_topk_half_gathered<METRIC, F16, 16>>(a, p, st);
}
template <int METRIC>
static hipError_t launch_bits_tn(const BitsGatherArgs& a, const HalfGatherPlan& p, hipStream_t st) {
  return p.TN == 128 ? launch_gathered<BitsGatherArgs, sweep_topk_bits_gathered<METRIC, 128>>(a, p, st)
                     : launch_gathered<BitsGatherArgs, sweep_topk_bits_gathered<METRIC, 16>>(a, p, st);
}
template <int METRIC>
static hipError_t launch_f32_tn(const F32GatherArgs& a, const HalfGatherPlan& p, hipStream_t st) {
  return p.TN == 128 ? launch_gathered<F32GatherArgs, sweep_topk_f32_gathered<METRIC, 128>>(a, p, st)
                     : launch_gathered<F32GatherArgs, sweep_topk_f32_gathered<METRIC, 16>>(a, p, st);
}
// does the plan cover the call?  (one that does not: nothing is launched)
static bool plan_covers(const HalfGatherPlan& p, uint32_t count, uint32_t nq, uint32_t k) {
  return p.blocks != 0 && (p.TN == 128 || p.TN == 16) && count != 0 && nq != 0 && nq <= p.qtiles * (uint32_t)p.TN &&
         (uint64_t)p.spans * p.per_block * kGtRows >= count && p.lds == hg_lds_bytes(p.TN, k) && p.lds <= kFmLdsBudget;
}

hipError_t launch_sweep_half_gathered(int metric, bool f16, const HalfGatherPlan& p, const uint16_t* rows, uint64_t row_stride, const float* norms,
                                      const uint8_t* alive, const uint32_t* list, uint32_t count, const uint16_t* queries16, uint64_t q_stride,
                                      const float* qnorms, uint64_t* part_keys, uint32_t dim, uint32_t nq, uint32_t k, hipStream_t st) {
  if (!plan_covers(p, count, nq, k) || (metric != kCosine && metric != kDot)) return hipErrorInvalidValue;
  HalfGatherArgs a{rows, norms, alive, list, queries16, qnorms, part_keys, row_stride, q_stride, count, dim, nq, k, p.per_block};
  if (metric == kCosine) return f16 ? launch_half_tn<kCosine, true>(a, p, st) : launch_half_tn<kCosine, false>(a, p, st);
  return f16 ? launch_half_tn<kDot, true>(a, p, st) : launch_half_tn<kDot, false>(a, p, st);
}

hipError_t launch_sweep_bits_gathered(int metric, const HalfGatherPlan& p, const uint32_t* bits, uint32_t words, const uint8_t* alive,
                                      const uint32_t* list, uint32_t count, const uint8_t* qimg, uint32_t q_stride, const float* qcnt,
                                      uint64_t* part_keys, uint32_t dim, uint32_t nq, uint32_t k, hipStream_t st) {
  if (!plan_covers(p, count, nq, k) || (metric != kHamming && metric != kJaccard) || q_stride % 128u != 0 || (uint64_t)words * 32u < dim)
    return hipErrorInvalidValue;
  BitsGatherArgs a{bits, alive, list, qimg, qcnt, part_keys, words, q_stride, count, dim, nq, k, p.per_block};
  return metric == kHamming ? launch_bits_tn<kHamming>(a, p, st) : launch_bits_tn<kJaccard>(a, p, st);
}

void launch_query_norms_f32(const float* queries, uint64_t q_stride, float* out, uint32_t nq, uint32_t dim, hipStream_t st) {
  if (nq) hipLaunchKernelGGL(query_norms_f32_kernel, dim3((nq + 3) / 4), dim3(256), 0, st, queries, q_stride, out, nq, dim);
}

hipError_t launch_sweep_f32_gathered(int metric, const HalfGatherPlan& p, const float* rows, uint64_t row_stride, const float* norms,
                                     const uint8_t* alive, const uint32_t* list, uint32_t count, const float* queries, uint64_t q_stride,
                                     const float* qnorms, uint64_t* part_keys, uint32_t dim, uint32_t nq, uint32_t k, hipStream_t st) {
  // (16-byte pieces of both operands: strides in whole float4, as every f32 row block of the library is laid out)
  if (!plan_covers(p, count, nq, k) || (metric != kCosine && metric != kDot) || dim == 0 || row_stride % 4u != 0 || q_stride % 4u != 0 ||
      row_stride < ((uint64_t)dim + 3) / 4 * 4 || q_stride < dim || (reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(queries)) % 16u != 0)
    return hipErrorInvalidValue;
  F32GatherArgs a{rows, norms, alive, list, queries, qnorms, part_keys, row_stride, q_stride, count, dim, nq, k, p.per_block};
  return metric == kCosine ? launch_f32_tn<kCosine>(a, p, st) : launch_f32_tn<kDot>(a, p, st);
}

}  // namespace vdb
