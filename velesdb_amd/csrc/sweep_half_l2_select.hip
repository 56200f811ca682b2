// sweep_half_l2_select.hip — Euclidean batches over the f16 / bf16 image on the matrix cores, with the streaming kernel's bits
// (VDB_KERNEL_SELECT_HALF_L2).  sweep_topk_half_l2 re-reads the corpus once per 16 queries and spends a vector-ALU
// difference chain on every (row, query) pair; here the chain is spent only on the few rows that can be among a query's k nearest:
//
//   seed      sweep_topk_half_l2_tiles over the first kHalfL2SeedRows rows + the merge: the query's k best prefix rows, exact.
//   bound     half_l2_tau: the declared chain once more for the k-th of them gives its chain SUM D_k (not a re-squared root); with
//             s(q, v) = q.v - |v|^2 / 2 the selection score, every row with a chain sum <= D_k has s >= tau_q = (|q|^2 - D_k) / 2 -
//             delta_q (vdb_half_l2.hpp: the bound holds for every summation order of the matrix instruction).  The same launch writes
//             the rounded query image.  A NaN / inf in the query, fewer than k live prefix rows, a non-finite bound: the fallback.
//   select    half_l2_select: a 128-row x 128-query tiled GEMM over the image (v_mfma_f32_16x16x32_f16 / _bf16, f32 accumulators in
//             registers, fragments through LDS in double-buffered 64-element k-steps); the epilogue subtracts |v|^2 / 2 — less the
//             row's own share of the error bound, so a row of huge norm loosens no other row's test — and appends every
//             live row with !(s < tau_q) — and every row whose norm is not finite — to the query's survivor list in HBM.  No top-k
//             lists, no merges, no barrier but the k-step's.
//   re-score  half_l2_rescore: one block per query runs the declared chain (half_l2_chunk, the streaming kernel's own) over the listed
//             rows, a wave per row, keeps the k best (distance bits, row) and writes the answer in the merge's format.  The list holds
//             every row at or inside the k-th best prefix row's distance — so the true k nearest, equal distances included — and the
//             distances are the streaming kernel's bits: the answer is the streaming path's, bit for bit.
//   fallback  a query that was marked, or whose list overflowed, lists itself (as sweep_split.hip list_unproven) and leaves its f32
//             query in a gathered array; ONE launch of sweep_topk_half_l2_tiles over all rows serves any number of them (its block rows
//             past the count leave at once), the merge and select_finish hand them their answers and post the verdict.
// Nothing is read back and nothing synchronises.
#include <algorithm>

#include "vdb_half_l2.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

typedef float f32x4_h __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_h __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_h __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_h __attribute__((ext_vector_type(8)));

// ---- bound + query image: one wave per query (blocks past nq zero their row of the image: whole 128-query tiles are staged) ----------
struct HalfTauArgs {
  const uint16_t* rows;      // the half image
  const float* queries;      // f32 queries of the batch
  const uint64_t* seed_rows; // [nq][k] internal rows of the seed's answer, best first
  const uint32_t* seed_n;    // [nq]
  uint32_t* qcount;          // the fallback's count, cleared here
  uint16_t* q16;             // [nq padded to 128][row_stride] rounded queries
  float* tau;                // [padded]
  uint32_t* cnt;             // [padded] survivor counters, cleared here
  uint32_t* flags;           // [nq] 1 = fallback
  uint64_t row_stride, q_stride;
  uint32_t nq, k, dim;
};
template <bool F16>
__global__ __launch_bounds__(64) void half_l2_tau_kernel(HalfTauArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);  // [row_stride]
  const uint32_t q = blockIdx.x, lane = threadIdx.x, stride = (uint32_t)a.row_stride;
  uint16_t* qi = a.q16 + (size_t)q * stride;
  if (q >= a.nq) {
    for (uint32_t c = lane; c < stride; c += 64) qi[c] = 0;
    if (lane == 0) {
      a.tau[q] = __uint_as_float(0x7F800000u);
      a.cnt[q] = 0u;
    }
    return;
  }
  double qn2 = 0.0;
  bool bad = false;
  for (uint32_t c = lane; c < stride; c += 64) {
    const float x = c < a.dim ? half_round<F16>(a.queries[(size_t)q * a.q_stride + c]) : 0.0f;
    qs[c] = x;
    qi[c] = F16 ? __builtin_bit_cast(uint16_t, (_Float16)x) : (uint16_t)(__float_as_uint(x) >> 16);
    qn2 += (double)x * (double)x;
    bad |= !(fabsf(x) < __uint_as_float(0x7F800000u));
  }
  for (int s = 32; s >= 1; s >>= 1) qn2 += __shfl_xor(qn2, s, 64);
  bad = __ballot(bad) != 0ull;
  __syncthreads();
  bool marked = bad || a.seed_n[q] < a.k;
  float t = __uint_as_float(0x7F800000u);
  if (!marked) {  // (wave-uniform)
    const uint32_t row = (uint32_t)a.seed_rows[(size_t)q * a.k + (a.k - 1)];
    const uint16_t* rp = a.rows + (size_t)row * a.row_stride;
    float acc = 0.0f;
    for (uint32_t c = lane; c < stride / 8; c += 64) {
      float4 x0, x1;
      unpack8<F16>(*reinterpret_cast<const uint4*>(rp + (size_t)c * 8), x0, x1);
      acc = half_l2_chunk(acc, qs + (size_t)c * 8, x0, x1);
    }
    const float dk = butterfly_all(acc);  // the chain SUM of the k-th best prefix row, the streaming kernel's bits before the root
    t = half_l2_tau(a.dim, qn2, 0.0, (double)dk);  // (the row's own |v|^2 term of the bound is added to its score: half_l2_select)
    marked = !(dk < __uint_as_float(0x7F800000u)) || !(fabsf(t) < __uint_as_float(0x7F800000u));
  }
  if (lane == 0) {
    if (q == 0) *a.qcount = 0u;
    a.tau[q] = marked ? __uint_as_float(0x7F800000u) : t;  // (a marked query's list stays empty but for non-finite rows)
    a.cnt[q] = 0u;
    a.flags[q] = marked ? 1u : 0u;
  }
}

// ---- selection: 128 rows x 128 queries per four-wave block, a wave owns 64 x 64 (4 x 4 accumulator fragments, 64 registers) ----------
// Fragments and lane maps are the 128 x 128 kernel's of sweep_gemm.hip: a k-step is 64 two-byte elements = 128 bytes = eight 16-byte slots
// per row; slot s of row r sits at slot s ^ ((r >> 1) & 7) of the row's 128 LDS bytes; lane (i = l & 15, kk = l >> 4) feeds the 16-byte
// fragment (slot 4 m + kk, m = the 32-deep half of the step) of row 16 f + i to one v_mfma_f32_16x16x32; accumulator register r of lane
// l is (row 4 (l >> 4) + r, query l & 15) of its 16 x 16 fragment.  Two LDS buffers of 32 KiB: the loads of step i + 1 are in registers
// while step i multiplies, and are stored to the other buffer behind it — one barrier per step.  64 KiB per block, two blocks per CU.
struct HalfSelArgs {
  const uint16_t* rows;   // the half image; rows past n_rows up to the tile's end are readable (kRowSlack)
  const float* norms;     // norms of the ROUNDED rows (likewise)
  const uint8_t* alive;   // nullable
  const uint16_t* q16;    // [query tiles x 128][row_stride]
  const float* tau;       // [query tiles x 128]
  uint32_t* cnt;          // [query tiles x 128]
  uint32_t* lists;        // [nq][cap] survivor rows
  uint64_t row_stride;
  uint32_t cap, n_rows, nq, KT;  // KT = dim / 64 k-steps per row tile
  float hk;               // 1 - 16 dim 2^-24: a row's score is raised by its own share of the bound, delta_row = 8 dim 2^-24 |v|^2
};
template <bool F16>
__global__ __launch_bounds__(256, 2) void half_l2_select(HalfSelArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2][A 16 KiB | B 16 KiB]
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wib >> 1, wq = wib & 1;
  const uint32_t qt = blockIdx.y, G = gridDim.x;
  const uint32_t ntiles = (a.n_rows + 127u) / 128u;
  const uint32_t my_tiles = blockIdx.x < ntiles ? (ntiles - blockIdx.x + G - 1) / G : 0u;
  const uint32_t total = my_tiles * a.KT;
  if (!total) return;

  // staging: thread t moves the 16-byte slot (t & 7) of rows (t >> 3) + 32 j
  const int st_slot = tid & 7, st_row = tid >> 3;
  const size_t ld_off = ((size_t)st_row * a.row_stride + (size_t)st_slot * 8) * 2;
  const size_t ld_step = (size_t)32 * a.row_stride * 2;
  const unsigned char* const q_base = reinterpret_cast<const unsigned char*>(a.q16) + (size_t)qt * 128 * a.row_stride * 2 + ld_off;
  const uint32_t st_wr = (uint32_t)st_row * 128u + (uint32_t)((st_slot ^ ((st_row >> 1) & 7)) << 4);
  u32x4_h ra[4], rb[4];
  uint32_t ld_rt = blockIdx.x, ld_kt = 0;
  // (macros, not lambdas: hipcc does not always promote arrays captured by a lambda to registers)
#define VDB_HSEL_GLOAD() do { \
    const unsigned char* pa = reinterpret_cast<const unsigned char*>(a.rows) + ((size_t)ld_rt * 128 * a.row_stride + (size_t)ld_kt * 64) * 2 + ld_off; \
    const unsigned char* pb = q_base + (size_t)ld_kt * 128; \
_Pragma("unroll") \
    for (int j = 0; j < 4; j++) ra[j] = *reinterpret_cast<const u32x4_h*>(pa + j * ld_step); \
_Pragma("unroll") \
    for (int j = 0; j < 4; j++) rb[j] = *reinterpret_cast<const u32x4_h*>(pb + j * ld_step); \
    if (++ld_kt == a.KT) { \
      ld_kt = 0; \
      ld_rt += G; \
    } \
  } while (0)
#define VDB_HSEL_LSTORE(buf_) do { \
    unsigned char* d = smem + (buf_) * 32768u + st_wr; \
_Pragma("unroll") \
    for (int j = 0; j < 4; j++) *reinterpret_cast<u32x4_h*>(d + j * 4096) = ra[j]; \
_Pragma("unroll") \
    for (int j = 0; j < 4; j++) *reinterpret_cast<u32x4_h*>(d + 16384 + j * 4096) = rb[j]; \
  } while (0)
  // fragment reads
  const int fi = lane & 15, kk = lane >> 4, sw = (fi >> 1) & 7;
  const uint32_t rd_a = (uint32_t)(wr * 64 + fi) * 128u, rd_b = 16384u + (uint32_t)(wq * 64 + fi) * 128u;
  const uint32_t rd_s0 = (uint32_t)((kk ^ sw) << 4), rd_s1 = (uint32_t)(((4 + kk) ^ sw) << 4);

  // the bounds of this lane's four queries, and whether they exist
  float tau_t[4];
  uint32_t q_t[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    q_t[t] = qt * 128u + (uint32_t)(wq * 64 + t * 16 + fi);
    tau_t[t] = a.tau[q_t[t]];
  }

  f32x4_h acc[4][4];
#pragma unroll
  for (int rf = 0; rf < 4; rf++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[rf][t] = f32x4_h{0.f, 0.f, 0.f, 0.f};

  VDB_HSEL_GLOAD();
  VDB_HSEL_LSTORE(0u);
  __syncthreads();
  uint32_t kt = 0, rt = blockIdx.x;
  for (uint32_t it = 0; it < total; it++) {
    const bool more = it + 1 < total;
    const uint32_t buf = it & 1u;
    if (more) VDB_HSEL_GLOAD();
    const bool last_k = kt + 1 == a.KT;
    float4 nv[4];
    if (last_k) {  // (block-uniform) the row tile's norms for the epilogue, requested in front of the step's multiplies
      const float* np = a.norms + (size_t)rt * 128 + wr * 64 + 4 * kk;
#pragma unroll
      for (int rf = 0; rf < 4; rf++) nv[rf] = *reinterpret_cast<const float4*>(np + rf * 16);
    }
    const unsigned char* sb = smem + buf * 32768u;
#pragma unroll
    for (int m = 0; m < 2; m++) {
      u32x4_h av[4], bv[4];
      const uint32_t so = m ? rd_s1 : rd_s0;
#pragma unroll
      for (int rf = 0; rf < 4; rf++) av[rf] = *reinterpret_cast<const u32x4_h*>(sb + rd_a + rf * 2048 + so);
#pragma unroll
      for (int t = 0; t < 4; t++) bv[t] = *reinterpret_cast<const u32x4_h*>(sb + rd_b + t * 2048 + so);
#pragma unroll
      for (int rf = 0; rf < 4; rf++)
#pragma unroll
        for (int t = 0; t < 4; t++)
          acc[rf][t] = F16 ? __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_h, av[rf]), __builtin_bit_cast(f16x8_h, bv[t]), acc[rf][t], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_h, av[rf]), __builtin_bit_cast(bf16x8_h, bv[t]), acc[rf][t], 0, 0, 0);
    }
    if (more) VDB_HSEL_LSTORE(buf ^ 1u);  // (every wave left that buffer at the barrier of the step before)
    if (last_k) {
      // epilogue: one bit per accumulator element that survives — e = 16 rf + 4 t + r
      const uint32_t row0 = rt * 128u + (uint32_t)(wr * 64 + 4 * kk);
      uint64_t pm = 0ull;
#pragma unroll
      for (int rf = 0; rf < 4; rf++) {
        const float nr[4] = {nv[rf].x, nv[rf].y, nv[rf].z, nv[rf].w};
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const bool finite = nr[r] < __uint_as_float(0x7F800000u);  // (false for NaN)
          const float h = 0.5f * nr[r] * nr[r] * a.hk;
          const bool row_ok = row0 + (uint32_t)(rf * 16 + r) < a.n_rows;
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const float s = acc[rf][t][r] - h;
            const bool keep = row_ok && (!(s < tau_t[t]) || !finite);  // a NaN score is kept, never dropped by a false comparison
            pm |= (uint64_t)keep << (rf * 16 + t * 4 + r);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) acc[rf][t] = f32x4_h{0.f, 0.f, 0.f, 0.f};
      }
      if (__ballot(pm != 0ull)) {  // (wave-uniform; survivors are a fraction of a percent of the pairs)
        while (pm) {
          const int e = __ffsll((long long)pm) - 1;
          pm &= pm - 1;
          const uint32_t row = row0 + (uint32_t)((e >> 4) * 16 + (e & 3));
          const int t = (e >> 2) & 3;
          const uint32_t q = t == 0 ? q_t[0] : (t == 1 ? q_t[1] : (t == 2 ? q_t[2] : q_t[3]));
          if (q < a.nq && (!a.alive || a.alive[row] != 0)) {
            const uint32_t pos = atomicAdd(a.cnt + q, 1u);
            if (pos < a.cap) a.lists[(size_t)q * a.cap + pos] = row;  // (past the capacity: the counter marks the query, the rows are not needed)
          }
        }
      }
      kt = 0;
      rt += G;
    } else {
      kt++;
    }
    __syncthreads();
  }
#undef VDB_HSEL_GLOAD
#undef VDB_HSEL_LSTORE
}

// ---- re-score: one block per query, a wave per listed row (four rows in flight), the k best by (distance bits, row) -------------------
struct HalfRescoreArgs {
  const uint16_t* rows;
  const float* queries;
  const uint32_t* lists;
  const uint32_t* cnt;
  uint32_t* flags;
  uint32_t* qcount;   // the fallback's list (sweep_split.hip list_unproven's layout)
  uint32_t* qmap;
  uint32_t* qslot;
  float* qgath;       // [nq][row_stride] f32 queries of the listed ones, in list order
  const uint64_t* ext_ids;
  uint64_t* out_ids;
  float* out_scores;
  uint32_t* out_n;
  uint64_t row_stride, q_stride;
  uint32_t cap, k, dim;
};
template <bool F16>
__global__ __launch_bounds__(256) void half_l2_rescore(HalfRescoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t stride = (uint32_t)a.row_stride, k = a.k, q = blockIdx.x;
  float* qs = reinterpret_cast<float*>(smem);                                          // [row_stride]
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(smem + (size_t)stride * 4);                // [4][k]
  lds_vu32* wcnt = (lds_vu32*)(lds_void_p)(smem + (size_t)stride * 4 + (size_t)4 * k * 8);  // [4] counts | [1] the fallback slot
  const int lane = lane_id();
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t c = a.cnt[q];
  if (a.flags[q] != 0u || c > a.cap) {  // (block-uniform) the fallback: the query lists itself and leaves its f32 row behind
    if (threadIdx.x == 0) {
      const uint32_t j = atomicAdd(a.qcount, 1u);
      a.qmap[j] = q;
      a.qslot[q] = j;
      a.flags[q] = 1u;
      wcnt[4] = j;
    }
    __syncthreads();
    const uint32_t j = wcnt[4];
    for (uint32_t e = threadIdx.x; e < stride; e += 256) a.qgath[(size_t)j * stride + e] = e < a.dim ? a.queries[(size_t)q * a.q_stride + e] : 0.0f;
    return;
  }
  for (uint32_t e = threadIdx.x; e < stride; e += 256) qs[e] = e < a.dim ? half_round<F16>(a.queries[(size_t)q * a.q_stride + e]) : 0.0f;
  __syncthreads();
  lds_vu64* mine = lists + (size_t)wib * k;
  uint32_t n_mine = 0;
  const uint32_t* list = a.lists + (size_t)q * a.cap;
  const uint32_t d8 = stride / 8;
  for (uint32_t g = (uint32_t)wib * 4u; g < c; g += 16u) {
    uint32_t row[4];
    const uint16_t* rp[4];
    float acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      row[i] = list[min(g + (uint32_t)i, c - 1u)];  // past the end: the last row again, not offered
      rp[i] = a.rows + (size_t)row[i] * a.row_stride;
      acc[i] = 0.0f;
    }
    for (uint32_t cc = (uint32_t)lane; cc < d8; cc += 64) {
      uint4 v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = *reinterpret_cast<const uint4*>(rp[i] + (size_t)cc * 8);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float4 x0, x1;
        unpack8<F16>(v[i], x0, x1);
        acc[i] = half_l2_chunk(acc[i], qs + (size_t)cc * 8, x0, x1);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float score = finish_score<kEuclidean>(butterfly_all(acc[i]), 0.0f, 0.0f);
      if (g + (uint32_t)i < c) wave_list_insert(mine, n_mine, k, make_key<false>(score, row[i]), lane);  // (uniform key and branch)
    }
  }
  if (lane == 0) wcnt[wib] = n_mine;
  __syncthreads();
  if (wib != 0) return;
  for (int w = 1; w < 4; w++) {  // (as merge_topk: the other waves' sorted lists into wave 0's)
    lds_vu64* src = lists + (size_t)w * k;
    const uint32_t cs = wcnt[w];
    for (uint32_t e = 0; e < cs; e++) {
      const uint64_t kk = src[e];
      if (n_mine == k && kk >= mine[k - 1]) break;
      wave_list_insert(mine, n_mine, k, kk, lane);
    }
  }
  for (uint32_t e = (uint32_t)lane; e < k; e += 64) {  // the merge's output format
    if (e < n_mine) {
      const uint64_t key = mine[e];
      a.out_ids[(size_t)q * k + e] = a.ext_ids[key_row(key)];
      a.out_scores[(size_t)q * k + e] = key_score<false>(key);
    } else {
      a.out_ids[(size_t)q * k + e] = ~0ull;
      a.out_scores[(size_t)q * k + e] = __uint_as_float(0x7FC00000u);
    }
  }
  if (lane == 0) a.out_n[q] = n_mine;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
size_t half_l2_select_scratch_words(uint32_t nq) { return (size_t)(nq + 127u) / 128u * 128u; }

hipError_t launch_half_l2_select_batch(const HalfL2SelectBatch& b, hipStream_t st) {
  const uint32_t nqp = (uint32_t)half_l2_select_scratch_words(b.nq);
  if (b.dim % 64 != 0 || b.dim < 128 || b.row_stride != b.dim || b.nq == 0 || b.k == 0 || b.k > kHalfL2MaxK || b.n_rows == 0)
    return hipErrorInvalidValue;
  // (1) bounds, query image, cleared counters
  HalfTauArgs ta{b.rows, b.queries, b.seed_rows, b.seed_n, b.ctl + 1, b.q16, b.tau, b.cnt, b.flags, b.row_stride, b.q_stride, b.nq, b.k, b.dim};
  const size_t lds_t = (size_t)b.row_stride * 4;
  if (b.f16) hipLaunchKernelGGL(half_l2_tau_kernel<true>, dim3(nqp), dim3(64), lds_t, st, ta);
  else hipLaunchKernelGGL(half_l2_tau_kernel<false>, dim3(nqp), dim3(64), lds_t, st, ta);
  // (2) selection: the row groups of a query tile share the chip with the other tiles'
  const uint32_t nqt = nqp / 128u, ntiles = (b.n_rows + 127u) / 128u;
  const uint32_t G = std::max<uint32_t>(1u, std::min<uint32_t>(ntiles, (uint32_t)(2 * b.n_cus) / nqt));
  HalfSelArgs sa{b.rows, b.norms, b.alive, b.q16, b.tau, b.cnt, b.lists, b.row_stride, kHalfL2ListCap, b.n_rows, b.nq, b.dim / 64u,
                  (float)(1.0 - 16.0 * (double)b.dim * 5.9604644775390625e-8 * 1.000001)};
  if (b.f16) hipLaunchKernelGGL(half_l2_select<true>, dim3(G, nqt), dim3(256), 65536, st, sa);
  else hipLaunchKernelGGL(half_l2_select<false>, dim3(G, nqt), dim3(256), 65536, st, sa);
  // (3) re-score
  HalfRescoreArgs ra{b.rows, b.queries, b.lists, b.cnt, b.flags, b.ctl + 1, b.qmap, b.qslot, b.qgath, b.ext_ids, b.out_ids, b.out_scores, b.out_n,
                     b.row_stride, b.q_stride, kHalfL2ListCap, b.k, b.dim};
  const size_t lds_r = (size_t)b.row_stride * 4 + (size_t)4 * b.k * 8 + 32;
  if (b.f16) hipLaunchKernelGGL(half_l2_rescore<true>, dim3(b.nq), dim3(256), lds_r, st, ra);
  else hipLaunchKernelGGL(half_l2_rescore<false>, dim3(b.nq), dim3(256), lds_r, st, ra);
  return hipGetLastError();
}

}  // namespace vdb
