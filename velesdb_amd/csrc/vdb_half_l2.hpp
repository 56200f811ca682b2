// vdb_half_l2.hpp — what the streaming Euclidean sweep over a half image (sweep_half_l2.hip) and its matrix-core selection path
// (sweep_half_l2_select.hip) share: the conversions, the declared lane chain of one 16-byte chunk, and — host and device, nothing of
// HIP in it, so that tests/half_l2_bound_model.cpp can run it on the CPU — the error bound of a selection score.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_HD __host__ __device__
#else
#define VDB_HD
#endif

namespace vdb {

constexpr uint32_t kHalfL2SeedRows = 4096;   // rows of the seed prefix (= kSplitSeedRows, vdb_kernels.hpp)
constexpr uint32_t kHalfL2ListCap = 16384;   // survivor rows a query's list holds; a query that passes it takes the fallback
constexpr uint32_t kHalfL2MaxK = 128;
// smallest batch, measured (tools/half_probe.py --l2-ab): at k = 10 sixteen queries are 1.34 x - 1.53 x ahead of the streaming
// kernel; at k = 100 sixteen are level with it (the seed's k-lists cost what the streaming pass's do) and 64 are 3.1 x ahead
constexpr uint32_t kHalfL2MinQueries = 16;
constexpr uint32_t kHalfL2MinQueriesBigK = 64;  // k > kHalfL2SmallK
constexpr uint32_t kHalfL2SmallK = 10;

// The selection score of row v for query q (both rounded to the half format, exact in f32) is s = q.v - |v|^2 / 2, so that
// |q - v|^2 = |q|^2 - 2 s.  The kernel's s differs from (|q|^2 - chain) / 2 — `chain` the declared f32 chain sum the streaming kernel
// reports the root of — by no more than delta, WHATEVER the order the matrix instruction adds in (u = 2^-24; products of two half
// values are exact in f32, so only additions round):
//   q.v accumulated over dim terms in any order:  <= dim u sum |q_i v_i| <= dim u (|q|^2 + |v|^2) / 2
//   |v|^2 / 2 from the stored f32 norm of the rounded row (dim additions, a root, a square, a halving): <= (dim + 4) u |v|^2 / 2
//   the subtraction:                               <= u (|q|^2 / 2 + |v|^2)
//   the chain against the real |q - v|^2 (dim additions, a rounded difference and its square per term):
//                                                  <= (dim + 3) u |q - v|^2 <= 2 (dim + 3) u (|q|^2 + |v|^2), halved
//   together <= (2 dim + 7) u (|q|^2 + |v|^2) for dim >= 2: the factor 8 dim of sweep_split.hip l2_rerank_verify's `slack` covers it
//   nearly four times over, and its 1e-6 E_k term is kept as well.
// qn2 = |q|^2, vn2 = the ROW's |v|^2, dk = the chain sum of the k-th best seed row.  The kernels split it: the query's share
// (vn2 = 0) lowers tau_q, the row's share 8 dim u |v|^2 raises the row's score in the selection epilogue (s = q.v - (1 - 16 dim u) |v|^2 / 2),
// so one row of huge norm loosens nobody's bound but its own.
VDB_HD static inline double half_l2_delta(uint32_t dim, double qn2, double vn2, double dk) {
  return 8.0 * (double)dim * 5.9604644775390625e-8 * (qn2 + vn2) + 1e-6 * dk;
}
// The bound a row's score is compared with: every row whose chain sum is <= dk has s >= tau.  Rounded DOWN to f32 (the relative
// 2^-22 is four times the rounding of the conversion), so the exclusion is strict: a row left out has a chain sum > dk.
VDB_HD static inline float half_l2_tau(uint32_t dim, double qn2, double vn2, double dk) {
  const double t = 0.5 * (qn2 - dk) - half_l2_delta(dim, qn2, vn2, dk);
  return (float)(t - (t < 0 ? -t : t) * 2.384185791015625e-7 - 1e-37);
}
// the list capacity covers the expected survivors n k / R0 twice
VDB_HD static inline bool half_l2_lists_fit(uint64_t n_rows, uint32_t k) {
  return n_rows * (uint64_t)k * 2u <= (uint64_t)kHalfL2ListCap * kHalfL2SeedRows;
}

}  // namespace vdb

#ifdef __HIPCC__
#include "vdb_device.hpp"

namespace vdb {

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
// the eight values of one 16-byte chunk of a half row
template <bool F16>
__device__ __forceinline__ void unpack8(const uint4& v, float4& x0, float4& x1) {
  float x[8];
  unpack2<F16>(v.x, x[0], x[1]);
  unpack2<F16>(v.y, x[2], x[3]);
  unpack2<F16>(v.z, x[4], x[5]);
  unpack2<F16>(v.w, x[6], x[7]);
  x0 = make_float4(x[0], x[1], x[2], x[3]);
  x1 = make_float4(x[4], x[5], x[6], x[7]);
}
// THE DECLARED LANE CHAIN (sweep_half_l2.hip), one chunk: the lane's sum advanced over the chunk's eight elements in increasing order;
// qp: the rounded query's eight values of the same chunk, f32, 16-byte aligned (LDS)
__device__ __forceinline__ float half_l2_chunk(float s, const float* qp, const float4& x0, const float4& x1) {
  s = chain4<kOpL2>(s, ld4(qp), x0);
  return chain4<kOpL2>(s, ld4(qp + 4), x1);
}

}  // namespace vdb
#endif
