// vdb_lds_sort.hpp — the block-wide building blocks fusion.hip's fuse_lists_kernel and hybrid.hip's hybrid_fuse_kernel share: a
// bitonic network over records in LDS and a prefix sum over the block's threads.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vdb {

// smallest power of two >= n (n >= 1)
__device__ __forceinline__ uint32_t lds_pow2(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// ascending bitonic sort of recs[0, P) under `less`, P a power of two; every thread of the block calls it (nt threads), the caller
// has a barrier between its last write of recs and the call; a barrier ends it
template <class R, class Less>
__device__ __forceinline__ void lds_bitonic(R* __restrict__ recs, uint32_t P, uint32_t tid, uint32_t nt, Less less) {
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t p = tid; p < (P >> 1); p += nt) {
        const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));  // i < P - j, partner i | j < P
        const uint32_t l = i | j;
        const R a = recs[i], b = recs[l];
        const bool swap = (i & k) == 0 ? less(b, a) : less(a, b);
        if (swap) {
          recs[i] = b;
          recs[l] = a;
        }
      }
      __syncthreads();
    }
  }
}

// inclusive prefix sum of v over the block's threads in scan[0, nt) (LDS): afterwards scan[tid] = v of threads 0..tid, scan[nt - 1] =
// the block's sum.  Every thread calls it; nobody may still be reading scan from an earlier use (the caller's barrier)
__device__ __forceinline__ void lds_scan(uint32_t* __restrict__ scan, uint32_t v, uint32_t tid, uint32_t nt) {
  scan[tid] = v;
  __syncthreads();
  for (uint32_t off = 1; off < nt; off <<= 1) {
    const uint32_t u = tid >= off ? scan[tid - off] : 0u;
    __syncthreads();
    scan[tid] += u;
    __syncthreads();
  }
}

}  // namespace vdb
