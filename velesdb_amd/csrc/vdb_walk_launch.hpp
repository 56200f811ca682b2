// vdb_walk_launch.hpp — how the graph kernels are launched: the metric x chunks-per-lane dispatch (vdb_walk_dispatch.hpp) on the
// launch's own (metric, dim), and the two launch forms every walk, insert and exact-pass kernel takes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vdb_device.hpp"
#include "vdb_kernels.hpp"
#include "vdb_walk_dispatch.hpp"

namespace vdb {

static_assert((int)kCosine == (int)VDB_COSINE && (int)kEuclidean == (int)VDB_EUCLIDEAN && (int)kDot == (int)VDB_DOT &&
                  (int)kHamming == (int)VDB_HAMMING && (int)kJaccard == (int)VDB_JACCARD,
              "vdb_walk_dispatch.hpp names the metrics by the C ABI's constants");

// f(int_c<METRIC>, int_c<CPL>) for a launch over `dim` dimensions; f(int_c<METRIC>) for the families that only have the generic kernel
template <BitMetrics BITS, class F>
hipError_t walk_dispatch(int metric, uint32_t dim, F&& f) {
  return dispatch_metric_cpl<BITS, hipError_t>(metric, sweep_cpl_for_dim(dim), hipErrorInvalidValue, f);
}
template <BitMetrics BITS, class F>
hipError_t walk_dispatch_metric(int metric, F&& f) {
  return dispatch_metric<BITS, hipError_t>(metric, hipErrorInvalidValue, f);
}

// One launch of persistent walk blocks: at most `slots` of them, and no more than are resident per CU of THIS instantiation
// (registers / LDS; capped at max_per_cu) — a larger grid would queue whole blocks behind the persistent ones, and the walk's visited
// bitmaps are sized for `slots` blocks.
template <class KERN, class ARGS>
hipError_t launch_walk_blocks(KERN kern, const ARGS& args, uint32_t n_cus, int slots, size_t lds, hipStream_t st, int block = 256,
                              int max_per_cu = 4) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  int occ = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, block, lds);
  if (e != hipSuccess) return e;
  occ = std::max(1, std::min(occ, max_per_cu));
  const int grid = (int)std::min<int64_t>((int64_t)slots, (int64_t)n_cus * occ);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, args);
  return hipGetLastError();
}

// ... of the grid as given (the latency-mode walk: one block per query; the insert kernels: one per node of the batch)
template <class KERN, class ARGS>
hipError_t launch_walk_grid(KERN kern, const ARGS& args, int grid, size_t lds, hipStream_t st, int block = 256) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, args);
  return hipGetLastError();
}

}  // namespace vdb
