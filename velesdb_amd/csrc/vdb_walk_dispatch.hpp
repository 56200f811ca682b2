// vdb_walk_dispatch.hpp — the run-time (metric, chunks-per-lane) pair of a graph-walk launch as compile-time constants: the one
// metric x CPL ladder of the walk, insert and neighbour-distance families (hnsw_kernels.hip, hnsw_half.hip, hnsw_int8.hip,
// hnsw_filtered.hip, hnsw_build.hip).  Plain C++17, no HIP header: tests/walk_dispatch_model.cpp compiles it with a host compiler.
#pragma once
#include <type_traits>

#include "../../include/velesdb_hip.h"

namespace vdb {

// Hamming and Jaccard (the packed-bit metrics; generic kernels only: CPL 0) in a kernel family:
//   kTaken      the family has them; any metric that is none of the other four is Jaccard
//   kFallToDot  it does not, and any metric but Cosine / Euclidean is DotProduct (the half and int8 walks, the half build, the
//               latency-mode walk: such a metric is refused, or routed elsewhere, in front of the call)
//   kRefused    it does not, and the launch answers `refused` (the filtered families: hipErrorInvalidValue)
enum class BitMetrics { kTaken, kFallToDot, kRefused };

template <int V>
using int_c = std::integral_constant<int, V>;

// f(std::bool_constant<b>)
template <class F>
auto dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(int_c<CPL>): CPL = chunks of 256 dimensions per lane, 1..4; 0 = the generic kernel (sweep_cpl_for_dim)
template <class F>
auto dispatch_cpl(int cpl, F&& f) {
  switch (cpl) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
    default: return f(int_c<0>{});
  }
}

// f(int_c<METRIC>)
template <BitMetrics BITS, class R, class F>
R dispatch_metric(int metric, R refused, F&& f) {
  switch (metric) {
    case VDB_COSINE: return f(int_c<VDB_COSINE>{});
    case VDB_EUCLIDEAN: return f(int_c<VDB_EUCLIDEAN>{});
    default: break;
  }
  if constexpr (BITS == BitMetrics::kFallToDot) {
    (void)refused;
    return f(int_c<VDB_DOT>{});
  } else {
    if (metric == VDB_DOT) return f(int_c<VDB_DOT>{});
    if constexpr (BITS == BitMetrics::kTaken) {
      (void)refused;
      if (metric == VDB_HAMMING) return f(int_c<VDB_HAMMING>{});
      return f(int_c<VDB_JACCARD>{});
    } else {
      return refused;
    }
  }
}

// f(int_c<METRIC>, int_c<CPL>), once: kernel<M(), C()> at the call site.  Hamming and Jaccard arrive with CPL 0 whatever `cpl` says.
template <BitMetrics BITS, class R, class F>
R dispatch_metric_cpl(int metric, int cpl, R refused, F&& f) {
  return dispatch_metric<BITS, R>(metric, refused, [&](auto M) -> R {
    if constexpr (M() == VDB_HAMMING || M() == VDB_JACCARD)
      return f(M, int_c<0>{});
    else
      return dispatch_cpl(cpl, [&](auto C) -> R { return f(M, C); });
  });
}

}  // namespace vdb
