// vdb_filter_route.hpp — which route a filtered exact call takes (vdb_hip_index_search_batch_filtered).
// Pure host logic without a HIP header: tests/filter_route_model.cpp compiles it alone and walks its boundaries.
#pragma once
#include <stdint.h>

namespace vdb {

enum FilterRoute : int { kFilterRouteDense = 0, kFilterRouteListed = 1 };

// VDB_OPT_FILTER_ROUTE: <= 0 auto, 1 the listed sweep wherever it exists, 2 mask substitution.
// `listed_available`: the metric has a listed kernel (Cosine / DotProduct / Euclidean) and its k-lists fit the LDS.
// Auto is a STATED GUESS, not a measurement: listed iff count <= n_rows / 4 and count * nq <= 8 * n_rows.  The exact path takes a
// flat 0.44-0.53 ms for 16-256 queries at 1 M x 768 whatever the mask; the listed kernel reads count rows once per pass of <= 16
// (mode M) or <= 8 (mode C) queries and was assumed to reach ~40 TFLOP/s of f32 — nobody has measured either on this route.
static inline int filter_route(int64_t opt, bool listed_available, uint64_t count, uint64_t n_rows, uint32_t nq) {
  if (!listed_available || count == 0) return kFilterRouteDense;
  if (opt == 1) return kFilterRouteListed;
  if (opt >= 2) return kFilterRouteDense;
  return (count <= n_rows / 4 && count * (uint64_t)nq <= 8 * n_rows) ? kFilterRouteListed : kFilterRouteDense;
}

// Mask substitution: does the call keep the selection stage (levels 1-3, WIDE)?  The stage seeds its bounds from a sample of the
// first rows and parks the handle after batches it cannot prove; both assume that almost every row is a candidate.  With fewer
// than 1/16 of the rows allowed the seed sample holds too few live rows to give k keys a bound (16 384 sample rows, one key per 64
// rows: 256 keys, 16 of them live at 1/16), so those calls go straight to the exact kernels — which serve any mask.
static inline bool filter_keeps_selection(uint64_t count, uint64_t n_rows) { return count * 16 >= n_rows; }

}  // namespace vdb
