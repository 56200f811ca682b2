// vdb_filter_route.hpp — which route a filtered exact call takes (vdb_hip_index_search_batch_filtered) and which a
// filtered graph call takes (vdb_hip_index_search_graph_filtered), and which queries of a call with one filter per
// query share a launch (vdb_hip_index_search_graph_filters) — the one-filter call is planned here too: it is a call
// of the second kind with every query on the same filter.
// Pure host logic without a HIP header: tests/filter_route_model.cpp, tests/filter_graph_route_model.cpp and
// tests/filters_plan_model.cpp compile it alone and walk its boundaries.
#pragma once
#include <stdint.h>

#include <vector>

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

// ---- filtered graph search (vdb_hip_index_search_graph_filtered): walk or exact pass, and the walk's first list ----
enum FilterGraphRoute : int { kFgRefuse = -1, kFgAuto = 0, kFgWalk = 1, kFgExact = 2 };
struct FilterGraphPlan {
  int route;      // kFgWalk, kFgExact, or kFgRefuse (route = walk and not even the smallest list fits cap_max)
  uint32_t cap;   // kFgWalk: the capacity of the first attempt (entries)
};
static inline uint64_t fg_round64(uint64_t v) { return (v + 63) / 64 * 64; }
// the list of the unfiltered walk (hnsw_search_prepare): ef results + room for candidates that tie with the furthest one
static inline uint64_t fg_min_list(uint32_t ef_eff) {
  return fg_round64((uint64_t)ef_eff + (ef_eff / 2 > 64 ? (uint64_t)ef_eff / 2 : 64));
}
// the density-sized list: while fewer than ef allowed nodes are known the walk admits everything, about ef * n_rows / matched
// nodes; twice that plus one chunk.  ~0 when it cannot fit any list (ef_eff > cap_max: the product below then stays far inside 64 bits)
static inline uint64_t fg_sized_list(uint32_t ef_eff, uint64_t matched, uint64_t n_rows, uint32_t cap_max) {
  if (matched == 0 || ef_eff > cap_max) return ~0ull;
  const uint64_t s = fg_round64(2ull * ef_eff * n_rows / matched + 64);
  const uint64_t m = fg_min_list(ef_eff);
  return s > m ? s : m;
}
// route: the caller's (0 auto, 1 walk, 2 exact pass); ef_eff = max(ef, k) after the Balanced rule; matched = rows in the filter;
// cap_max = the largest list the launch can hold (160 KB of LDS at its nbmax, lowered by the caller's max_list).
// Auto is a STATED GUESS, not a measurement — the factor 2 and the `matched < ef_eff` cut: tools/filter_probe.py's graph leg is
// what would settle them.
static inline FilterGraphPlan filter_graph_route(int route, uint32_t ef_eff, uint64_t matched, uint64_t n_rows, uint32_t cap_max) {
  if (route == kFgExact || matched == 0) return FilterGraphPlan{kFgExact, 0};
  const uint64_t sized = fg_sized_list(ef_eff, matched, n_rows, cap_max);
  if (route == kFgWalk) {
    if (fg_min_list(ef_eff) > cap_max) return FilterGraphPlan{kFgRefuse, 0};
    return FilterGraphPlan{kFgWalk, (uint32_t)(sized < cap_max ? sized : cap_max)};
  }
  if (matched < ef_eff) return FilterGraphPlan{kFgExact, 0};  // the walk could never fill its result set
  if (sized > cap_max) return FilterGraphPlan{kFgExact, 0};
  return FilterGraphPlan{kFgWalk, (uint32_t)sized};
}

// ---- one filter per query (vdb_hip_index_search_graph_filters): which queries share a launch ----
// Every query keeps the plan filter_graph_route gives ITS filter and climbs ITS OWN ladder — first list plan.cap, four times the
// room while it overflows, cap_max last, then the exact pass.  When every query has the same plan a round is one launch at that
// capacity: the loop the one-filter call ran while it had one of its own (tests/filters_plan_model.cpp keeps a transcription and
// holds filters_walk_ladders to it).  Only the grouping into launches looks at the other queries, and a launch changes nothing a query computes: the kernel sizes the LDS layout by the
// launch's PHYSICAL capacity and runs all list logic of a query on its own LOGICAL one.
struct FiltersSlot {   // one launch slot (device layout, 16 bytes)
  uint32_t query, filter, cap, pad;  // cap: the query's logical list capacity in this attempt
};
struct FiltersLaunch {
  uint32_t begin, count;  // slots [begin, begin + count) of the round's grouped slot array
  uint32_t cap;           // physical capacity: the largest logical one of the group
  uint32_t per_cu;        // walks a CU holds at that footprint (1..4)
};
constexpr uint64_t kFgLdsBudget = 160 * 1024;
// walks per CU at an LDS footprint: hnsw_search_prepare's rule
static inline uint32_t fg_per_cu(uint64_t lds) {
  const uint64_t n = lds ? kFgLdsBudget / lds : 4;
  return (uint32_t)(n > 4 ? 4 : (n < 1 ? 1 : n));
}
// the next step of a query's ladder after an overflow at `cap`; 0 = the ladder is over (the exact pass, or the refusal of route 1)
static inline uint32_t fg_ladder_next(uint32_t cap, uint32_t cap_max) {
  if (cap >= cap_max) return 0;
  const uint64_t n = (uint64_t)cap * 4;
  return (uint32_t)(n < cap_max ? n : cap_max);
}
// One round (the first attempts, or the re-runs): `in[n]` grouped into at most four launches by fg_per_cu(lds_of(cap)), fullest CUs
// first, the order of `in` kept inside a group.  out[n] receives the grouped slots; returns the number of launches.
template <class LdsOf>
static inline uint32_t filters_plan_round(const FiltersSlot* in, uint32_t n, FiltersSlot* out, FiltersLaunch launches[4], LdsOf&& lds_of) {
  uint32_t n_launch = 0, at = 0;
  for (uint32_t pc = 4; pc >= 1; pc--) {
    FiltersLaunch l{at, 0, 0, pc};
    for (uint32_t i = 0; i < n; i++) {
      if (fg_per_cu(lds_of(in[i].cap)) != pc) continue;
      out[at++] = in[i];
      l.count++;
      if (in[i].cap > l.cap) l.cap = in[i].cap;
    }
    if (l.count) launches[n_launch++] = l;
  }
  return n_launch;
}
// The ladders of a call.  `round` = the first attempts (cap = the query's plan.cap).  run(slots, n, launches, n_launches, over)
// runs one round and sets over[i] != 0 for every slot whose list overflowed; a non-zero return ends the call with that value.
// Queries whose ladder is over land in *leftover with the capacity of their last attempt.
template <class LdsOf, class Run>
static inline int filters_walk_ladders(std::vector<FiltersSlot> round, uint32_t cap_max, LdsOf&& lds_of, Run&& run,
                                       std::vector<FiltersSlot>* leftover) {
  std::vector<FiltersSlot> grouped, next;
  std::vector<unsigned char> over;
  while (!round.empty()) {
    const uint32_t n = (uint32_t)round.size();
    FiltersLaunch launches[4];
    grouped.resize(n);
    const uint32_t nl = filters_plan_round(round.data(), n, grouped.data(), launches, lds_of);
    over.assign(n, 0);
    const int rc = run((const FiltersSlot*)grouped.data(), n, (const FiltersLaunch*)launches, nl, over.data());
    if (rc != 0) return rc;
    next.clear();
    for (uint32_t i = 0; i < n; i++) {
      if (!over[i]) continue;
      FiltersSlot s = grouped[i];
      const uint32_t nc = fg_ladder_next(s.cap, cap_max);
      if (nc) {
        s.cap = nc;
        next.push_back(s);
      } else {
        leftover->push_back(s);
      }
    }
    round.swap(next);
  }
  return 0;
}

}  // namespace vdb
