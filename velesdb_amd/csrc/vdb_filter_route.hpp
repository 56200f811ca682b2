// vdb_filter_route.hpp — which route a filtered exact call takes (vdb_hip_index_search_batch_filtered) and which a
// filtered graph call takes (vdb_hip_index_search_graph_filtered), and which queries of a call with one filter per
// query share a launch (vdb_hip_index_search_graph_filters) — the one-filter call is planned here too: it is a call
// of the second kind with every query on the same filter — and how an EXACT call with one filter per query groups its queries and
// cuts its listed groups into the work items of the grouped launches (vdb_hip_index_search_batch_filters), and the route
// and the listed passes of a filtered exact call over the SQ8 / Binary / half images (vdb_hip_index_search_batch_filtered_mode),
// and the groups and grouped launches of such a call with one filter per query (vdb_hip_index_search_batch_filters_mode),
// and the two phases of a fused search with one filter per query (vdb_hip_index_hybrid_search_filters /
// vdb_hip_index_multi_query_search_filters).
// Pure host logic without a HIP header: tests/filter_route_model.cpp, tests/filter_mode_route_model.cpp,
// tests/filter_graph_route_model.cpp, tests/filters_plan_model.cpp, tests/listed_groups_plan_model.cpp,
// tests/mode_groups_plan_model.cpp and tests/hybrid_filters_plan_model.cpp compile it alone and walk its boundaries.
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

// ---- filtered exact search over the SQ8 / Binary / half row images (vdb_hip_index_search_batch_filtered_mode) ----
// (the values of enum vdb_search_mode / vdb_metric this header needs; index.hip holds them to include/velesdb_hip.h)
constexpr int kFmModeBf16 = 3, kFmModeSq8 = 5, kFmModeBinary = 6, kFmModeF16 = 7;
constexpr int kFmMetricEuclidean = 1;
constexpr uint32_t kFmSq8ListedMaxQueries = 3;  // SQ8: the largest batch auto gives to the listed kernel (one-query passes only, below)
// which of the four modes has a listed kernel for this metric at all: SQ8 (Cosine / Euclidean / DotProduct: the caller checks the
// metric is one of the three), Euclidean over a half image.  Binary and Cosine / DotProduct over a half image run on mask substitution.
static inline bool filter_mode_has_listed(int mode, int metric) {
  if (mode == kFmModeSq8) return true;
  if (mode == kFmModeBf16 || mode == kFmModeF16) return metric == kFmMetricEuclidean;
  return false;
}
// The route of a filtered call in one of those modes.  Forced values behave as in filter_route; `listed_available`: the mode and
// metric have a listed kernel (above) AND its plan fits the LDS (mode_listed_plan below).
// Auto started as a stated guess and was then held against ONE measurement (100 K x 768, k = 10, 1 / 16 / 1 024 queries, densities
// 0.01 - 1.0); what it is now:
//   * Euclidean over a half image: the listed kernel does per listed row what the full sweep does per row, plus a gathered instead of
//     a streamed read — listed iff count <= 3/4 n_rows.  Measured: listed ahead at 0.01 / 0.1 / 0.5 at all three batch sizes (0.24 -
//     0.84 of the unfiltered call), 2 % behind at 1.0.
//   * SQ8, all three metrics: listed iff the batch runs as one-query passes (nq <= kFmSq8ListedMaxQueries) and count <= 3/4 n_rows.
//     Measured: at one query listed is ahead at 0.01 - 0.5 (0.65 - 0.77 of the unfiltered call); at 16 and 1 024 queries an 8-query
//     listed pass costs ~0.23 ms whatever the list's length — more than a full 8-query pass over 100 K rows (0.16 ms) — and from six
//     queries up mask substitution keeps the selection stage (Euclidean too: select_level_sq8), so mask substitution wins at every
//     density.  The first guess (Euclidean: 3/4 at every batch size; Cosine / DotProduct: the f32 rule from six queries up) was wrong
//     there.  NOT measured: batches of 2 - 15 queries (the 4-query pass), other corpus sizes; the fixed cost of the 4- and 8-query
//     listed passes is not explained.
static inline int filter_mode_route(int64_t opt, int mode, int metric, uint64_t count, uint64_t n_rows, uint32_t nq, bool listed_available) {
  if (!listed_available || count == 0 || !filter_mode_has_listed(mode, metric)) return kFilterRouteDense;
  if (opt == 1) return kFilterRouteListed;
  if (opt >= 2) return kFilterRouteDense;
  if (mode == kFmModeSq8 && nq > kFmSq8ListedMaxQueries) return kFilterRouteDense;
  return count * 4 <= n_rows * 3 ? kFilterRouteListed : kFilterRouteDense;
}

// LDS footprints of the two streaming kernels (storage_modes.hip sweep_topk_sq8 / sweep_half_l2.hip sweep_topk_half_l2 and their listed
// forms: the same layouts).  SQ8: queries [dpad][B] f32 | 4 staging tiles of 64 rows x 80 B | lists [B][k] | cnt, lock, qsum, qnsq [B]
static inline uint64_t fm_sq8_lds_bytes(int B, uint32_t k, uint32_t dim) {
  const uint64_t dpad = ((uint64_t)dim + 3u) & ~(uint64_t)3;
  return (dpad * (uint64_t)B * 4 + (uint64_t)4 * 64 * 80 + (uint64_t)B * k * 8 + (uint64_t)B * 16 + 15) & ~(uint64_t)15;
}
// half Euclidean: q[B][stride] f32 | lists[B][k] | cnt[B] | lock[B], stride = dim rounded up to 8
static inline uint64_t fm_half_l2_lds_bytes(int B, uint32_t k, uint32_t dim) {
  const uint64_t stride = ((uint64_t)dim + 7) / 8 * 8;
  return (((uint64_t)B * stride * 4 + (uint64_t)B * k * 8 + (uint64_t)B * 8) + 15) & ~(uint64_t)15;
}
// One pass of a listed sweep in these modes, next to sweep_listed_plan: the queries per pass follow the unlisted dispatch (SQ8: 8 from 8
// queries left, 4 from 4, else 1; half Euclidean: 16 above 4 left, 4 above 1, else 1; a class whose LDS does not fit gives way to the
// next), blocks take contiguous chunks of per_block row groups (a group = 64 listed rows for SQ8 — one per lane —, 64 / B for the half
// kernel), four waves a block, at most n_cus x (resident blocks per CU) blocks.  blocks == 0: the route is "not available" (count,
// k or nq zero, or not even one query fits 160 KiB).
struct ModeListedPlan {
  int blocks = 0;
  int B = 0;
  uint32_t nq_pass = 0, per_block = 0;
  uint64_t lds = 0;
};
constexpr uint64_t kFmLdsBudget = 160 * 1024;
static inline ModeListedPlan mode_listed_plan(bool half, uint32_t dim, uint32_t k, uint64_t count, uint32_t nq_left, int n_cus) {
  ModeListedPlan p;
  if (count == 0 || k == 0 || nq_left == 0 || count > 0xFFFFFFFFull) return p;
  int B = half ? (nq_left > 4 ? 16 : (nq_left > 1 ? 4 : 1)) : (nq_left >= 8 ? 8 : (nq_left >= 4 ? 4 : 1));
  auto lds_of = [&](int b) { return half ? fm_half_l2_lds_bytes(b, k, dim) : fm_sq8_lds_bytes(b, k, dim); };
  while (B > 1 && lds_of(B) > kFmLdsBudget) B = half ? B / 4 : (B == 8 ? 4 : 1);
  const uint64_t lds = lds_of(B);
  if (lds > kFmLdsBudget) return p;
  const uint64_t rpg = half ? 64u / (uint64_t)B : 64u;
  const uint64_t ngroups = (count + rpg - 1) / rpg;
  uint64_t per_cu = kFmLdsBudget / lds, cap = half ? 3 : 4;  // (the half kernel runs at 3 waves per SIMD)
  if (per_cu > cap) per_cu = cap;
  uint64_t want = (ngroups + 3) / 4;
  const uint64_t room = (uint64_t)(n_cus > 0 ? n_cus : 1) * per_cu;
  if (want > room) want = room;
  if (want < 1) want = 1;
  p.per_block = (uint32_t)((ngroups + want - 1) / want);
  p.blocks = (int)((ngroups + p.per_block - 1) / p.per_block);
  p.B = B;
  p.nq_pass = nq_left < (uint32_t)B ? nq_left : (uint32_t)B;
  p.lds = lds;
  return p;
}

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

// ---- one filter per query on the exact sweep (vdb_hip_index_search_batch_filters) ----
// Queries are grouped by filter; every group takes the route filter_route gives it with ITS count and ITS number of queries.  The
// groups on the listed route share one set of grouped launches (below); the groups on mask substitution and the unfiltered queries
// run one after another through the existing exact path.
struct FxPass {        // what sweep_listed_plan gives a group with nq_left queries still to serve
  int B;               // mode C: 8, 4 or 1 queries per wave pass; mode M: 0
  uint32_t nq_pass;    // queries of the next pass; 0 = the listed kernels cannot take the shape (k-lists / queries do not fit the LDS)
};
struct FxGroup {
  uint32_t filter;                 // index into the call's table; n_filters = the unfiltered queries
  int route;                       // kFilterRouteListed or kFilterRouteDense (mask substitution; the unfiltered queries: the plain path)
  std::vector<uint32_t> queries;   // positions in the call, ascending
};
// groups in the order their first query appears.  count_of(f) = rows of filter f; pass_of(nq_left) -> FxPass
template <class CountOf, class PassOf>
static inline std::vector<FxGroup> filters_exact_groups(const uint32_t* fq, uint32_t nq, uint32_t n_filters, int64_t opt, uint64_t n_rows,
                                                        CountOf&& count_of, PassOf&& pass_of) {
  std::vector<uint32_t> at(n_filters + 1u, ~0u);
  std::vector<FxGroup> g;
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t f = fq[i];
    if (at[f] == ~0u) {
      at[f] = (uint32_t)g.size();
      g.push_back(FxGroup{f, kFilterRouteDense, {}});
    }
    g[at[f]].queries.push_back(i);
  }
  for (FxGroup& x : g) {
    if (x.filter == n_filters) continue;
    const uint32_t nq_g = (uint32_t)x.queries.size();
    x.route = filter_route(opt, pass_of(nq_g).nq_pass > 0, count_of(x.filter), n_rows, nq_g);
  }
  return g;
}

// The grouped launches.  Every listed group is cut into PASSES of pass_of(nq_left).nq_pass queries (the loop of the one-filter
// call), every pass into CHUNKS of per_block units of its list — a unit is a row group of 64 / B rows (mode C) or a 64-row tile
// (mode M).  One chunk = one work item = one block.  Passes of one class (B) share a launch and its per_block:
//   units  = sum over the launch's passes of ceil(count / rows per unit)
//   want   = mode C: max(1, min(ceil(units / 4), n_cus * occ))     (four waves, a unit each: sweep_listed_plan's rule)
//            mode M: min(units, n_cus * occ)
//   per_block = ceil(units / want), raised until no pass has more than max_lists chunks
// so a launch has at most want + (its passes) blocks — a pass's last chunk may be short, none is empty — and a table of one
// pass is sweep_listed_plan's plan.  A query owns lists_per_query partial lists (the largest chunk count of any pass of the call);
// chunk c of a pass writes list c of each of its queries, the lists past a pass's chunk count stay invalid.
constexpr uint32_t kLgPassQueries = 16;
struct ListedGroupItem {    // device layout, 96 bytes
  const uint32_t* list;     // the chunk: where it starts in the filter's ascending rows ...
  uint32_t count;           // ... and its rows (per_block units; the last chunk of a pass may hold fewer)
  uint32_t nq;              // queries of the pass
  uint32_t slot;            // the partial list of each of its queries this block writes (the chunk's number in its pass)
  uint32_t units;           // ceil(count / rows per unit): where the block's sweep ends
  uint32_t q[kLgPassQueries];  // the pass's queries: positions in the call (unused entries 0)
  uint32_t pad2[2];
};
static_assert(sizeof(ListedGroupItem) == 96, "device layout");
struct ListedGroupsLaunch {
  int B;                    // class (mode M: 0)
  uint32_t begin, count;    // items [begin, begin + count)
  uint32_t per_block, want, passes;
  uint32_t nq_max;          // the largest pass (mode M sizes its LDS by it)
};
struct ListedGroupsPlan {
  std::vector<ListedGroupItem> items;
  ListedGroupsLaunch launches[3];
  uint32_t n_launches = 0;
  uint32_t lists_per_query = 0;
};
// list_of(f) -> const uint32_t*; count_of(f) -> rows; pass_of(f, nq_left) -> FxPass; occ_of(B, nq_max) -> resident blocks per CU;
// classes[n_classes]: the pass widths that launch, widest first (mode M: the one class 0); rpu_of(B) -> rows of a unit
template <class ListOf, class CountOf, class PassOf, class OccOf, class RpuOf>
static inline void listed_groups_plan_core(const std::vector<FxGroup>& groups, bool mode_m, const int* classes, int n_classes, int n_cus,
                                           uint32_t max_lists, ListOf&& list_of, CountOf&& count_of, PassOf&& pass_of, OccOf&& occ_of,
                                           RpuOf&& rpu_of, ListedGroupsPlan* out) {
  struct Pass {
    uint32_t group, q0, nq, units;
    int B;
  };
  std::vector<Pass> passes;
  for (uint32_t gi = 0; gi < (uint32_t)groups.size(); gi++) {
    const FxGroup& g = groups[gi];
    if (g.route != kFilterRouteListed) continue;
    const uint64_t count = count_of(g.filter);
    for (uint32_t q0 = 0, nq_g = (uint32_t)g.queries.size(); q0 < nq_g;) {
      const FxPass p = pass_of(g.filter, nq_g - q0);
      if (p.nq_pass == 0) break;  // (cannot happen for a group its grouping put on this route)
      const uint32_t rpu = rpu_of(mode_m ? 0 : p.B);
      passes.push_back(Pass{gi, q0, p.nq_pass, (uint32_t)((count + rpu - 1) / rpu), mode_m ? 0 : p.B});
      q0 += p.nq_pass;
    }
  }
  *out = ListedGroupsPlan{};
  if (max_lists == 0) max_lists = 1;
  for (int ci = 0; ci < n_classes; ci++) {
    const int B = classes[ci];
    uint64_t units = 0;
    uint32_t n_pass = 0, nq_max = 0, units_max = 0;
    for (const Pass& p : passes) {
      if (p.B != B) continue;
      units += p.units;
      n_pass++;
      if (p.nq > nq_max) nq_max = p.nq;
      if (p.units > units_max) units_max = p.units;
    }
    if (!n_pass) continue;
    const uint64_t room = (uint64_t)(n_cus > 0 ? n_cus : 1) * (uint64_t)occ_of(B, nq_max);
    uint64_t want = mode_m ? (units < room ? units : room) : ((units + 3) / 4 < room ? (units + 3) / 4 : room);
    if (want < 1) want = 1;
    uint32_t per_block = (uint32_t)((units + want - 1) / want);
    if ((units_max + per_block - 1) / per_block > max_lists) per_block = (units_max + max_lists - 1) / max_lists;
    ListedGroupsLaunch l{B, (uint32_t)out->items.size(), 0, per_block, (uint32_t)want, n_pass, nq_max};
    for (const Pass& p : passes) {
      if (p.B != B) continue;
      const FxGroup& g = groups[p.group];
      const uint32_t rpu = rpu_of(B);
      uint32_t slot = 0;
      for (uint32_t u = 0; u < p.units; u += per_block, slot++) {
        ListedGroupItem it{};
        const uint64_t first = (uint64_t)u * rpu, left = count_of(g.filter) - first, room = (uint64_t)per_block * rpu;
        it.list = list_of(g.filter) + first;
        it.count = (uint32_t)(left < room ? left : room);
        it.units = (it.count + rpu - 1) / rpu;
        it.nq = p.nq;
        it.slot = slot;
        for (uint32_t j = 0; j < p.nq; j++) it.q[j] = g.queries[p.q0 + j];
        out->items.push_back(it);
      }
      if (slot > out->lists_per_query) out->lists_per_query = slot;
    }
    l.count = (uint32_t)out->items.size() - l.begin;
    out->launches[out->n_launches++] = l;
  }
}
// the f32 rows: mode C in the classes 8 / 4 / 1 with 64 / B rows a unit, mode M in one class with 64-row tiles;
// pass_of(nq_left) -> FxPass
template <class ListOf, class CountOf, class PassOf, class OccOf>
static inline void listed_groups_plan(const std::vector<FxGroup>& groups, bool mode_m, int n_cus, uint32_t max_lists, ListOf&& list_of,
                                      CountOf&& count_of, PassOf&& pass_of, OccOf&& occ_of, ListedGroupsPlan* out) {
  static const int kClassesC[3] = {8, 4, 1}, kClassesM[1] = {0};
  listed_groups_plan_core(
      groups, mode_m, mode_m ? kClassesM : kClassesC, mode_m ? 1 : 3, n_cus, max_lists, list_of, count_of,
      [&](uint32_t, uint32_t nq_left) { return pass_of(nq_left); }, occ_of, [&](int B) { return mode_m ? 64u : 64u / (uint32_t)B; }, out);
}

// ---- one filter per query over the SQ8 / Binary / half images (vdb_hip_index_search_batch_filters_mode) ----
// The grouping of 4.1n with the route rule of 4.1o: every group takes the route filter_mode_route gives it with ITS count and ITS
// number of queries — `listed_available` as the one-filter call computes it: the mode and metric have a listed kernel and the plan
// of the group's first pass fits the LDS.  (Auto therefore sends an SQ8 group to the listed kernel only with at most
// kFmSq8ListedMaxQueries queries; Binary and Cosine / DotProduct over a half image have no listed kernel at all.)
template <class CountOf>
static inline std::vector<FxGroup> filters_mode_groups(const uint32_t* fq, uint32_t nq, uint32_t n_filters, int64_t opt, int mode, int metric,
                                                       uint64_t n_rows, uint32_t dim, uint32_t k, int n_cus, CountOf&& count_of) {
  const bool half = mode == kFmModeBf16 || mode == kFmModeF16;
  // (filters_exact_groups asks pass_of only whether the group's first pass fits: answered per group below instead)
  std::vector<FxGroup> g = filters_exact_groups(fq, nq, n_filters, 2, n_rows, count_of, [](uint32_t) { return FxPass{0, 0}; });
  for (FxGroup& x : g) {
    if (x.filter == n_filters) continue;
    const uint32_t nq_g = (uint32_t)x.queries.size();
    const uint64_t count = count_of(x.filter);
    const bool listed_ok = filter_mode_has_listed(mode, metric) && mode_listed_plan(half, dim, k, count, nq_g, n_cus).blocks > 0;
    x.route = filter_mode_route(opt, mode, metric, count, n_rows, nq_g, listed_ok);
  }
  return g;
}
// The grouped launches of the groups on the listed route: every group is cut into the passes mode_listed_plan runs for it alone
// (SQ8: 8 / 4 / 1 queries over units of 64 rows; half Euclidean: 16 / 4 / 1 over units of 64 / B rows), every pass into chunks of
// per_block units, per_block by the rule above with mode_listed_plan's room (n_cus x resident blocks at the class's LDS footprint),
// so a table of one pass is mode_listed_plan's plan.  The item is 4.1n's record unchanged.
template <class ListOf, class CountOf>
static inline void mode_groups_plan(const std::vector<FxGroup>& groups, bool half, uint32_t dim, uint32_t k, int n_cus, uint32_t max_lists,
                                    ListOf&& list_of, CountOf&& count_of, ListedGroupsPlan* out) {
  static const int kClassesSq8[3] = {8, 4, 1}, kClassesHalf[3] = {16, 4, 1};
  listed_groups_plan_core(
      groups, false, half ? kClassesHalf : kClassesSq8, 3, n_cus, max_lists, list_of, count_of,
      [&](uint32_t f, uint32_t nq_left) {
        const ModeListedPlan p = mode_listed_plan(half, dim, k, count_of(f), nq_left, n_cus);
        return FxPass{p.B, p.blocks > 0 ? p.nq_pass : 0u};
      },
      [&](int B, uint32_t) {
        const uint64_t lds = half ? fm_half_l2_lds_bytes(B, k, dim) : fm_sq8_lds_bytes(B, k, dim);
        const uint64_t per_cu = kFmLdsBudget / (lds ? lds : 1), cap = half ? 3 : 4;
        return (uint32_t)(per_cu > cap ? cap : per_cu);
      },
      [&](int B) { return half ? 64u / (uint32_t)B : 64u; }, out);
}

// ---- one filter per query in the fused searches (vdb_hip_index_hybrid_search_filters, vdb_hip_index_multi_query_search_filters;
// DESIGN 4.1r) ----
// The two kinds of a call ask their walks for lists of different lengths (hybrid: 2k without a filter, max(4k, k + 10) with one), so a
// call runs in two PHASES on one lease: the unfiltered units through the plain walk, then the filtered ones through the walk with one
// filter per query; each phase is one walk call and one fusion launch over that walk's result block.  A unit is a user query (hybrid)
// or a group of reformulations (multi-query); it fuses lists_of(u) vector lists of its phase's length plus extra_of(u) further records
// (its text hits), and that sum is held to `limit` (what one block's LDS takes) unit by unit, with the unit's OWN list length: a
// query that is legal without a filter may be past the limit with one.
constexpr int kPhaseUnfiltered = 0, kPhaseFiltered = 1;
// text.rs:137 (k * 2) and 244 (k.saturating_mul(4).max(k + 10)); 64-bit, so that a product past u32 is seen by the limit
static inline uint64_t hybrid_list_len(uint32_t k, bool filtered) {
  const uint64_t a = (uint64_t)k * 4, b = (uint64_t)k + 10;
  return filtered ? (a > b ? a : b) : (uint64_t)k * 2;
}
struct FusedPhase {
  uint64_t list_len = 0;         // k' of the phase's walk
  std::vector<uint32_t> units;   // positions in the call, ascending
  uint64_t lists = 0;            // vectors the phase's walk searches (the sum of lists_of over its units)
  uint64_t most = 0;             // records of its largest unit: sizes the fusion launch
};
struct FusedPhasesPlan {
  FusedPhase phase[2];           // [kPhaseUnfiltered], [kPhaseFiltered]; a phase without units launches nothing
  int64_t over = -1;             // the first unit past `limit` (nothing may run then), -1: none ...
  uint64_t over_records = 0;     // ... and what it would fuse
  int over_phase = 0;
};
// fq[u] in 0..n_filters, n_filters = no filter (null with n_units = 0 only); len_unfiltered / len_filtered: the phases' k'
template <class ListsOf, class ExtraOf>
static inline FusedPhasesPlan fused_phases_plan(const uint32_t* fq, uint32_t n_units, uint32_t n_filters, uint64_t len_unfiltered,
                                                uint64_t len_filtered, uint64_t limit, ListsOf&& lists_of, ExtraOf&& extra_of) {
  FusedPhasesPlan p;
  p.phase[kPhaseUnfiltered].list_len = len_unfiltered;
  p.phase[kPhaseFiltered].list_len = len_filtered;
  for (uint32_t u = 0; u < n_units; u++) {
    const int ph = fq[u] < n_filters ? kPhaseFiltered : kPhaseUnfiltered;
    FusedPhase& P = p.phase[ph];
    const uint64_t lists = lists_of(u);
    const uint64_t records = lists * P.list_len + (uint64_t)extra_of(u);  // (lists <= 2^32, list_len < 2^35: inside 64 bits)
    if (records > limit && p.over < 0) {
      p.over = u;
      p.over_records = records;
      p.over_phase = ph;
    }
    P.units.push_back(u);
    P.lists += lists;
    if (records > P.most) P.most = records;
  }
  return p;
}

}  // namespace vdb
