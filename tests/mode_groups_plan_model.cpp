// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the plan of an exact call
// with one filter per query over the SQ8 codes, the sign bits or a half image (filters_mode_groups / mode_groups_plan).
// tests/test_filters_modes_cpu.py builds it with ASan + UBSan and reads the JSON line.  Random and boundary tables — counts 0, 1,
// unit +- 1, around 3/4 of the rows, group sizes around 3, 4, 8 and 16, 1 ... 4 096 groups, 1 and 256 CUs, the three route options,
// the four modes, all three metrics, shapes whose wide passes do not fit the LDS — are planned, and the plan is held to:
//   * the route of every group is filter_mode_route's with the group's count and its number of queries (listed_available as the
//     one-filter call computes it);
//   * every query of a listed group appears in exactly the passes mode_listed_plan gives its group alone (the same widths at the same
//     boundaries), every (query, list position) is covered exactly once;
//   * no block is empty, chunks of a pass are numbered 0, 1, ... and every pass has at most lists_per_query <= max_lists chunks;
//   * at most three launches, one per pass width present, each with at most want + passes blocks;
//   * a table of one pass equals mode_listed_plan (per_block and block count);
//   * Binary and Cosine / DotProduct over a half image never plan a listed group.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "vdb_filter_route.hpp"

using namespace vdb;

static int g_bad = 0;
static long g_cases = 0, g_checks = 0, g_items = 0, g_listed = 0, g_dense = 0, g_capped = 0, g_three = 0, g_one_pass = 0;
static void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0) {
  g_checks++;
  if (!ok && g_bad++ < 50) std::fprintf(stderr, "violation: %s (%llu, %llu) in case %ld\n", what, (unsigned long long)a, (unsigned long long)b, g_cases);
}
static uint64_t mix(uint64_t x) {  // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Call {
  std::vector<uint64_t> counts;  // rows per filter
  std::vector<uint32_t> fq;      // filter per query (counts.size() = none)
  uint64_t n_rows;
  int64_t opt;
  int mode, metric, n_cus;
  uint32_t dim, k, max_lists;
};

static void check(const Call& c) {
  g_cases++;
  const uint32_t nf = (uint32_t)c.counts.size(), nq = (uint32_t)c.fq.size();
  const bool half = c.mode == kFmModeBf16 || c.mode == kFmModeF16;
  static std::vector<uint32_t> arena(1);  // list pointers are only compared and subtracted: one base, never dereferenced
  const uint32_t* base0 = arena.data();
  std::vector<uint64_t> off(nf + 1, 0);
  for (uint32_t f = 0; f < nf; f++) off[f + 1] = off[f] + c.counts[f] + 7;  // disjoint ranges with a gap
  auto count_of = [&](uint32_t f) { return c.counts[f]; };
  auto list_of = [&](uint32_t f) { return reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(base0) + 4 * off[f]); };
  auto alone = [&](uint32_t f, uint32_t nq_left) { return mode_listed_plan(half, c.dim, c.k, c.counts[f], nq_left, c.n_cus); };
  const std::vector<FxGroup> groups = filters_mode_groups(c.fq.data(), nq, nf, c.opt, c.mode, c.metric, c.n_rows, c.dim, c.k, c.n_cus, count_of);

  // ---- the groups: every query in exactly one, in call order, on the route filter_mode_route gives the group ----
  std::vector<int> seen(nq, 0);
  std::map<uint32_t, uint32_t> group_of_filter;
  for (uint32_t gi = 0; gi < groups.size(); gi++) {
    const FxGroup& g = groups[gi];
    expect(!g.queries.empty(), "empty group");
    expect(group_of_filter.emplace(g.filter, gi).second, "a filter in two groups", g.filter);
    if (gi) expect(groups[gi - 1].queries[0] < g.queries[0], "groups not in the order their first query appears");
    for (size_t j = 0; j < g.queries.size(); j++) {
      expect(g.queries[j] < nq && c.fq[g.queries[j]] == g.filter, "a query in the wrong group", g.queries[j]);
      if (g.queries[j] < nq) seen[g.queries[j]]++;
      if (j) expect(g.queries[j - 1] < g.queries[j], "call order lost inside a group");
    }
    const uint32_t nq_g = (uint32_t)g.queries.size();
    if (g.filter == nf) {
      expect(g.route == kFilterRouteDense, "unfiltered queries on the listed route");
    } else {
      const bool listed_ok = filter_mode_has_listed(c.mode, c.metric) && alone(g.filter, nq_g).blocks > 0;
      const int want = filter_mode_route(c.opt, c.mode, c.metric, c.counts[g.filter], c.n_rows, nq_g, listed_ok);
      expect(g.route == want, "group route differs from filter_mode_route", g.filter);
      if (c.counts[g.filter] == 0 || !listed_ok) expect(g.route == kFilterRouteDense, "a group the listed kernels cannot take is listed");
      if (c.mode == kFmModeBinary || (half && c.metric != kFmMetricEuclidean)) expect(g.route == kFilterRouteDense, "a listed group in a mode without a listed kernel");
      if (c.opt <= 0 && c.mode == kFmModeSq8 && nq_g > kFmSq8ListedMaxQueries) expect(g.route == kFilterRouteDense, "auto: an SQ8 group of more than three queries listed");
    }
    (g.route == kFilterRouteListed ? g_listed : g_dense)++;
  }
  for (uint32_t i = 0; i < nq; i++) expect(seen[i] == 1, "a query in no group or in two", i);

  // ---- the grouped launches ----
  ListedGroupsPlan plan;
  mode_groups_plan(groups, half, c.dim, c.k, c.n_cus, c.max_lists, list_of, count_of, &plan);
  g_items += (long)plan.items.size();
  expect(plan.n_launches <= 3u, "too many launches", plan.n_launches);
  if (plan.n_launches == 3) g_three++;
  expect(plan.lists_per_query <= (c.max_lists ? c.max_lists : 1), "more lists per query than allowed", plan.lists_per_query, c.max_lists);
  std::vector<uint64_t> covered(nq, 0);
  uint32_t at = 0, slots_max = 0;
  int last_B = 1 << 30;
  for (uint32_t li = 0; li < plan.n_launches; li++) {
    const ListedGroupsLaunch& l = plan.launches[li];
    expect(l.begin == at && l.count > 0, "launches are not consecutive", l.begin, at);
    expect(l.B < last_B && (half ? (l.B == 16 || l.B == 4 || l.B == 1) : (l.B == 8 || l.B == 4 || l.B == 1)), "launch classes: one per width, widest first", (uint64_t)l.B);
    last_B = l.B;
    expect(l.count <= (uint64_t)l.want + l.passes, "more blocks than want + passes", l.count, (uint64_t)l.want + l.passes);
    const uint64_t lds = half ? fm_half_l2_lds_bytes(l.B, c.k, c.dim) : fm_sq8_lds_bytes(l.B, c.k, c.dim);
    expect(lds <= kFmLdsBudget, "a launch whose class does not fit the LDS", lds);
    const uint64_t per_cu = std::min<uint64_t>(kFmLdsBudget / lds, half ? 3 : 4);
    expect(l.want <= (uint64_t)std::max(c.n_cus, 1) * per_cu, "want above the chip", l.want);
    const uint32_t rpu = half ? 64u / (uint32_t)l.B : 64u;
    std::map<uint32_t, std::pair<uint32_t, uint64_t>> pass_state;  // first query -> (next slot, next row)
    uint32_t passes = 0;
    for (uint32_t i = l.begin; i < l.begin + l.count && i < plan.items.size(); i++) {
      const ListedGroupItem& it = plan.items[i];
      expect(it.count > 0 && it.nq > 0 && it.units > 0, "an empty item", i);
      expect(it.units == (it.count + rpu - 1) / rpu && it.units <= l.per_block, "units do not match the chunk", it.units, l.per_block);
      expect(it.nq <= kLgPassQueries && it.nq <= (uint32_t)l.B && it.nq <= l.nq_max, "pass wider than the launch's class", it.nq, l.nq_max);
      const uint32_t f = it.nq ? c.fq[it.q[0]] : nf;
      expect(f < nf, "an item of unfiltered queries");
      if (f >= nf) continue;
      const FxGroup& g = groups[group_of_filter[f]];
      expect(g.route == kFilterRouteListed, "an item of a group on mask substitution", f);
      // one pass of one group: consecutive members of the group, the width mode_listed_plan gives the group alone at that point
      const size_t p0 = (size_t)(std::find(g.queries.begin(), g.queries.end(), it.q[0]) - g.queries.begin());
      for (uint32_t j = 0; j < it.nq; j++) expect(p0 + j < g.queries.size() && g.queries[p0 + j] == it.q[j], "item crosses a pass or a group", i, j);
      const ModeListedPlan want = alone(f, (uint32_t)(g.queries.size() - p0));
      expect(want.blocks > 0 && want.nq_pass == it.nq && want.B == l.B, "pass width / class differs from the one-filter plan", it.nq, want.nq_pass);
      size_t walked = 0;  // the pass starts where the one-filter call's passes before it end
      for (size_t q0 = 0; q0 < p0;) {
        const uint32_t step = alone(f, (uint32_t)(g.queries.size() - q0)).nq_pass;
        if (!step) break;
        q0 += step;
        walked = q0;
      }
      expect(walked == p0, "a pass that does not start at a pass boundary", p0);
      const uint64_t first = (uint64_t)(it.list - list_of(f));
      auto ins = pass_state.emplace(it.q[0], std::make_pair(0u, (uint64_t)0));
      if (ins.second) passes++;
      expect(it.slot == ins.first->second.first, "slot out of order", it.slot, ins.first->second.first);
      expect(it.slot < plan.lists_per_query, "a pass with more chunks than lists_per_query", it.slot, plan.lists_per_query);
      expect(first == ins.first->second.second, "chunk does not follow the one before", first, ins.first->second.second);
      expect(first % rpu == 0 && first + it.count <= c.counts[f], "chunk outside the list or off a unit boundary", first, it.count);
      if (first + it.count < c.counts[f]) expect(it.units == l.per_block && it.count == (uint64_t)l.per_block * rpu, "a short chunk inside a pass", i);
      ins.first->second.first++;
      ins.first->second.second = first + it.count;
      slots_max = std::max(slots_max, it.slot + 1);
      for (uint32_t j = 0; j < it.nq; j++) {
        expect(covered[it.q[j]] == first, "a (query, position) covered twice or skipped", it.q[j], first);
        covered[it.q[j]] = first + it.count;
      }
      for (uint32_t j = it.nq; j < kLgPassQueries; j++) expect(it.q[j] == 0, "unused query entries not zero");
    }
    expect(passes == l.passes, "pass count of the launch", passes, l.passes);
    at += l.count;
  }
  expect(at == plan.items.size(), "items outside every launch", at, plan.items.size());
  expect(slots_max == plan.lists_per_query, "lists_per_query is not the largest chunk count", slots_max, plan.lists_per_query);
  for (const FxGroup& g : groups)
    for (uint32_t q : g.queries)
      expect(covered[q] == (g.route == kFilterRouteListed ? c.counts[g.filter] : 0), "coverage of a query", q, covered[q]);
  if (c.max_lists < 4096 && plan.lists_per_query == c.max_lists) g_capped++;

  // ---- a table of one pass: mode_listed_plan's per_block and blocks ----
  if (plan.n_launches == 1 && plan.launches[0].passes == 1 && c.max_lists >= 4096) {
    const ListedGroupItem& it0 = plan.items[0];
    const uint32_t f = c.fq[it0.q[0]];
    const ModeListedPlan p = alone(f, it0.nq);
    expect(groups[group_of_filter[f]].queries.size() == it0.nq, "one pass, but not the whole group");
    expect(plan.launches[0].per_block == p.per_block && plan.items.size() == (size_t)p.blocks && plan.launches[0].B == p.B,
           "one pass: not the one-filter plan", plan.items.size(), (uint64_t)p.blocks);
    g_one_pass++;
  }
}

int main() {
  const int modes[] = {kFmModeSq8, kFmModeBinary, kFmModeBf16, kFmModeF16};
  // (dim, k): small; the headline shape; k-lists that push the wide classes out of the LDS; a shape where only one query fits; none fits
  const uint32_t shapes[][2] = {{17, 3}, {768, 10}, {100, 64}, {768, 2000}, {4096, 128}, {4096, 4000}, {20000, 2000}, {60000, 10}};
  const uint64_t count_edges[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 25000, 74999, 75000, 75001, 100000};
  const uint32_t size_edges[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 21, 31, 32, 33};
  uint64_t s = 4242;
  auto rnd = [&](uint64_t m) { return (s = mix(s)) % m; };
  for (int round = 0; round < 3200; round++) {
    Call c;
    c.mode = modes[round < 60 ? (round & 1 ? 0 : 3) : rnd(8) % 4 == 1 ? 1 : (rnd(3) == 0 ? 0 : (rnd(2) ? 2 : 3))];
    if (round >= 60 && round % 3 == 0) c.mode = kFmModeSq8;
    c.metric = (c.mode == kFmModeBf16 || c.mode == kFmModeF16) ? (rnd(4) ? kFmMetricEuclidean : (int)rnd(3)) : (int)rnd(3);
    const uint32_t* sh = shapes[rnd(3) ? rnd(3) : rnd(8)];
    c.dim = sh[0];
    c.k = sh[1];
    c.n_rows = 100000;
    c.opt = (int64_t)rnd(3);
    c.n_cus = rnd(2) ? 256 : 1;
    c.max_lists = rnd(4) == 0 ? 1 + (uint32_t)rnd(6) : 4096;
    uint32_t nf = round < 60 ? 1 : (round % 97 == 0 ? 4096 : 1 + (uint32_t)rnd(round % 5 == 0 ? 300 : 12));
    for (uint32_t f = 0; f < nf; f++) c.counts.push_back(rnd(3) ? count_edges[rnd(21)] : rnd(30000));
    std::vector<uint32_t> fq;
    for (uint32_t f = 0; f < nf; f++) {
      const uint32_t sz = nf > 300 ? 1 + (uint32_t)rnd(3) : (rnd(3) ? size_edges[rnd(16)] : 1 + (uint32_t)rnd(40));
      for (uint32_t j = 0; j < sz; j++) fq.push_back(f);
    }
    if (round >= 60)
      for (uint32_t j = (uint32_t)rnd(9); j > 0; j--) fq.push_back(nf);  // unfiltered queries
    for (size_t i = fq.size(); i > 1; i--) std::swap(fq[i - 1], fq[rnd(i)]);  // no group is contiguous
    c.fq = fq;
    check(c);
  }
  std::printf("{\"ok\": %s, \"violations\": %d, \"cases\": %ld, \"checks\": %ld, \"items\": %ld, \"listed_groups\": %ld, \"dense_groups\": %ld, \"capped\": %ld, "
              "\"three_launches\": %ld, \"one_pass\": %ld}\n",
              g_bad ? "false" : "true", g_bad, g_cases, g_checks, g_items, g_listed, g_dense, g_capped, g_three, g_one_pass);
  return g_bad ? 1 : 0;
}
