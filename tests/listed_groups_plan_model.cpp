// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the plan of an exact call
// with one filter per query (filters_exact_groups / listed_groups_plan).  tests/test_filters_exact_cpu.py builds it
// with ASan + UBSan and reads the JSON line.  Random and boundary tables — counts 0, 1, RPG +- 1 and tile +- 1, group sizes around
// 8 and 16, 1 ... 4 096 groups, 1 and 256 CUs, the three route options, both arithmetic modes, shapes the listed kernels cannot
// take — are planned, and the plan is held to what the kernels need:
//   * every (query, list position) of a listed group is covered by exactly one work item, no item is empty, no item crosses a pass
//     (its queries are one pass of one group, its rows one contiguous chunk of that group's list);
//   * chunks of a pass are numbered 0, 1, ... (the partial-list slots) and stay under lists_per_query <= max_lists;
//   * a launch holds at most want + passes blocks, all of its class;
//   * a group the listed kernels cannot take, an empty filter and the unfiltered queries are on no item;
//   * a table of one filter and one pass yields sweep_listed_plan's per_block and block count (transcribed below).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "vdb_filter_route.hpp"

using namespace vdb;

static int g_bad = 0;
static long g_cases = 0, g_checks = 0, g_items = 0, g_listed = 0, g_dense = 0, g_capped = 0;
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

// the pass rule of sweep_listed_plan (sweep_listed.hip), restated: mode C picks B by nq_left and halves it while the k-lists do
// not fit 60 KB; mode M takes up to 16 queries and halves while 160 KB do not hold them.  `unit` bytes stand for k * 8 (+ queries).
struct Shape {
  bool mode_m;
  uint64_t per_query_bytes;  // LDS a query of a pass costs
  uint64_t fixed_bytes;      // ... and what a block costs whatever the pass
  uint64_t budget() const { return mode_m ? 160 * 1024 : 60 * 1024; }
  FxPass operator()(uint32_t nq_left) const {
    if (nq_left == 0) return FxPass{0, 0};
    if (mode_m) {
      uint32_t nqp = nq_left < 16 ? nq_left : 16;
      while (nqp > 1 && fixed_bytes + nqp * per_query_bytes > budget()) nqp = (nqp + 1) / 2;
      if (fixed_bytes + nqp * per_query_bytes > budget()) return FxPass{0, 0};
      return FxPass{0, nqp};
    }
    int B = nq_left >= 5 ? 8 : (nq_left >= 2 ? 4 : 1);
    while (B > 1 && fixed_bytes + (uint64_t)B * per_query_bytes > budget()) B = B == 8 ? 4 : 1;
    if (fixed_bytes + (uint64_t)B * per_query_bytes > budget()) return FxPass{0, 0};
    return FxPass{B, nq_left < (uint32_t)B ? nq_left : (uint32_t)B};
  }
  uint32_t occ(int B, uint32_t nq_max) const {
    if (!mode_m) return B == 1 ? 4u : (B == 8 ? 2u : 3u);
    const uint64_t lds = fixed_bytes + nq_max * per_query_bytes, n = budget() / (lds ? lds : 1);
    return (uint32_t)(n > 4 ? 4 : (n < 1 ? 1 : n));
  }
};

struct Call {
  std::vector<uint64_t> counts;  // rows per filter
  std::vector<uint32_t> fq;      // filter per query (counts.size() = none)
  uint64_t n_rows;
  int64_t opt;
  int n_cus;
  uint32_t max_lists;
  Shape shape;
};

static void check(const Call& c) {
  g_cases++;
  const uint32_t nf = (uint32_t)c.counts.size(), nq = (uint32_t)c.fq.size();
  static std::vector<uint32_t> arena(1);  // list pointers are only compared and subtracted: one base, never dereferenced
  const uint32_t* base0 = arena.data();
  std::vector<uint64_t> off(nf + 1, 0);
  for (uint32_t f = 0; f < nf; f++) off[f + 1] = off[f] + c.counts[f] + 7;  // disjoint ranges with a gap
  auto count_of = [&](uint32_t f) { return c.counts[f]; };
  auto list_of = [&](uint32_t f) { return reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(base0) + 4 * off[f]); };
  auto pass_of = [&](uint32_t nq_left) { return c.shape(nq_left); };
  auto occ_of = [&](int B, uint32_t nq_max) { return c.shape.occ(B, nq_max); };
  const std::vector<FxGroup> groups = filters_exact_groups(c.fq.data(), nq, nf, c.opt, c.n_rows, count_of, pass_of);

  // ---- the groups: every query in exactly one, in call order, on the route filter_route gives the group ----
  std::vector<int> seen(nq, 0);
  std::map<uint32_t, uint32_t> group_of_filter;
  for (uint32_t gi = 0; gi < groups.size(); gi++) {
    const FxGroup& g = groups[gi];
    expect(!g.queries.empty(), "empty group");
    expect(group_of_filter.emplace(g.filter, gi).second, "a filter in two groups", g.filter);
    for (size_t j = 0; j < g.queries.size(); j++) {
      expect(g.queries[j] < nq && c.fq[g.queries[j]] == g.filter, "a query in the wrong group", g.queries[j]);
      if (g.queries[j] < nq) seen[g.queries[j]]++;
      if (j) expect(g.queries[j - 1] < g.queries[j], "call order lost inside a group");
    }
    const uint32_t nq_g = (uint32_t)g.queries.size();
    if (g.filter == nf) {
      expect(g.route == kFilterRouteDense, "unfiltered queries on the listed route");
    } else {
      const int want = filter_route(c.opt, c.shape(nq_g).nq_pass > 0, c.counts[g.filter], c.n_rows, nq_g);
      expect(g.route == want, "group route differs from filter_route", g.filter);
      if (c.counts[g.filter] == 0 || c.shape(nq_g).nq_pass == 0) expect(g.route == kFilterRouteDense, "a group the listed kernels cannot take is listed");
    }
    (g.route == kFilterRouteListed ? g_listed : g_dense)++;
  }
  for (uint32_t i = 0; i < nq; i++) expect(seen[i] == 1, "a query in no group or in two", i);

  // ---- the grouped launches ----
  ListedGroupsPlan plan;
  listed_groups_plan(groups, c.shape.mode_m, c.n_cus, c.max_lists, list_of, count_of, pass_of, occ_of, &plan);
  g_items += (long)plan.items.size();
  expect(plan.n_launches <= (c.shape.mode_m ? 1u : 3u), "too many launches", plan.n_launches);
  expect(plan.lists_per_query <= (c.max_lists ? c.max_lists : 1), "more lists per query than allowed", plan.lists_per_query, c.max_lists);
  // cover[q] = rows of its filter's list covered so far; pass bookkeeping: (first query of the pass) -> next slot, next row
  std::vector<uint64_t> covered(nq, 0);
  uint32_t at = 0, slots_max = 0;
  for (uint32_t li = 0; li < plan.n_launches; li++) {
    const ListedGroupsLaunch& l = plan.launches[li];
    expect(l.begin == at && l.count > 0, "launches are not consecutive", l.begin, at);
    expect(l.count <= (uint64_t)l.want + l.passes, "more blocks than want + passes", l.count, (uint64_t)l.want + l.passes);
    expect(l.want <= (uint64_t)std::max(c.n_cus, 1) * c.shape.occ(l.B, l.nq_max), "want above the chip", l.want);
    const uint32_t rpu = c.shape.mode_m ? 64u : 64u / (uint32_t)(l.B ? l.B : 1);
    std::map<uint32_t, std::pair<uint32_t, uint64_t>> pass_state;  // first query -> (next slot, next row)
    uint32_t passes = 0;
    for (uint32_t i = l.begin; i < l.begin + l.count && i < plan.items.size(); i++) {
      const ListedGroupItem& it = plan.items[i];
      expect(it.count > 0 && it.nq > 0 && it.units > 0, "an empty item", i);
      expect(it.units == (it.count + rpu - 1) / rpu && it.units <= l.per_block, "units do not match the chunk", it.units, l.per_block);
      expect(it.nq <= kLgPassQueries && it.nq <= l.nq_max, "pass wider than the launch says", it.nq, l.nq_max);
      const uint32_t f = it.nq ? c.fq[it.q[0]] : nf;
      expect(f < nf, "an item of unfiltered queries");
      if (f >= nf) continue;
      const FxGroup& g = groups[group_of_filter[f]];
      expect(g.route == kFilterRouteListed, "an item of a group on mask substitution", f);
      // one pass of one group: consecutive members of the group, the width the pass rule gives at that point
      const size_t p0 = (size_t)(std::find(g.queries.begin(), g.queries.end(), it.q[0]) - g.queries.begin());
      for (uint32_t j = 0; j < it.nq; j++) expect(p0 + j < g.queries.size() && g.queries[p0 + j] == it.q[j], "item crosses a pass or a group", i, j);
      const FxPass want = c.shape((uint32_t)(g.queries.size() - p0));
      expect(want.nq_pass == it.nq && (c.shape.mode_m ? 0 : want.B) == l.B, "pass width / class differs from the pass rule", it.nq, want.nq_pass);
      uint64_t walked = 0;  // the pass starts where the rule's passes before it end
      for (size_t q0 = 0; q0 < p0;) {
        q0 += c.shape((uint32_t)(g.queries.size() - q0)).nq_pass;
        walked = q0;
      }
      expect(walked == p0, "a pass that does not start at a pass boundary", p0);
      // one contiguous chunk of the list, chunks of a pass in order, slots 0, 1, ...
      const uint64_t first = (uint64_t)(it.list - list_of(f));
      auto ins = pass_state.emplace(it.q[0], std::make_pair(0u, (uint64_t)0));
      if (ins.second) passes++;
      expect(it.slot == ins.first->second.first, "slot out of order", it.slot, ins.first->second.first);
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

  // ---- one filter, one pass: sweep_listed_plan's per_block and blocks (transcribed from sweep_listed.hip) ----
  if (groups.size() == 1 && groups[0].route == kFilterRouteListed && plan.n_launches == 1 && plan.launches[0].passes == 1 && c.max_lists >= 4096) {
    const FxPass p = c.shape(nq);
    const uint32_t rpu = c.shape.mode_m ? 64u : 64u / (uint32_t)p.B;
    const uint64_t units = (c.counts[groups[0].filter] + rpu - 1) / rpu, room = (uint64_t)c.n_cus * c.shape.occ(p.B, p.nq_pass);
    const uint64_t want = c.shape.mode_m ? std::min(units, room) : std::max<uint64_t>(1, std::min((units + 3) / 4, room));
    const uint64_t per_block = (units + want - 1) / want, blocks = (units + per_block - 1) / per_block;
    expect(plan.launches[0].per_block == per_block && plan.items.size() == blocks, "one filter: not the one-filter plan", plan.items.size(), blocks);
  }
}

int main() {
  const Shape shapes[] = {
      {false, 10 * 8 + 8, 0},            // mode C, k = 10, a CPL dim
      {false, 200 * 8 + 8 + 3072, 0},    // mode C, k = 200, generic dim 768: B = 8 still fits
      {false, 3000 * 8 + 8, 0},          // mode C, k = 3000: B falls to 1 (two lists pass 60 KB)
      {false, 9000 * 8 + 8, 0},          // mode C: not even one list fits — no listed kernel
      {true, 768 * 4 + 10 * 8, 35136},   // mode M, k = 10, dim 768
      {true, 4096 * 4 + 200 * 8, 35136}, // mode M, dim 4096, k = 200: the pass shrinks below 16
      {true, 40000 * 4, 35136},          // mode M: one query does not fit
  };
  const uint64_t count_edges[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 25000, 100000};
  const uint32_t size_edges[] = {1, 2, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33};
  uint64_t s = 42;
  auto rnd = [&](uint64_t m) { return (s = mix(s)) % m; };
  for (int round = 0; round < 2600; round++) {
    Call c;
    c.shape = shapes[rnd(7)];
    c.n_rows = 100000;
    c.opt = (int64_t)rnd(3);
    c.n_cus = rnd(2) ? 256 : 1;
    c.max_lists = rnd(4) == 0 ? 1 + (uint32_t)rnd(6) : 4096;
    uint32_t nf = round < 40 ? 1 : (round % 97 == 0 ? 4096 : 1 + (uint32_t)rnd(round % 5 == 0 ? 300 : 12));
    if (round == 41) nf = 4096;
    for (uint32_t f = 0; f < nf; f++) c.counts.push_back(rnd(3) ? count_edges[rnd(18)] : rnd(30000));
    std::vector<uint32_t> fq;
    for (uint32_t f = 0; f < nf; f++) {
      const uint32_t sz = nf > 300 ? 1 + (uint32_t)rnd(2) : (rnd(3) ? size_edges[rnd(13)] : 1 + (uint32_t)rnd(40));
      for (uint32_t j = 0; j < sz; j++) fq.push_back(f);
    }
    if (round >= 40)
      for (uint32_t j = (uint32_t)rnd(9); j > 0; j--) fq.push_back(nf);  // unfiltered queries
    for (size_t i = fq.size(); i > 1; i--) std::swap(fq[i - 1], fq[rnd(i)]);  // no group is contiguous
    c.fq = fq;
    check(c);
  }
  std::printf("{\"ok\": %s, \"violations\": %d, \"cases\": %ld, \"checks\": %ld, \"items\": %ld, \"listed_groups\": %ld, \"dense_groups\": %ld, \"capped\": %ld}\n",
              g_bad ? "false" : "true", g_bad, g_cases, g_checks, g_items, g_listed, g_dense, g_capped);
  return g_bad ? 1 : 0;
}
