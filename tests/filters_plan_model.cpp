// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the launch plan of a graph
// call with one filter per query (filters_plan_round / filters_walk_ladders).  tests/test_filters_graph_cpu.py builds
// it with ASan + UBSan and reads the JSON line.  Generated calls — ef, the largest list, filter sizes 0 ... n_rows, 1 ... 300 queries,
// the three routes — are run through the library's own ladder loop with a walk that overflows by a fixed function of (query, list
// capacity); the expectations restate the single-filter host loop for one query at a time.  A second set of calls puts every query
// on ONE filter and holds the plan to a transcription of the host loop the one-filter call had before it was served by this path:
// rounds, one launch per round, its capacity, walks per CU, the slot order and the queries left for the exact pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "vdb_filter_route.hpp"

using namespace vdb;

static int g_bad = 0;
static long g_cases = 0, g_checks = 0, g_rounds = 0, g_shared_rounds = 0, g_split_rounds = 0, g_reruns = 0, g_failed = 0;
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

// the LDS footprint of a walk launch (hnsw_lds_bytes): list keys and flags, two neighbour arrays, control words, the query
struct Lds {
  uint32_t nbmax, qbytes;
  uint64_t operator()(uint32_t cap) const {
    const uint64_t s = (uint64_t)cap * 8 + (uint64_t)nbmax * 8 + 16 + (((uint64_t)cap + 15) & ~15ull) + qbytes;
    return (s + 15) & ~15ull;
  }
};

struct Query {
  uint64_t uid;      // identity across the permuted / reduced calls
  uint64_t matched;  // rows in its filter
  uint32_t thresh;   // its walk overflows every list shorter than this (0: never)
};
struct Trace {
  int route = 0;               // 0 nothing ran, 1 the walk answered, 2 the exact pass
  std::vector<uint32_t> caps;  // the logical capacity of every attempt
  bool operator==(const Trace& o) const { return route == o.route && caps == o.caps; }
};

// one query alone, as the single-filter host loop runs it (hnsw_filtered.hip) -> false: the call is refused / fails
static bool alone(const Query& q, int route, uint32_t ef, uint64_t n_rows, uint32_t cap_max, Trace* t) {
  *t = Trace{};
  if (q.matched == 0) return true;
  const FilterGraphPlan p = filter_graph_route(route, ef, q.matched, n_rows, cap_max);
  if (p.route == kFgRefuse) return false;
  if (p.route == kFgExact) {
    t->route = 2;
    return true;
  }
  for (uint64_t cap = p.cap;;) {
    t->caps.push_back((uint32_t)cap);
    const bool over = cap < q.thresh;
    if (!over) {
      t->route = 1;
      return true;
    }
    if (cap >= cap_max) break;
    cap = std::min<uint64_t>(cap * 4, cap_max);
  }
  if (route == kFgWalk) return false;
  t->route = 2;
  return true;
}

// the whole call through the library's plan -> false: refused / failed; traces by uid
static bool call(const std::vector<Query>& qs, int route, uint32_t ef, uint64_t n_rows, uint32_t cap_max, const Lds& lds,
                 std::map<uint64_t, Trace>* traces) {
  traces->clear();
  std::vector<FiltersSlot> first;
  for (uint32_t i = 0; i < qs.size(); i++) {
    Trace& t = (*traces)[qs[i].uid];
    if (qs[i].matched == 0) continue;
    const FilterGraphPlan p = filter_graph_route(route, ef, qs[i].matched, n_rows, cap_max);
    if (p.route == kFgRefuse) return false;
    if (p.route == kFgExact) t.route = 2;
    else first.push_back(FiltersSlot{i, 0, p.cap, 0});
  }
  uint32_t expected_n = (uint32_t)first.size();
  std::vector<FiltersSlot> prev = first;  // what the coming round must consist of
  auto run = [&](const FiltersSlot* slots, uint32_t n, const FiltersLaunch* launches, uint32_t nl, unsigned char* over) -> int {
    expect(n == expected_n && n == prev.size(), "the round holds the queries that are due", n, expected_n);
    expect(nl >= 1 && nl <= 4, "at most four launches per round", nl);
    g_rounds++;
    g_split_rounds += nl > 1;
    g_reruns += n != first.size() || !(*traces)[qs[slots[0].query].uid].caps.empty();
    for (uint32_t l = 0; l < nl; l++) {  // a launch whose queries differ in logical capacity
      bool differ = false;
      for (uint32_t s = launches[l].begin; s < launches[l].begin + launches[l].count && s < n; s++) differ |= slots[s].cap != launches[l].cap;
      g_shared_rounds += differ;
    }
    // the launches partition [0, n) ...
    uint32_t at = 0;
    for (uint32_t l = 0; l < nl; l++) {
      const FiltersLaunch& L = launches[l];
      expect(L.begin == at && L.count > 0, "launches are contiguous and non-empty", L.begin, at);
      at += L.count;
      if (at > n) break;
      uint32_t mx = 0;
      for (uint32_t s = L.begin; s < L.begin + L.count; s++) {
        mx = std::max(mx, slots[s].cap);
        expect(slots[s].cap <= L.cap, "physical capacity >= logical", L.cap, slots[s].cap);
        expect(fg_per_cu(lds(slots[s].cap)) == L.per_cu, "a group is one class of walks per CU", L.per_cu, slots[s].cap);
      }
      expect(mx == L.cap, "physical capacity = the largest logical one of the group", L.cap, mx);
      expect(lds(L.cap) <= kFgLdsBudget, "the launch fits 160 KB of LDS", lds(L.cap));
      expect(fg_per_cu(lds(L.cap)) == L.per_cu && L.per_cu >= 1 && L.per_cu <= 4, "walks per CU of the launch", L.per_cu);
      for (uint32_t m = 0; m < l; m++) expect(launches[m].per_cu != L.per_cu, "one launch per class", L.per_cu);
    }
    expect(at == n, "the launches cover the round", at, n);
    // ... and the grouped slots are the round's queries, each once, with the capacity its own ladder says, in the round's order
    // inside a group
    std::vector<int> seen(qs.size(), 0);
    for (uint32_t s = 0; s < n; s++) {
      const uint32_t qi = slots[s].query;
      if (qi >= qs.size()) {
        expect(false, "a slot names a query of the call", qi);
        continue;
      }
      seen[qi]++;
      Trace& t = (*traces)[qs[qi].uid];
      Trace solo;
      alone(qs[qi], route, ef, n_rows, cap_max, &solo);
      expect(t.caps.size() < solo.caps.size() && solo.caps[t.caps.size()] == slots[s].cap, "logical capacity = the single-filter ladder's step",
             qi, slots[s].cap);
      t.caps.push_back(slots[s].cap);
      over[s] = slots[s].cap < qs[qi].thresh;
    }
    for (const FiltersSlot& p : prev) expect(seen[p.query] == 1, "every query of the round runs exactly once", p.query, (uint64_t)seen[p.query]);
    for (uint32_t l = 0; l < nl && launches[l].begin + launches[l].count <= n; l++) {  // stable: the order of `prev` inside a group
      size_t from = 0;
      for (uint32_t s = launches[l].begin; s < launches[l].begin + launches[l].count; s++) {
        while (from < prev.size() && prev[from].query != slots[s].query) from++;
        expect(from < prev.size(), "stable order inside a group", slots[s].query);
      }
    }
    // what the next round must be
    std::vector<FiltersSlot> next;
    for (uint32_t s = 0; s < n; s++)
      if (over[s] && slots[s].cap < cap_max) next.push_back(slots[s]);
      else if (!over[s] && slots[s].query < qs.size()) (*traces)[qs[slots[s].query].uid].route = 1;
    prev.swap(next);
    expected_n = (uint32_t)prev.size();
    return 0;
  };
  std::vector<FiltersSlot> left;
  const int rc = filters_walk_ladders(first, cap_max, lds, run, &left);
  expect(rc == 0 && prev.empty(), "the ladders end when nothing is due", (uint64_t)rc, prev.size());
  if (!left.empty() && route == kFgWalk) return false;
  for (const FiltersSlot& s : left) {
    expect(s.query < qs.size() && s.cap == cap_max, "a leftover query overflowed the largest list", s.query, s.cap);
    if (s.query < qs.size()) (*traces)[qs[s.query].uid].route = 2;
  }
  return true;
}

static void one_case(uint64_t seed) {
  g_cases++;
  uint64_t r = mix(seed);
  auto next = [&](uint64_t mod) -> uint64_t { r = mix(r); return mod ? r % mod : 0; };
  const uint32_t efs[] = {1, 10, 16, 64, 128, 300, 1000, 4000};
  const uint64_t rows[] = {1, 100, 3000, 65536, 1000000, 0xFFFFFE00ull};
  const uint32_t nbs[] = {64, 128, 256}, qbs[] = {0, 16, 160, 3072};
  const uint32_t ef = efs[next(8)];
  const uint64_t n_rows = rows[next(6)];
  const Lds lds{nbs[next(3)], qbs[next(4)]};
  uint32_t cap_max = (160 * 1024) / 9 / 64 * 64;  // the largest list of the launch, as the library finds it
  while (cap_max && lds(cap_max) > kFgLdsBudget) cap_max -= 64;
  const uint64_t ml = next(5);  // max_list: none, or something between a small list and the largest
  if (ml == 1) cap_max = std::min<uint32_t>(cap_max, 128 + (uint32_t)next(1024));
  if (ml == 2) cap_max = std::min<uint32_t>(cap_max, 1 + (uint32_t)next(cap_max));
  if (ml == 3) cap_max = std::min<uint32_t>(cap_max, 4096);
  const int route = (int)next(3);
  const uint32_t nq = 1 + (uint32_t)next(300);
  const uint32_t n_filters = 1 + (uint32_t)next(nq < 40 ? nq : 40);
  std::vector<uint64_t> sizes(n_filters);
  for (uint64_t& m : sizes) {
    const uint64_t kind = next(6);
    m = kind == 0 ? 0 : kind == 1 ? n_rows : kind == 2 ? std::min<uint64_t>(n_rows, ef ? ef - 1 + next(3) : 0) : kind == 3 ? n_rows / (1 + next(2000)) : next(n_rows + 1);
  }
  std::vector<Query> qs(nq);
  for (uint32_t i = 0; i < nq; i++) {
    qs[i].uid = seed * 1000 + i;
    qs[i].matched = sizes[next(n_filters)];
    const uint64_t kind = next(4);  // never overflows; overflows small lists; ... up to the largest; always
    qs[i].thresh = kind == 0 ? 0 : kind == 1 ? (uint32_t)next(2048) : kind == 2 ? (uint32_t)next((uint64_t)cap_max + 2) : 0xFFFFFFFFu;
  }
  std::map<uint64_t, Trace> whole, other;
  const bool ok = call(qs, route, ef, n_rows, cap_max, lds, &whole);
  // every query: what it gets alone — and the call fails exactly when one of its queries fails alone
  bool want_ok = true;
  for (const Query& q : qs) {
    Trace solo;
    const bool s = alone(q, route, ef, n_rows, cap_max, &solo);
    want_ok = want_ok && s;
    if (ok) expect(s && whole[q.uid] == solo, "a query of the call = the query alone", q.uid % 1000, solo.caps.size());
  }
  expect(ok == want_ok, "the call fails iff a query fails alone", ok, want_ok);
  g_failed += !ok;
  if (!ok) return;
  // permuted, and with some companions removed: every remaining query's plan is unchanged
  std::vector<Query> perm = qs;
  for (size_t i = perm.size(); i > 1; i--) std::swap(perm[i - 1], perm[next(i)]);
  expect(call(perm, route, ef, n_rows, cap_max, lds, &other), "the permuted call runs");
  for (const Query& q : qs) expect(other[q.uid] == whole[q.uid], "unchanged when the companions are permuted", q.uid % 1000);
  std::vector<Query> fewer;
  for (const Query& q : perm)
    if (next(3) != 0) fewer.push_back(q);
  if (fewer.empty()) fewer.push_back(perm[0]);
  expect(call(fewer, route, ef, n_rows, cap_max, lds, &other), "the reduced call runs");
  for (const Query& q : fewer) expect(other[q.uid] == whole[q.uid], "unchanged when companions are removed", q.uid % 1000);
}

// ---- every query on ONE filter: the one-filter call (vdb_hip_index_search_graph_filtered) is served by the per-query path ----
// What that call ran while it had a host loop of its own, transcribed: the first list plan.cap for every query; the overflowing
// queries again, in ascending query order, at min(4 * cap, cap_max); stop at cap_max; the exact pass for what is left.  Per attempt
// per_cu = min(4, max(1, 160 KB / lds)) walks per CU and slots = min(n, n_cus * per_cu) resident blocks.
struct Attempt {
  uint32_t cap, per_cu, slots;
  std::vector<uint32_t> queries;  // launch slot -> query
};
static bool single_filter_loop(uint64_t matched, const std::vector<uint32_t>& thresh, int route, uint32_t ef, uint64_t n_rows, uint32_t cap_max,
                               const Lds& lds, uint32_t n_cus, std::vector<Attempt>* attempts, std::vector<uint32_t>* exact) {
  attempts->clear();
  exact->clear();
  const uint32_t nq = (uint32_t)thresh.size();
  if (matched == 0) return true;
  const FilterGraphPlan plan = filter_graph_route(route, ef, matched, n_rows, cap_max);
  if (plan.route == kFgRefuse) return false;
  std::vector<uint32_t> left;
  bool all = true;
  if (plan.route == kFgWalk) {
    for (uint64_t cap = plan.cap;;) {
      const uint64_t bytes = lds((uint32_t)cap);
      if (bytes > 160 * 1024) return false;
      Attempt at{(uint32_t)cap, 0, 0, {}};
      if (all)
        for (uint32_t i = 0; i < nq; i++) at.queries.push_back(i);
      else
        at.queries = left;
      at.per_cu = (uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, (160 * 1024) / bytes));
      at.slots = (uint32_t)std::min<uint64_t>(at.queries.size(), (uint64_t)n_cus * at.per_cu);
      std::vector<uint32_t> over;
      for (uint32_t i : at.queries)
        if (cap < thresh[i]) over.push_back(i);
      attempts->push_back(at);
      left.swap(over);
      all = false;
      if (left.empty() || cap >= cap_max) break;
      cap = std::min<uint64_t>(cap * 4, cap_max);
    }
    if (!left.empty() && route == kFgWalk) return false;
  }
  if (all)
    for (uint32_t i = 0; i < nq; i++) exact->push_back(i);
  else
    *exact = left;
  return true;
}

static long g_one_cases = 0, g_one_rounds = 0, g_one_reruns = 0, g_one_exact_after_walk = 0, g_one_exact_calls = 0, g_one_failed = 0;
static void one_filter_case(uint64_t seed) {
  g_cases++;
  g_one_cases++;
  uint64_t r = mix(seed ^ 0x5EEDF00Dull);
  auto next = [&](uint64_t mod) -> uint64_t { r = mix(r); return mod ? r % mod : 0; };
  const uint32_t efs[] = {1, 10, 16, 64, 128, 300, 1000, 4000};
  const uint64_t rows[] = {1, 100, 3000, 65536, 1000000, 0xFFFFFE00ull};
  const uint32_t nbs[] = {64, 128, 256}, qbs[] = {0, 16, 160, 3072}, cus[] = {1, 8, 256};
  const uint32_t ef = efs[next(8)];
  const uint64_t n_rows = rows[next(6)];
  const Lds lds{nbs[next(3)], qbs[next(4)]};
  const uint32_t n_cus = cus[next(3)];
  uint32_t cap_max = (160 * 1024) / 9 / 64 * 64;
  while (cap_max && lds(cap_max) > kFgLdsBudget) cap_max -= 64;
  const uint64_t ml = next(5);
  if (ml == 1) cap_max = std::min<uint32_t>(cap_max, 128 + (uint32_t)next(1024));
  if (ml == 2) cap_max = std::min<uint32_t>(cap_max, 1 + (uint32_t)next(cap_max));
  if (ml == 3) cap_max = std::min<uint32_t>(cap_max, 4096);
  const int route = (int)next(3);
  const uint32_t nq = 1 + (uint32_t)next(300);
  const uint64_t kind = next(6);  // the one filter's size, as one_case draws them
  const uint64_t matched = kind == 0 ? 0 : kind == 1 ? n_rows : kind == 2 ? std::min<uint64_t>(n_rows, ef - 1 + next(3)) : kind == 3 ? n_rows / (1 + next(2000)) : next(n_rows + 1);
  std::vector<uint32_t> thresh(nq);
  for (uint32_t& t : thresh) {
    const uint64_t k = next(4);
    t = k == 0 ? 0 : k == 1 ? (uint32_t)next(2048) : k == 2 ? (uint32_t)next((uint64_t)cap_max + 2) : 0xFFFFFFFFu;
  }
  std::vector<Attempt> want;
  std::vector<uint32_t> want_exact;
  const bool want_ok = single_filter_loop(matched, thresh, route, ef, n_rows, cap_max, lds, n_cus, &want, &want_exact);

  // the per-query path with a table of that one filter and every query on it (search_graph_filters_to_device's plan loop)
  bool ok = true;
  std::vector<FiltersSlot> first, exact;
  for (uint32_t i = 0; i < nq && ok; i++) {
    if (matched == 0) continue;
    const FilterGraphPlan p = filter_graph_route(route, ef, matched, n_rows, cap_max);
    if (p.route == kFgRefuse) ok = false;
    else if (p.route == kFgWalk) first.push_back(FiltersSlot{i, 0, p.cap, 0});
    else exact.push_back(FiltersSlot{i, 0, 0, 0});
  }
  size_t round = 0;
  if (ok) {
    auto run = [&](const FiltersSlot* slots, uint32_t n, const FiltersLaunch* launches, uint32_t nl, unsigned char* over) -> int {
      g_one_rounds++;
      g_one_reruns += round > 0;
      const bool known = round < want.size();
      expect(known, "no more rounds than the one-filter loop made attempts", round, want.size());
      expect(nl == 1 && launches[0].begin == 0 && launches[0].count == n, "one launch per round", nl, n);
      if (known && nl >= 1) {
        const Attempt& at = want[round];
        expect(launches[0].cap == at.cap, "the launch's physical capacity = the attempt's list", launches[0].cap, at.cap);
        expect(launches[0].per_cu == at.per_cu, "walks per CU = the attempt's", launches[0].per_cu, at.per_cu);
        expect(std::min<uint64_t>(launches[0].count, (uint64_t)n_cus * launches[0].per_cu) == at.slots, "resident blocks = the attempt's", at.slots);
        expect(n == at.queries.size(), "the round holds the attempt's queries", n, at.queries.size());
        for (uint32_t s = 0; s < n && s < at.queries.size(); s++) {
          expect(slots[s].query == at.queries[s], "slot order = ascending query order of the attempt", slots[s].query, at.queries[s]);
          expect(slots[s].cap == at.cap && slots[s].filter == 0, "every slot on the one filter at the attempt's capacity", slots[s].cap, at.cap);
        }
      }
      for (uint32_t s = 0; s < n; s++) over[s] = slots[s].query < nq && slots[s].cap < thresh[slots[s].query];
      round++;
      return 0;
    };
    std::vector<FiltersSlot> left;
    const int rc = filters_walk_ladders(first, cap_max, lds, run, &left);
    expect(rc == 0, "the ladders run", (uint64_t)rc);
    if (!left.empty() && route == kFgWalk) ok = false;
    exact.insert(exact.end(), left.begin(), left.end());
    std::sort(exact.begin(), exact.end(), [](const FiltersSlot& x, const FiltersSlot& y) { return x.query < y.query; });
  }
  expect(ok == want_ok, "the call fails iff the one-filter loop fails", ok, want_ok);
  g_one_failed += !ok;
  if (!ok || !want_ok) return;
  expect(round == want.size(), "as many rounds as the one-filter loop made attempts", round, want.size());
  expect(exact.size() == want_exact.size(), "the exact pass takes the queries the one-filter loop left", exact.size(), want_exact.size());
  for (size_t i = 0; i < exact.size() && i < want_exact.size(); i++)
    expect(exact[i].query == want_exact[i], "the exact pass in the one-filter loop's order", exact[i].query, want_exact[i]);
  g_one_exact_after_walk += !want.empty() && !want_exact.empty();
  g_one_exact_calls += want.empty() && !want_exact.empty();
}

int main() {
  for (uint64_t seed = 1; seed <= 12000; seed++) one_case(seed);
  for (uint64_t seed = 1; seed <= 12000; seed++) one_filter_case(seed);
  // hand-computed points: the ladder ...
  expect(fg_ladder_next(384, 17984) == 1536 && fg_ladder_next(6144, 17984) == 17984 && fg_ladder_next(17984, 17984) == 0, "ladder steps");
  expect(fg_ladder_next(0xC0000000u, 0xFFFFFFFFu) == 0xFFFFFFFFu && fg_ladder_next(100, 100) == 0 && fg_ladder_next(200, 100) == 0, "ladder ends");
  // ... and the classes: 160 KB / lds, at most 4, at least 1
  expect(fg_per_cu(40 * 1024) == 4 && fg_per_cu(40 * 1024 + 16) == 3 && fg_per_cu(54 * 1024) == 2 && fg_per_cu(81 * 1024) == 1 &&
             fg_per_cu(160 * 1024) == 1 && fg_per_cu(16) == 4,
         "walks per CU");
  // (what the generated calls covered: rounds with more than one launch, launches whose queries differ in capacity, re-run rounds,
  // calls that fail as a whole)
  std::printf("{\"ok\": %s, \"cases\": %ld, \"checks\": %ld, \"violations\": %d, \"rounds\": %ld, \"split_rounds\": %ld, \"mixed_launches\": %ld, "
              "\"rerun_rounds\": %ld, \"failed_calls\": %ld, \"one_filter_cases\": %ld, \"one_filter_rounds\": %ld, \"one_filter_rerun_rounds\": %ld, "
              "\"one_filter_exact_after_walk\": %ld, \"one_filter_exact_calls\": %ld, \"one_filter_failed_calls\": %ld}\n",
              g_bad ? "false" : "true", g_cases, g_checks, g_bad, g_rounds, g_split_rounds, g_shared_rounds, g_reruns, g_failed, g_one_cases,
              g_one_rounds, g_one_reruns, g_one_exact_after_walk, g_one_exact_calls, g_one_failed);
  return g_bad ? 1 : 0;
}
