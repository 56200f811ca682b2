// hybrid_filters_plan_model.cpp — fused_phases_plan (velesdb_amd/csrc/vdb_filter_route.hpp) walked over its boundaries on
// the host: which unit goes to which phase, each phase's list length, the per-unit record limit with the unit's OWN list length, the
// largest unit of each launch.  A stand-alone program (built with ASan + UBSan by tests/test_hybrid_filters_cpu.py); the last line of
// its output is one JSON record.  Every expectation below is worked out here from the contract, not taken from the function.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "vdb_filter_route.hpp"

using namespace vdb;

static uint64_t g_cases = 0, g_violations = 0, g_over = 0, g_empty_phase = 0, g_mixed = 0;
#define HOLD(cond)                                                  \
  do {                                                              \
    if (!(cond)) {                                                  \
      g_violations++;                                               \
      fprintf(stderr, "violated at line %d: %s\n", __LINE__, #cond); \
    }                                                               \
  } while (0)

constexpr uint64_t kLimit = 8192;  // VDB_HYBRID_MAX_RECORDS = VDB_FUSE_MAX_RECORDS

// the hybrid call: one list per query, text_n further records
static void hybrid_case(const std::vector<uint32_t>& fq, uint32_t n_filters, uint32_t k, const std::vector<uint32_t>& text_n) {
  g_cases++;
  const uint32_t nq = (uint32_t)fq.size();
  const uint64_t len_un = (uint64_t)k * 2, len_fl = std::max<uint64_t>((uint64_t)k * 4, (uint64_t)k + 10);
  HOLD(hybrid_list_len(k, false) == len_un && hybrid_list_len(k, true) == len_fl);
  const FusedPhasesPlan p = fused_phases_plan(
      fq.data(), nq, n_filters, hybrid_list_len(k, false), hybrid_list_len(k, true), kLimit, [](uint32_t) { return 1u; },
      [&](uint32_t i) { return text_n[i]; });
  HOLD(p.phase[kPhaseUnfiltered].list_len == len_un && p.phase[kPhaseFiltered].list_len == len_fl);
  // the partition: every query once, in its phase, ascending
  std::vector<int> seen(nq, 0);
  int64_t first_over = -1;
  uint64_t most[2] = {0, 0};
  size_t count[2] = {0, 0};
  for (uint32_t i = 0; i < nq; i++) {
    const int ph = fq[i] == n_filters ? kPhaseUnfiltered : kPhaseFiltered;
    const uint64_t rec = (ph == kPhaseFiltered ? len_fl : len_un) + text_n[i];
    most[ph] = std::max(most[ph], rec);
    count[ph]++;
    if (rec > kLimit && first_over < 0) first_over = i;
  }
  for (int ph = 0; ph < 2; ph++) {
    const FusedPhase& P = p.phase[ph];
    HOLD(P.units.size() == count[ph] && P.lists == count[ph]);
    HOLD(std::is_sorted(P.units.begin(), P.units.end()));
    for (uint32_t u : P.units) {
      HOLD(u < nq);
      if (u < nq) {
        seen[u]++;
        HOLD((fq[u] == n_filters) == (ph == kPhaseUnfiltered));
      }
    }
    HOLD(P.most == most[ph]);
    if (P.units.empty()) {
      HOLD(P.most == 0);
      g_empty_phase++;
    }
  }
  for (uint32_t i = 0; i < nq; i++) HOLD(seen[i] == 1);
  HOLD(p.over == first_over);
  if (first_over >= 0) {
    g_over++;
    const bool fl = fq[first_over] != n_filters;
    HOLD(p.over_phase == (fl ? kPhaseFiltered : kPhaseUnfiltered));
    HOLD(p.over_records == (fl ? len_fl : len_un) + text_n[first_over]);
  }
  if (count[0] && count[1]) g_mixed++;
}

// the multi-query call: group_sizes lists per group, one list length for both phases, no further records
static void multi_case(const std::vector<uint32_t>& fg, uint32_t n_filters, uint64_t kf, const std::vector<uint32_t>& sizes) {
  g_cases++;
  const uint32_t ng = (uint32_t)fg.size();
  const FusedPhasesPlan p = fused_phases_plan(
      fg.data(), ng, n_filters, kf, kf, kLimit, [&](uint32_t g) { return sizes[g]; }, [](uint32_t) { return 0u; });
  uint64_t lists[2] = {0, 0}, most[2] = {0, 0};
  int64_t first_over = -1;
  for (uint32_t g = 0; g < ng; g++) {
    const int ph = fg[g] == n_filters ? kPhaseUnfiltered : kPhaseFiltered;
    lists[ph] += sizes[g];
    most[ph] = std::max(most[ph], (uint64_t)sizes[g] * kf);
    if ((uint64_t)sizes[g] * kf > kLimit && first_over < 0) first_over = g;
  }
  for (int ph = 0; ph < 2; ph++) {
    HOLD(p.phase[ph].list_len == kf && p.phase[ph].lists == lists[ph] && p.phase[ph].most == most[ph]);
    HOLD(std::is_sorted(p.phase[ph].units.begin(), p.phase[ph].units.end()));
  }
  HOLD(p.phase[0].units.size() + p.phase[1].units.size() == ng);
  HOLD(p.over == first_over);
  if (first_over >= 0) g_over++;
}

int main() {
  const uint32_t ks[] = {0, 1, 2, 3, 10, 11, 75, 2047, 2048, 2049, 4095, 4096, 4097, 0xFFFFFFFFu};
  // nq 0 and 1, all-unfiltered, all-filtered and mixed tables (n_filters 0: only "no filter" exists)
  for (uint32_t k : ks) {
    hybrid_case({}, 0, k, {});
    hybrid_case({}, 3, k, {});
    for (uint32_t tn : {0u, 1u, 10u, 8192u}) {
      hybrid_case({0}, 0, k, {tn});  // (n_filters = 0: value 0 = no filter)
      hybrid_case({2}, 2, k, {tn});
      hybrid_case({0}, 2, k, {tn});
      hybrid_case({1}, 2, k, {tn});
    }
    hybrid_case({3, 3, 3, 3}, 3, k, {0, 5, 9, 2});
    hybrid_case({0, 1, 2, 0}, 3, k, {0, 5, 9, 2});
    hybrid_case({3, 0, 1, 0, 2, 3}, 3, k, {1, 2, 3, 4, 5, 6});   // the table of the GPU test: none, A, B, A, empty, none
    hybrid_case({0, 1, 3, 3}, 3, k, {1, 2, 3, 4});               // the unfiltered queries behind the filtered ones
  }
  // the 8192-record limit, phase by phase.  k = 2048: unfiltered 4096 + text, filtered 8192 + text.
  {
    // legal unfiltered (4096 + 4096 = 8192), not legal filtered (8192 + 4096)
    const FusedPhasesPlan a = fused_phases_plan((const uint32_t*)std::vector<uint32_t>{1}.data(), 1, 1, hybrid_list_len(2048, false),
                                                hybrid_list_len(2048, true), kLimit, [](uint32_t) { return 1u; }, [](uint32_t) { return 4096u; });
    HOLD(a.over < 0 && a.phase[kPhaseUnfiltered].most == 8192);
    const FusedPhasesPlan b = fused_phases_plan((const uint32_t*)std::vector<uint32_t>{0}.data(), 1, 1, hybrid_list_len(2048, false),
                                                hybrid_list_len(2048, true), kLimit, [](uint32_t) { return 1u; }, [](uint32_t) { return 4096u; });
    HOLD(b.over == 0 && b.over_phase == kPhaseFiltered && b.over_records == 8192 + 4096);
    // the same two queries in one call: the unfiltered one in front is legal, the call is refused for the filtered one
    hybrid_case({1, 0}, 1, 2048, {4096, 4096});
    const std::vector<uint32_t> fq = {1, 0}, tn = {4096, 4096};
    const FusedPhasesPlan c = fused_phases_plan(fq.data(), 2, 1, hybrid_list_len(2048, false), hybrid_list_len(2048, true), kLimit,
                                                [](uint32_t) { return 1u; }, [&](uint32_t i) { return tn[i]; });
    HOLD(c.over == 1 && c.over_phase == kPhaseFiltered);
    // exactly at the limit and one past it, either kind
    hybrid_case({1}, 1, 4096, {0});   // 2k = 8192: legal
    hybrid_case({1}, 1, 4096, {1});   // 8193
    hybrid_case({0}, 1, 2048, {0});   // 4k = 8192: legal
    hybrid_case({0}, 1, 2048, {1});
    hybrid_case({0}, 1, 4096, {0});   // 4k = 16384
    const FusedPhasesPlan d = fused_phases_plan((const uint32_t*)std::vector<uint32_t>{1}.data(), 1, 1, hybrid_list_len(4096, false),
                                                hybrid_list_len(4096, true), kLimit, [](uint32_t) { return 1u; }, [](uint32_t) { return 0u; });
    HOLD(d.over < 0 && d.phase[kPhaseUnfiltered].most == 8192 && d.phase[kPhaseFiltered].units.empty());
    // a product past 32 bits is seen, not wrapped
    HOLD(hybrid_list_len(0xFFFFFFFFu, true) == 4ull * 0xFFFFFFFFull && hybrid_list_len(0xFFFFFFFFu, false) == 2ull * 0xFFFFFFFFull);
    HOLD(hybrid_list_len(0, true) == 10 && hybrid_list_len(0, false) == 0 && hybrid_list_len(3, true) == 13 && hybrid_list_len(4, true) == 16);
  }
  // generated tables
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint32_t n) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)(s % n);
  };
  for (int it = 0; it < 4000; it++) {
    const uint32_t nq = rnd(40), n_filters = rnd(5), k = ks[rnd(13)];
    const int kind = (int)rnd(3);  // 0: all unfiltered, 1: all filtered (when a filter exists), 2: mixed
    std::vector<uint32_t> fq(nq), tn(nq);
    for (uint32_t i = 0; i < nq; i++) {
      fq[i] = kind == 0 || n_filters == 0 ? n_filters : (kind == 1 ? rnd(n_filters) : rnd(n_filters + 1));
      tn[i] = rnd(8) == 0 ? 8192u - rnd(3) : rnd(300);
    }
    hybrid_case(fq, n_filters, k, tn);
    std::vector<uint32_t> sizes(nq);
    for (uint32_t i = 0; i < nq; i++) sizes[i] = 1 + rnd(10);
    const uint64_t kfs[] = {0, 20, 200, 500, 819, 820, 8192, 8193};
    multi_case(fq, n_filters, kfs[rnd(8)], sizes);
  }
  const bool ok = g_violations == 0;
  printf("{\"ok\": %s, \"cases\": %llu, \"violations\": %llu, \"over\": %llu, \"empty_phases\": %llu, \"mixed\": %llu}\n", ok ? "true" : "false",
         (unsigned long long)g_cases, (unsigned long long)g_violations, (unsigned long long)g_over, (unsigned long long)g_empty_phase,
         (unsigned long long)g_mixed);
  return ok ? 0 : 1;
}
