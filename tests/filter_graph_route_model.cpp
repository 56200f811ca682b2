// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the route rule of a
// filtered GRAPH call (filter_graph_route) at its boundaries.  tests/test_filtered_graph_cpu.py builds it with ASan + UBSan and
// reads the JSON line.  The expectations restate the rule of include/velesdb_hip.h with 128-bit arithmetic of their own.
#include <cstdint>
#include <cstdio>

#include "vdb_filter_route.hpp"

using namespace vdb;

static int g_bad = 0, g_cases = 0;
static void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) {
  g_cases++;
  if (!ok) {
    g_bad++;
    std::fprintf(stderr, "violation: %s (ef %llu matched %llu rows %llu cap_max %llu)\n", what, (unsigned long long)a,
                 (unsigned long long)b, (unsigned long long)c, (unsigned long long)d);
  }
}

typedef unsigned __int128 u128;
static u128 r64(u128 v) { return (v + 63) / 64 * 64; }
static u128 want_min(uint32_t ef) { return r64((u128)ef + (ef / 2 > 64 ? ef / 2 : 64)); }
static u128 want_sized(uint32_t ef, uint64_t m, uint64_t n) {  // 64-rounded(2 ef n / m + 64), never below the unfiltered walk's list
  const u128 s = r64((u128)2 * ef * n / m + 64);
  return s > want_min(ef) ? s : want_min(ef);
}

static void check(uint32_t ef, uint64_t m, uint64_t n, uint32_t cap_max) {
  const FilterGraphPlan ex = filter_graph_route(kFgExact, ef, m, n, cap_max);
  expect(ex.route == kFgExact, "route 2 is always the exact pass", ef, m, n, cap_max);
  const FilterGraphPlan au = filter_graph_route(kFgAuto, ef, m, n, cap_max);
  const FilterGraphPlan wk = filter_graph_route(kFgWalk, ef, m, n, cap_max);
  if (m == 0) {
    expect(au.route == kFgExact && wk.route == kFgExact, "the empty filter never walks", ef, m, n, cap_max);
    return;
  }
  const u128 sized = want_sized(ef, m, n), mn = want_min(ef);
  // auto: exact when the walk could never fill its results, or when the density-sized list exceeds the largest list
  const bool exact = m < ef || sized > cap_max;
  expect((au.route == kFgExact) == exact && (au.route == kFgWalk) == !exact, "auto route", ef, m, n, cap_max);
  if (!exact) {
    expect(au.cap == (uint32_t)sized && (u128)au.cap == sized, "auto: first list = the density-sized one", ef, m, n, cap_max);
    expect(au.cap % 64 == 0 && au.cap >= mn && au.cap <= cap_max, "auto: 64-rounded, >= the unfiltered list, <= cap_max", ef, m, n, cap_max);
  }
  // walk: refused only when not even the unfiltered walk's list fits; otherwise the sized list clamped to the largest
  if (mn > cap_max) {
    expect(wk.route == kFgRefuse, "walk: refused below the minimum list", ef, m, n, cap_max);
  } else {
    expect(wk.route == kFgWalk, "walk: walks", ef, m, n, cap_max);
    expect((u128)wk.cap == (sized < cap_max ? sized : (u128)cap_max), "walk: first list", ef, m, n, cap_max);
    expect(wk.cap >= mn || wk.cap == cap_max, "walk: never below the unfiltered list", ef, m, n, cap_max);
  }
}

int main() {
  const uint64_t sizes[] = {1, 2, 100, 777, 3000, 65536, 1000000, 0xFFFFFE00ull};  // ... up to the per-index row limit 2^32 - 512
  const uint32_t efs[] = {1, 10, 16, 63, 64, 65, 128, 129, 300, 1000, 17000, 20000, 0x7FFFFFFFu, 0xFFFFFFFFu};
  const uint32_t caps[] = {0, 1, 63, 64, 127, 128, 192, 1344, 4096, 17984, 18112, 0xFFFFFFFFu};  // (17 984: 160 KB at nbmax 64, 768 dims)
  for (uint64_t n : sizes)
    for (uint32_t ef : efs)
      for (uint32_t cap_max : caps) {
        // matched = 0, ef - 1, ef, n and what lies around them
        const uint64_t ms[] = {0, 1, ef > 1 ? (uint64_t)ef - 1 : 1, ef, (uint64_t)ef + 1, n / 1024, n / 100, n / 10, n / 2, n > 1 ? n - 1 : 1, n};
        for (uint64_t m : ms)
          if (m <= n) check(ef, m, n, cap_max);
        // the density at which the sized list crosses cap_max: the smallest matched whose list still fits, and one below it
        if (cap_max >= 128 && ef <= cap_max) {
          uint64_t lo = 1, hi = n;  // smallest m in [1, n] with sized(m) <= cap_max (sized falls as m grows)
          if (want_sized(ef, n, n) <= cap_max) {
            while (lo < hi) {
              const uint64_t mid = lo + (hi - lo) / 2;
              if (want_sized(ef, mid, n) <= cap_max) hi = mid; else lo = mid + 1;
            }
            check(ef, lo, n, cap_max);
            if (lo > 1) check(ef, lo - 1, n, cap_max);
            if (lo >= ef) expect(filter_graph_route(kFgAuto, ef, lo, n, cap_max).route == kFgWalk, "crossing: fits => walk", ef, lo, n, cap_max);
            if (lo > 1 && lo - 1 >= ef)
              expect(filter_graph_route(kFgAuto, ef, lo - 1, n, cap_max).route == kFgExact, "crossing: one row fewer => exact", ef, lo - 1, n, cap_max);
          }
        }
      }
  // 64-rounding at hand-computed points: ef 64, 3 000 rows, 300 matched: 2 * 64 * 10 + 64 = 1 344 (a multiple of 64 already);
  // ef 16, 1 200 rows, 120 matched: 384; ef 10, 1 000 rows, 333 matched: 2 * 10 * 1000 / 333 = 60, + 64 = 124 -> 128 (= the minimum list too)
  expect(filter_graph_route(kFgAuto, 64, 300, 3000, 17984).cap == 1344, "sized list 1 344");
  expect(filter_graph_route(kFgAuto, 16, 120, 1200, 17984).cap == 384, "sized list 384");
  expect(filter_graph_route(kFgAuto, 10, 333, 1000, 17984).cap == 128, "sized list 128");
  expect(filter_graph_route(kFgAuto, 64, 300, 3000, 1343).route == kFgExact, "max_list one below the sized list: exact");
  expect(filter_graph_route(kFgWalk, 64, 300, 3000, 1343).cap == 1343, "walk route starts at max_list");
  expect(filter_graph_route(kFgWalk, 64, 300, 3000, 127).route == kFgRefuse, "max_list below the minimum list (128): refused");
  expect(filter_graph_route(kFgAuto, 64, 300, 3000, 127).route == kFgExact, "... and auto answers exactly");
  // every row allowed: the unfiltered walk's list or the sized one, whichever is larger: ef 128 -> max(192, 2 * 128 + 64 = 320)
  expect(filter_graph_route(kFgAuto, 128, 1000000, 1000000, 17984).cap == 320, "all rows: 320");
  std::printf("{\"ok\": %s, \"cases\": %d, \"violations\": %d}\n", g_bad ? "false" : "true", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
