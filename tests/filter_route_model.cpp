// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the route rule of a
// filtered exact call at its boundaries.  tests/test_filtered_cpu.py builds it with ASan + UBSan and reads the JSON line.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "vdb_filter_route.hpp"

using namespace vdb;

static int g_bad = 0, g_cases = 0;
static void expect(bool ok, const char* what) {
  g_cases++;
  if (!ok) {
    g_bad++;
    std::fprintf(stderr, "violation: %s\n", what);
  }
}

int main() {
  const uint64_t sizes[] = {1, 3, 4, 777, 65536, 1000000, 0xFFFFFE00ull};
  const uint32_t nqs[] = {1, 2, 8, 16, 64, 256, 1024};
  for (uint64_t n : sizes) {
    for (uint32_t nq : nqs) {
      // the empty filter and a metric without a listed kernel always take the mask route, whatever the option
      for (int64_t opt = -1; opt <= 2; opt++) {
        expect(filter_route(opt, true, 0, n, nq) == kFilterRouteDense, "count = 0 is dense");
        expect(filter_route(opt, false, n / 8, n, nq) == kFilterRouteDense, "no listed kernel: dense");
        expect(filter_route(opt, false, n, n, nq) == kFilterRouteDense, "no listed kernel: dense (all rows)");
      }
      // forced routes
      for (uint64_t c : {(uint64_t)1, n / 2 + 1, n}) {
        expect(filter_route(1, true, c, n, nq) == kFilterRouteListed, "forced listed");
        expect(filter_route(2, true, c, n, nq) == kFilterRouteDense, "forced dense");
      }
      // auto: count = n_rows is never listed (n_rows / 4 < n_rows for every n >= 1)
      expect(filter_route(0, true, n, n, nq) == kFilterRouteDense, "auto: every row allowed is dense");
      expect(filter_route(-1, true, n, n, nq) == kFilterRouteDense, "auto (< 0): every row allowed is dense");
      // auto at the two thresholds: count <= n / 4 and count * nq <= 8 n
      const uint64_t q = n / 4;
      if (q >= 1) {
        const bool second = q * nq <= 8 * n;
        expect((filter_route(0, true, q, n, nq) == kFilterRouteListed) == second, "auto at count = n / 4");
        expect(filter_route(0, true, q + 1, n, nq) == kFilterRouteDense, "auto just above n / 4");
        const uint64_t c2 = 8 * n / nq;  // largest count the second condition admits
        if (c2 >= 1 && c2 <= q) expect(filter_route(0, true, c2, n, nq) == kFilterRouteListed, "auto at count * nq = 8 n");
        if (c2 + 1 <= q) expect(filter_route(0, true, c2 + 1, n, nq) == kFilterRouteDense, "auto just above count * nq = 8 n");
      }
    }
    // one query: the second condition never binds below n / 4
    for (uint64_t c = 1; c <= n / 4 && c < 64; c++) expect(filter_route(0, true, c, n, 1) == kFilterRouteListed, "nq = 1 below n / 4");
    // nothing wraps at the per-index row limit with 1 024 queries (2^32 x 2^10 < 2^64)
    expect(filter_route(0, true, n / 4, n, 1024) == ((n / 4) >= 1 && (n / 4) * 1024 <= 8 * n ? kFilterRouteListed : kFilterRouteDense), "no wrap");
    // the selection stage is kept from 1/16 of the rows up
    expect(filter_keeps_selection(n, n), "all rows keep the selection stage");
    expect(filter_keeps_selection((n + 15) / 16, n), "1/16 keeps it");
    if (n >= 32) expect(!filter_keeps_selection(n / 16 - 1, n), "below 1/16 does not");
    expect(!filter_keeps_selection(0, n), "the empty filter does not");
  }
  std::printf("{\"ok\": %s, \"cases\": %d, \"violations\": %d}\n", g_bad ? "false" : "true", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
