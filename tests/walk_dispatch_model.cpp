// Stand-alone host program over velesdb_amd/csrc/vdb_walk_dispatch.hpp (the text the library compiles): the metric x chunks-per-lane
// dispatch of the graph-walk launches.  tests/test_walk_dispatch_cpu.py builds it with ASan + UBSan and reads the JSON line.  Every
// metric 0..4 (and two values that are no metric) at dims 1, 255, 256, 257, 512, 768, 1024, 1280 and 4096, through the project's
// dim -> CPL rule, for the three kinds of kernel family: the callable is called exactly once with the constants the hand-written
// ladders selected — written down below as a table, not computed the way the header computes them — or, in a family that refuses
// the packed-bit metrics, not at all.
#include <cstdint>
#include <cstdio>

#include "vdb_walk_dispatch.hpp"

using namespace vdb;

static int g_bad = 0;
static long g_cases = 0;
static void expect(bool ok, const char* what, long a, long b, long c) {
  if (!ok && g_bad++ < 50) std::fprintf(stderr, "violation: %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// sweep_cpl_for_dim (sweep.hip), restated: whole chunks of 256 dimensions per lane, one to four of them; 0 = the generic kernel
static int cpl_for_dim(uint32_t dim) {
  if (dim % 256 != 0) return 0;
  const int c = (int)(dim / 256);
  return (c >= 1 && c <= 4) ? c : 0;
}

// what a call site instantiates: kernel<M(), C()>
template <int METRIC, int CPL>
static int kernel_tag() {
  return METRIC * 10 + CPL;
}

constexpr int kRefusedTag = -1;
struct Seen {
  int calls = 0, metric = -1, cpl = -1, tag = -2;
};

template <BitMetrics BITS>
static Seen run(int metric, int cpl) {
  Seen s;
  s.tag = dispatch_metric_cpl<BITS, int>(metric, cpl, kRefusedTag, [&](auto M, auto C) {
    static_assert(M() >= 0 && M() <= 4 && C() >= 0 && C() <= 4, "constants out of range");
    static_assert(BITS == BitMetrics::kTaken || (M() != VDB_HAMMING && M() != VDB_JACCARD), "a family without the packed-bit metrics got one");
    static_assert((M() != VDB_HAMMING && M() != VDB_JACCARD) || C() == 0, "the packed-bit metrics only have the generic kernel");
    s.calls++;
    s.metric = M();
    s.cpl = C();
    return kernel_tag<M(), C()>();
  });
  return s;
}

// the hand-written ladders this replaced, as data.  Row: the metric given; column: the family.  {metric selected, takes the dim's CPL}
struct Want {
  int metric;    // -1: the launch is refused, nothing is called
  bool dim_cpl;  // false: CPL 0 whatever the dim
};
static Want want(BitMetrics bits, int metric) {
  // Cosine, Euclidean: themselves in every family
  if (metric == 0) return {0, true};
  if (metric == 1) return {1, true};
  switch (bits) {
    case BitMetrics::kTaken:  // switch (metric) { ... case kDot: cpl ladder; case kHamming: <kHamming, 0>; default: <kJaccard, 0> }
      if (metric == 2) return {2, true};
      if (metric == 3) return {3, false};
      return {4, false};
    case BitMetrics::kFallToDot:  // switch (metric) { case kCosine: ...; case kEuclidean: ...; default: kDot's cpl ladder }
      return {2, true};
    default:  // the filtered ladders: case kDot: cpl ladder; default: return hipErrorInvalidValue
      if (metric == 2) return {2, true};
      return {-1, false};
  }
}

int main() {
  const uint32_t dims[] = {1, 255, 256, 257, 512, 768, 1024, 1280, 4096};
  const int table[] = {0, 0, 1, 0, 2, 3, 4, 0, 0};  // the CPL of each: 256 -> 1, 512 -> 2, 768 -> 3, 1024 -> 4, everything else -> 0
  const int metrics[] = {0, 1, 2, 3, 4, 5, -1};
  const BitMetrics families[] = {BitMetrics::kTaken, BitMetrics::kFallToDot, BitMetrics::kRefused};
  for (size_t d = 0; d < sizeof(dims) / sizeof(dims[0]); d++) {
    const int cpl = cpl_for_dim(dims[d]);
    expect(cpl == table[d], "dim -> CPL", dims[d], cpl, table[d]);
    for (int metric : metrics) {
      for (BitMetrics bits : families) {
        g_cases++;
        const Seen s = bits == BitMetrics::kTaken        ? run<BitMetrics::kTaken>(metric, cpl)
                       : bits == BitMetrics::kFallToDot ? run<BitMetrics::kFallToDot>(metric, cpl)
                                                        : run<BitMetrics::kRefused>(metric, cpl);
        const Want w = want(bits, metric);
        if (w.metric < 0) {
          expect(s.calls == 0 && s.tag == kRefusedTag, "a refused launch called something", metric, (long)bits, s.calls);
          continue;
        }
        const int wcpl = w.dim_cpl ? table[d] : 0;
        expect(s.calls == 1, "not exactly one call", metric, (long)bits, s.calls);
        expect(s.metric == w.metric && s.cpl == wcpl, "wrong constants", metric * 100 + (long)dims[d], s.metric, s.cpl);
        expect(s.tag == w.metric * 10 + wcpl, "the callable's value did not come back", metric, s.tag, w.metric * 10 + wcpl);
      }
      // the metric alone (the walk that only has the generic kernel): the same metric, once
      g_cases++;
      int calls = 0;
      const int got = dispatch_metric<BitMetrics::kTaken, int>(metric, kRefusedTag, [&](auto M) {
        calls++;
        return (int)M();
      });
      expect(calls == 1 && got == want(BitMetrics::kTaken, metric).metric, "metric-only dispatch", metric, got, calls);
    }
    // the chunks alone
    g_cases++;
    int calls = 0;
    const int got = dispatch_cpl(cpl, [&](auto C) {
      calls++;
      return (int)C();
    });
    expect(calls == 1 && got == table[d], "CPL-only dispatch", dims[d], got, calls);
  }
  for (int b = 0; b < 2; b++) {
    g_cases++;
    int calls = 0;
    const bool got = dispatch_bool(b != 0, [&](auto B) {
      calls++;
      return (bool)B();
    });
    expect(calls == 1 && got == (b != 0), "two-way dispatch", b, got, calls);
  }
  std::printf("{\"ok\": %s, \"violations\": %d, \"cases\": %ld}\n", g_bad == 0 ? "true" : "false", g_bad, g_cases);
  return g_bad == 0 ? 0 : 1;
}
