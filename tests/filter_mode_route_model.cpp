// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the route rule of a filtered
// exact call over the SQ8 / Binary / half images (filter_mode_route) at its boundaries, and the plan of its listed passes
// (mode_listed_plan).  tests/test_filtered_modes_cpu.py builds it with ASan + UBSan and reads the JSON line.
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
  const int kCosine = 0, kEuclid = kFmMetricEuclidean, kDot = 2, kHamming = 3;
  const int modes[] = {kFmModeSq8, kFmModeBinary, kFmModeBf16, kFmModeF16};
  const uint64_t sizes[] = {1, 3, 4, 5, 777, 65536, 1000000, 0xFFFFFE00ull};
  const uint32_t nqs[] = {1, 2, 5, 6, 8, 16, 64, 256, 1024};

  // which (mode, metric) has a listed kernel at all
  for (int me : {kCosine, kEuclid, kDot}) {
    expect(filter_mode_has_listed(kFmModeSq8, me), "SQ8 has a listed kernel for its three metrics");
    expect(!filter_mode_has_listed(kFmModeBinary, me), "Binary has none");
    expect(filter_mode_has_listed(kFmModeF16, me) == (me == kEuclid), "f16: Euclidean only");
    expect(filter_mode_has_listed(kFmModeBf16, me) == (me == kEuclid), "bf16: Euclidean only");
  }
  expect(!filter_mode_has_listed(1, kEuclid) && !filter_mode_has_listed(2, kEuclid) && !filter_mode_has_listed(0, kCosine), "other modes have none");

  for (uint64_t n : sizes) {
    for (uint32_t nq : nqs) {
      for (int mo : modes) {
        for (int me : {kCosine, kEuclid, kDot, kHamming}) {
          const bool has = filter_mode_has_listed(mo, me);
          for (int64_t opt = -1; opt <= 3; opt++) {
            expect(filter_mode_route(opt, mo, me, 0, n, nq, true) == kFilterRouteDense, "count = 0 is dense");
            expect(filter_mode_route(opt, mo, me, n / 8 + 1, n, nq, false) == kFilterRouteDense, "listed not available: dense");
            if (!has) expect(filter_mode_route(opt, mo, me, 1, n, nq, true) == kFilterRouteDense, "no listed kernel for the mode / metric: dense");
          }
          if (!has) continue;
          // forced routes
          for (uint64_t c : {(uint64_t)1, n / 2 + 1, n}) {
            expect(filter_mode_route(1, mo, me, c, n, nq, true) == kFilterRouteListed, "forced listed");
            expect(filter_mode_route(2, mo, me, c, n, nq, true) == kFilterRouteDense, "forced dense");
            expect(filter_mode_route(3, mo, me, c, n, nq, true) == kFilterRouteDense, "values above 2 are dense");
          }
          const bool sq8_batch = mo == kFmModeSq8 && nq > kFmSq8ListedMaxQueries;  // SQ8 beyond one-query passes: always mask substitution
          if (n >= 2) {  // (n = 1: the only non-empty filter holds every row ... and 4 <= 3 is false as well)
            expect(filter_mode_route(0, mo, me, n, n, nq, true) == kFilterRouteDense, "auto: every row allowed is dense");
            expect(filter_mode_route(-1, mo, me, n, n, nq, true) == kFilterRouteDense, "auto (< 0): every row allowed is dense");
          }
          if (sq8_batch) {
            for (uint64_t c : {(uint64_t)1, n / 100 + 1, n / 4, 3 * n / 4, n})
              if (c >= 1 && c <= n) expect(filter_mode_route(0, mo, me, c, n, nq, true) == kFilterRouteDense, "auto: SQ8 batches take mask substitution");
          } else {
            // the streaming rule: count <= 3/4 n, whatever nq
            const uint64_t c3 = 3 * n / 4;  // largest count with 4 count <= 3 n
            if (c3 >= 1) expect(filter_mode_route(0, mo, me, c3, n, nq, true) == kFilterRouteListed, "auto at count = 3 n / 4");
            if (c3 >= 2) expect(filter_mode_route(0, mo, me, c3 - 1, n, nq, true) == kFilterRouteListed, "auto just below 3 n / 4");
            if (c3 + 1 <= n) expect(filter_mode_route(0, mo, me, c3 + 1, n, nq, true) == kFilterRouteDense, "auto just above 3 n / 4");
            if (n >= 4) expect(filter_mode_route(0, mo, me, 1, n, nq, true) == kFilterRouteListed, "auto: one row is listed");
          }
        }
      }
      // the SQ8 cut in the batch size sits at kFmSq8ListedMaxQueries queries, one step either side; the half image has no such cut
      if (n >= 4) {
        for (int me : {kCosine, kEuclid, kDot}) {
          expect(filter_mode_route(0, kFmModeSq8, me, n / 2, n, kFmSq8ListedMaxQueries - 1, true) == kFilterRouteListed, "SQ8 below the batch cut");
          expect(filter_mode_route(0, kFmModeSq8, me, n / 2, n, kFmSq8ListedMaxQueries, true) == kFilterRouteListed, "SQ8 at the batch cut");
          expect(filter_mode_route(0, kFmModeSq8, me, n / 2, n, kFmSq8ListedMaxQueries + 1, true) == kFilterRouteDense, "SQ8 just above the batch cut");
        }
        expect(filter_mode_route(0, kFmModeF16, kEuclid, n / 2, n, kFmSq8ListedMaxQueries + 1, true) == kFilterRouteListed, "half Euclidean has no batch cut");
        expect(filter_mode_route(0, kFmModeBf16, kEuclid, n / 2, n, 1024, true) == kFilterRouteListed, "half Euclidean has no batch cut (1 024 queries)");
      }
    }
  }

  // ---- the plans ----
  const int n_cus = 256;
  for (bool half : {false, true}) {
    for (uint32_t dim : {1u, 17u, 100u, 768u, 1024u, 4096u}) {
      for (uint32_t k : {1u, 10u, 64u, 128u, 1000u}) {
        for (uint64_t count : {(uint64_t)1, (uint64_t)9, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)1000, (uint64_t)65537, (uint64_t)1000000, (uint64_t)0xFFFFFE00ull}) {
          for (uint32_t nq : {1u, 2u, 4u, 5u, 7u, 8u, 9u, 16u, 17u, 1024u}) {
            const ModeListedPlan p = mode_listed_plan(half, dim, k, count, nq, n_cus);
            const uint64_t lds1 = half ? fm_half_l2_lds_bytes(1, k, dim) : fm_sq8_lds_bytes(1, k, dim);
            expect((p.blocks > 0) == (lds1 <= kFmLdsBudget), "a plan exists iff one query fits the LDS");
            if (!p.blocks) continue;
            expect(p.lds <= kFmLdsBudget, "LDS within 160 KiB");
            expect(p.lds == (half ? fm_half_l2_lds_bytes(p.B, k, dim) : fm_sq8_lds_bytes(p.B, k, dim)), "lds is the class's footprint");
            expect(half ? (p.B == 16 || p.B == 4 || p.B == 1) : (p.B == 8 || p.B == 4 || p.B == 1), "a class the kernels are built for");
            expect(p.nq_pass >= 1 && p.nq_pass <= (uint32_t)p.B && p.nq_pass <= nq, "queries of the pass");
            const uint64_t rpg = half ? 64u / (uint64_t)p.B : 64u, ngroups = (count + rpg - 1) / rpg;
            expect((uint64_t)p.blocks * p.per_block >= ngroups, "the chunks cover the list");
            expect((uint64_t)(p.blocks - 1) * p.per_block < ngroups, "no block is empty");
            expect((uint64_t)p.blocks <= (uint64_t)n_cus * 4, "at most four resident blocks per CU");
            // the class follows the unlisted dispatch unless its LDS does not fit
            const int want = half ? (nq > 4 ? 16 : (nq > 1 ? 4 : 1)) : (nq >= 8 ? 8 : (nq >= 4 ? 4 : 1));
            const uint64_t lds_want = half ? fm_half_l2_lds_bytes(want, k, dim) : fm_sq8_lds_bytes(want, k, dim);
            if (lds_want <= kFmLdsBudget) expect(p.B == want, "the unlisted dispatch's class");
            else expect(p.B < want, "a smaller class when the LDS does not fit");
          }
        }
      }
    }
  }
  // nothing to do: no plan
  expect(mode_listed_plan(false, 768, 10, 0, 8, n_cus).blocks == 0, "count = 0");
  expect(mode_listed_plan(false, 768, 0, 100, 8, n_cus).blocks == 0, "k = 0");
  expect(mode_listed_plan(true, 768, 10, 100, 0, n_cus).blocks == 0, "nq = 0");
  // "listed not available" when not even one query fits: SQ8 at dim 40 000 (160 000 B of query alone), half at k = 20 480
  expect(mode_listed_plan(false, 40000, 10, 1000, 1, n_cus).blocks == 0, "SQ8: the query tile does not fit");
  expect(mode_listed_plan(true, 768, 20480, 1000, 1, n_cus).blocks == 0, "half: the k-list does not fit");
  expect(filter_mode_route(1, kFmModeSq8, kCosine, 1000, 100000, 1, mode_listed_plan(false, 40000, 10, 1000, 1, n_cus).blocks > 0) == kFilterRouteDense,
         "forced listed without a plan is dense");
  // the passes of a batch: 9 SQ8 queries = 8 + 1, 7 = 4 + 1 + 1 + 1, 17 = 8 + 8 + 1; 17 half queries = 16 + 1, 70 = 4 x 16 + 6
  auto passes = [&](bool half, uint32_t nq) {
    uint32_t n = 0;
    for (uint32_t q0 = 0; q0 < nq; n++) q0 += mode_listed_plan(half, 768, 10, 5000, nq - q0, n_cus).nq_pass;
    return n;
  };
  expect(passes(false, 9) == 2 && passes(false, 7) == 4 && passes(false, 17) == 3 && passes(true, 17) == 2 && passes(true, 70) == 5, "passes");

  std::printf("{\"ok\": %s, \"cases\": %d, \"violations\": %d}\n", g_bad ? "false" : "true", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
