// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the launch plan of the gathered
// four-bit tier (bits_gather_plan) at its boundaries.  tests/test_bits_gathered_cpu.py builds it with ASan + UBSan and reads
// the JSON line; with four arguments (k count nq n_cus) it prints that one plan instead.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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

int main(int argc, char** argv) {
  if (argc == 5) {
    const HalfGatherPlan p = bits_gather_plan((uint32_t)std::strtoul(argv[1], nullptr, 10), std::strtoull(argv[2], nullptr, 10),
                                              (uint32_t)std::strtoul(argv[3], nullptr, 10), std::atoi(argv[4]));
    std::printf("{\"blocks\": %d, \"tn\": %d, \"nq_chunk\": %u, \"qtiles\": %u, \"per_block\": %u, \"spans\": %u, \"lds\": %llu}\n", p.blocks, p.TN, p.nq_chunk,
                p.qtiles, p.per_block, p.spans, (unsigned long long)p.lds);
    return 0;
  }
  uint32_t first_k_16 = 0, first_k_none = 0;  // the first k whose lists do not fit the 128-query / the 16-query instance
  for (uint32_t k = 1; k < 5000 && !first_k_none; k++) {
    const HalfGatherPlan p = bits_gather_plan(k, 1000, 1024, 256);
    if (!first_k_16 && p.TN != 128) first_k_16 = k;
    if (p.blocks == 0) first_k_none = k;
  }
  expect(first_k_16 > 64 && first_k_none > first_k_16, "k = 64 fits the 128-query instance; the 16-query instance takes over before no plan is left");
  // the kernel's LDS: two slabs of (64 + TN) lines of 128 B | TN k-lists | counters, locks | three tiles' rows and bit counts
  expect(hg_lds_bytes(16, first_k_none - 1) <= kFmLdsBudget && hg_lds_bytes(16, first_k_none) > kFmLdsBudget, "the last k is the last whose 16 lists fit");
  const uint64_t counts[] = {1, 63, 64, 65, 3000, 100000, 1000000, 0xFFFFFFFFull};
  const uint32_t nqs[] = {1, 16, 17, 63, 64, 130, 1024, 1025, 5000};
  const uint32_t ks[] = {1, 10, 64, first_k_16 - 1, first_k_16, 500, first_k_none - 1, first_k_none, 4096};
  const int cus[] = {0, 1, 256};
  for (uint64_t count : counts)
    for (uint32_t nq : nqs)
      for (uint32_t k : ks)
        for (int n_cus : cus) {
          const HalfGatherPlan p = bits_gather_plan(k, count, nq, n_cus);
          if (k >= first_k_none) {
            expect(p.blocks == 0, "no plan past the k at which the lists of 16 queries overflow");
            continue;
          }
          const uint32_t chunk = nq < kHgMaxQueries ? nq : kHgMaxQueries;
          const uint64_t slabs = 2ull * (64 + (uint64_t)p.TN) * 128, ntiles = (count + 63) / 64;
          expect(p.blocks > 0 && p.lds <= 160 * 1024 && p.lds >= slabs + (uint64_t)p.TN * k * 8 + (uint64_t)p.TN * 8 + 3 * 64 * 8, "the kernel's LDS within 160 KiB");
          expect(p.nq_chunk == chunk && p.TN == ((chunk >= 64 && k < first_k_16) ? 128 : 16), "128-query tiles from 64 queries up while their lists fit");
          expect((uint64_t)p.qtiles * p.TN >= chunk && (uint64_t)(p.qtiles - 1) * p.TN < chunk, "the query tiles cover the chunk, none empty");
          expect(p.spans >= 1 && (uint64_t)p.spans * p.per_block >= ntiles && (uint64_t)(p.spans - 1) * p.per_block < ntiles,
                 "the spans cover the tiles, no block without a tile");
          expect((uint64_t)p.blocks == (uint64_t)p.spans * p.qtiles, "grid");
          expect((uint64_t)p.blocks <= (uint64_t)(n_cus > 0 ? n_cus : 1) * 4 || p.spans == 1, "at most the resident blocks of the chip");
          expect((uint64_t)chunk * p.spans * k * 8 <= kHgScratchCap || p.spans == 1, "partial keys within 256 MB");
        }
  expect(bits_gather_plan(0, 1000, 16, 256).blocks == 0 && bits_gather_plan(10, 0, 16, 256).blocks == 0 && bits_gather_plan(10, 1000, 0, 256).blocks == 0 &&
             bits_gather_plan(10, 0x100000000ull, 16, 256).blocks == 0,
         "no plan for zero k, count or nq, or a list past 2^32 - 1 rows");
  std::printf("{\"cases\": %d, \"failed_checks\": %d, \"first_k_16\": %u, \"first_k_none\": %u}\n", g_cases, g_bad, first_k_16, first_k_none);
  return g_bad ? 1 : 0;
}
