// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): the launch plan of the gathered
// matrix-core tier (half_gather_plan) at its boundaries.  tests/test_half_gathered_cpu.py builds it with ASan + UBSan and
// reads the JSON line; with five arguments (dim k count nq n_cus) it prints that one plan instead.
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
  if (argc == 6) {
    const HalfGatherPlan p = half_gather_plan((uint32_t)std::strtoul(argv[1], nullptr, 10), (uint32_t)std::strtoul(argv[2], nullptr, 10),
                                              std::strtoull(argv[3], nullptr, 10), (uint32_t)std::strtoul(argv[4], nullptr, 10), std::atoi(argv[5]));
    std::printf("{\"blocks\": %d, \"tn\": %d, \"nq_chunk\": %u, \"qtiles\": %u, \"per_block\": %u, \"spans\": %u, \"lds\": %llu}\n", p.blocks, p.TN, p.nq_chunk,
                p.qtiles, p.per_block, p.spans, (unsigned long long)p.lds);
    return 0;
  }
  const uint64_t counts[] = {1, 63, 64, 65, 3000, 100000, 1000000, 0xFFFFFE00ull, 0xFFFFFFFFull};
  const uint32_t nqs[] = {1, 16, 17, 63, 64, 130, 1024, 1025, 5000}, ks[] = {1, 10, 27, 64, 111, 112, 500, 1119, 1120, 4096};
  const int cus[] = {0, 1, 256};
  uint32_t first_k_128 = 0, first_k_none = 0;  // the first k whose lists do not fit the instance
  for (uint32_t k = 1; k < 5000 && !first_k_none; k++) {
    const HalfGatherPlan p = half_gather_plan(768, k, 1000, 1024, 256);
    if (!first_k_128 && p.TN != 128) first_k_128 = k;
    if (p.blocks == 0) first_k_none = k;
  }
  expect(first_k_128 > 64 && first_k_none > first_k_128, "k = 64 fits the 128-query instance; the 16-query instance takes over before no plan is left");
  for (uint64_t count : counts)
    for (uint32_t nq : nqs)
      for (uint32_t k : ks)
        for (int n_cus : cus) {
          const HalfGatherPlan p = half_gather_plan(768, k, count, nq, n_cus), q = half_gather_plan(7, k, count, nq, n_cus);
          expect(p.blocks == q.blocks && p.lds == q.lds && p.per_block == q.per_block && p.TN == q.TN, "nothing depends on dim");
          if (k >= first_k_none) {
            expect(p.blocks == 0, "lists that fit neither instance: no plan");
            continue;
          }
          expect(p.blocks > 0 && p.lds <= kFmLdsBudget && p.lds == hg_lds_bytes(p.TN, k), "a plan within 160 KiB");
          const uint32_t chunk = nq < kHgMaxQueries ? nq : kHgMaxQueries;
          expect(p.nq_chunk == chunk, "chunks of <= 1 024 queries");
          expect(p.TN == ((chunk >= 64 && k < first_k_128) ? 128 : 16), "128-query tiles from 64 queries up, 16 below and where the lists of 128 do not fit");
          expect((uint64_t)p.qtiles * p.TN >= chunk && (uint64_t)(p.qtiles - 1) * p.TN < chunk, "the query tiles cover the chunk, none empty");
          const uint64_t ntiles = (count + kHgTileRows - 1) / kHgTileRows;
          expect(p.spans >= 1 && (uint64_t)p.spans * p.per_block >= ntiles && (uint64_t)(p.spans - 1) * p.per_block < ntiles,
                 "the spans cover the list, no block without a tile");
          expect((uint64_t)p.blocks == (uint64_t)p.spans * p.qtiles && p.spans <= 65535u * 4u && p.qtiles <= 65535u, "grid bounds");
          expect((uint64_t)p.spans * p.qtiles <= (uint64_t)(n_cus > 0 ? n_cus : 1) * 4 || p.spans == 1, "at most the resident blocks of the chip");
          expect((uint64_t)chunk * p.spans * k * 8 <= kHgScratchCap || p.spans == 1, "partial keys within the scratch cap");
        }
  for (uint32_t z = 0; z < 3; z++)
    expect(half_gather_plan(768, z == 0 ? 0 : 10, z == 1 ? 0 : 1000, z == 2 ? 0 : 16, 256).blocks == 0, "no plan for zero k, count or nq");
  expect(half_gather_plan(768, 10, 0x100000000ull, 16, 256).blocks == 0, "a list past 2^32 - 1 rows has no plan");
  expect(filter_route_opt(3) == 0 && filter_route_opt(0) == 0 && filter_route_opt(1) == 1 && filter_route_opt(2) == 2 && filter_route_opt(-1) == -1,
         "value 3 is auto to the existing route functions");
  std::printf("{\"cases\": %d, \"failed_checks\": %d, \"first_k_16\": %u, \"first_k_none\": %u}\n", g_cases, g_bad, first_k_128, first_k_none);
  return g_bad ? 1 : 0;
}
