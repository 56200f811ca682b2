// Stand-alone host program over velesdb_amd/csrc/vdb_filter_route.hpp (the text the library compiles): mode_listed_plan, the plan of
// one pass of a listed sweep over the SQ8 codes or a half image, at the shapes of tests/test_gpu_large_dim_filters_modes.py.
// tests/test_large_dim_filters_modes_shapes_cpu.py builds it with ASan + UBSan, passes the cases as arguments
// ("sq8:dim:k:nq:count:n_cus" or "half:..."), and holds the JSON line to the literal tables of the GPU file: B, nq_pass, lds and
// blocks of every case, and the footprint of every class (fm_sq8_lds_bytes / fm_half_l2_lds_bytes).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vdb_filter_route.hpp"

using namespace vdb;

int main(int argc, char** argv) {
  std::printf("[");
  for (int i = 1; i < argc; i++) {
    char mode[8] = {0};
    unsigned long dim = 0, k = 0, nq = 0, count = 0, n_cus = 0;
    if (std::sscanf(argv[i], "%7[a-z0-9]:%lu:%lu:%lu:%lu:%lu", mode, &dim, &k, &nq, &count, &n_cus) != 6 ||
        (std::strcmp(mode, "sq8") != 0 && std::strcmp(mode, "half") != 0)) {
      std::fprintf(stderr, "bad case: %s\n", argv[i]);
      return 2;
    }
    const bool half = std::strcmp(mode, "half") == 0;
    const ModeListedPlan p = mode_listed_plan(half, (uint32_t)dim, (uint32_t)k, (uint64_t)count, (uint32_t)nq, (int)n_cus);
    const int wide = half ? 16 : 8;
    auto lds_of = [&](int b) { return (unsigned long long)(half ? fm_half_l2_lds_bytes(b, (uint32_t)k, (uint32_t)dim) : fm_sq8_lds_bytes(b, (uint32_t)k, (uint32_t)dim)); };
    std::printf("%s{\"mode\": \"%s\", \"dim\": %lu, \"k\": %lu, \"nq\": %lu, \"count\": %lu, \"n_cus\": %lu, \"B\": %d, \"nq_pass\": %u, \"lds\": %llu, "
                "\"blocks\": %d, \"per_block\": %u, \"lds_wide\": %llu, \"lds_4\": %llu, \"lds_1\": %llu, \"budget\": %llu}",
                i > 1 ? ", " : "", mode, dim, k, nq, count, n_cus, p.B, p.nq_pass, (unsigned long long)p.lds, p.blocks, p.per_block, lds_of(wide),
                lds_of(4), lds_of(1), (unsigned long long)kFmLdsBudget);
  }
  std::printf("]\n");
  return 0;
}
