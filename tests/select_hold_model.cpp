// select_hold_model.cpp — the selection stage's park-after-failure state machine (velesdb_amd/csrc/vdb_select_hold.hpp, the text the
// library compiles) run on the CPU.  Test infrastructure (tests/test_select_hold_cpu.py); no GPU, no HIP.
//
// The model restates what index.hip asks and in which order, for a handle whose shapes every selector is eligible for (n >= 65 536,
// dim % 64 == 0, dim >= 128, a batch of 32 queries, the default selector level 3):
//   * brute_dev (f32 rows): select_level_wide first; then, Cosine / DotProduct with k <= 10, select_level (2, or 1 while held); then,
//     Euclidean with k <= 10, select_level_l2 (2, or 0 while held); else the exact kernels (0);
//   * brute_mode_dev (SQ8 storage mode, Cosine / DotProduct): select_level_wide first; then, k <= 10, select_level_sq8 (3, or 0).
// A selection batch posts {unproven, queries, sequence, level} when it ends — level 4 for WIDE, 2 / 1 for the Cosine levels, 5 for
// Euclidean level 2, 3 for SQ8; the exact kernels post nothing — and the model has it arrive before the next call (the GPU test of the
// same traces, tests/test_gpu_dev_sequences.py test_hold_trace_with_a_sync_per_call, synchronises after every call).
//
// Output: one JSON line with the level traces of four configurations over data that defeats every selection (every query of every
// batch unproven), and the number of failed checks of the rules below.
#include <cstdio>

#include "vdb_select_hold.hpp"

using namespace vdb;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #cond); \
      g_fail++;                                                            \
    }                                                                      \
  } while (0)

struct Handle {
  SelectHolds holds;
  volatile uint32_t stats[4] = {0, 0, 0, 0};  // what select_finish_kernel writes
  uint32_t seq = 0;
  // one ask in a search call of its own
  bool ask(SelectHold& hold) { return hold.ask(stats, ++holds.call); }
  void post(uint32_t unproven, uint32_t queries, uint32_t level) {
    stats[0] = unproven;
    stats[1] = queries;
    stats[3] = level;
    stats[2] = ++seq;
  }
};

enum Config { kCosine, kEuclidean, kSq8 };

// one call of 32 queries: the level that answers (vdb_hip_index_last_select_level) and the verdict level its batch posts (0: none).
// The ladder asks per chunk: a selection tier takes the whole batch, and so do the exact tiers of Cosine / DotProduct and the SQ8
// sweep; a Euclidean batch below 64 queries goes to the vector-ALU sweep 8 queries at a time, and the rules are asked again for the
// 24 and the 16 that remain (not for the last 8: below kSelectMinQueries).
static int one_call(Handle& h, Config c, uint32_t k, uint32_t* posts) {
  const bool small_k = k <= 10;  // kGemmBf16MaxK: the block-local lists of levels 1 / 2 / 3 / Euclidean 2
  const uint64_t call = ++h.holds.call;
  int level = 0;
  for (uint32_t rest = 32; rest > 0;) {
    int took = 0;
    if (rest >= 16) {
      if (!h.holds.wide.ask(h.stats, call)) {
        took = 4;
      } else if (c == kCosine && small_k) {
        took = h.holds.sel16.ask(h.stats, call) ? 1 : 2;
      } else if (c == kEuclidean && small_k) {
        took = h.holds.l2.ask(h.stats, call) ? 0 : 2;
      } else if (c == kSq8 && small_k) {
        took = h.holds.sq8.ask(h.stats, call) ? 0 : 3;
      }
    }
    if (took) level = took;
    rest -= (took == 0 && c == kEuclidean) ? 8 : rest;
  }
  *posts = level == 0 ? 0u : (c == kEuclidean && level == 2 ? 5u : (uint32_t)level);
  return level;
}

static void trace(const char* name, Config c, uint32_t k, int calls, bool last) {
  Handle h;
  std::printf("\"%s\": [", name);
  for (int i = 0; i < calls; i++) {
    uint32_t posts = 0;
    const int level = one_call(h, c, k, &posts);
    if (posts) h.post(32, 32, posts);  // the data defeats every selection: all 32 queries unproven
    std::printf("%s%d", i ? ", " : "", level);
  }
  std::printf("]%s", last ? "" : ", ");
}

int main() {
  // (1) a verdict at or below 1/16 unproven starts no hold; one query more does
  {
    Handle h;
    h.post(2, 32, 4);
    CHECK(!h.ask(h.holds.wide) && h.holds.wide.left == 0 && h.holds.wide.seen == 1);
    h.post(0, 32, 4);
    CHECK(!h.ask(h.holds.wide));
    h.post(3, 32, 4);
    CHECK(h.ask(h.holds.wide) && h.holds.wide.left == kSelectHoldBatches - 1);
  }
  // (2) a verdict posted by another level starts none — and the selector it belongs to still sees it afterwards
  {
    Handle h;
    h.post(32, 32, 2);
    CHECK(!h.ask(h.holds.wide) && !h.ask(h.holds.l2) && !h.ask(h.holds.sq8));
    CHECK(h.ask(h.holds.sel16) && h.holds.sel16.left == kSelectHoldBatches - 1);
    h.post(32, 32, 5);
    CHECK(!h.ask(h.holds.wide) && h.ask(h.holds.l2));
    h.post(32, 32, 3);
    CHECK(!h.ask(h.holds.wide) && h.ask(h.holds.sq8));
  }
  // (3) a stale sequence number is ignored: the verdict that started a hold does not start it again, whatever the counts say now;
  // a hold lasts `length` batches, and no pinned block at all (no selection batch so far) starts nothing
  {
    Handle h;
    h.post(32, 32, 4);
    for (uint32_t i = 0; i < kSelectHoldBatches; i++) CHECK(h.ask(h.holds.wide));
    CHECK(!h.ask(h.holds.wide) && h.holds.wide.left == 0);
    h.stats[0] = 32;  // (same sequence number)
    CHECK(!h.ask(h.holds.wide));
    SelectHold fresh{4u};
    CHECK(!fresh.ask(nullptr, 1));
    // a verdict that arrives during a hold restarts it
    h.post(32, 32, 4);
    CHECK(h.ask(h.holds.wide));
    h.post(32, 32, 4);
    CHECK(h.ask(h.holds.wide) && h.holds.wide.left == kSelectHoldBatches - 1);
    // a filtered call's copy-and-restore leaves no trace
    const SelectHolds saved = h.holds;
    h.post(0, 32, 4);
    (void)h.ask(h.holds.wide);
    h.holds = saved;
    CHECK(h.holds.wide.left == kSelectHoldBatches - 1 && h.holds.wide.seen == h.seq - 1);
  }
  // (4) a hold counts search calls: asked again for a later chunk of the same call, the first answer stands and is not counted twice
  {
    Handle h;
    h.post(32, 32, 4);
    const uint64_t call = ++h.holds.call;
    for (int chunk = 0; chunk < 3; chunk++) CHECK(h.holds.wide.ask(h.stats, call));
    CHECK(h.holds.wide.left == kSelectHoldBatches - 1);
    h.holds.wide.left = 1;
    CHECK(h.ask(h.holds.wide) && h.holds.wide.left == 0);
    const uint64_t next = ++h.holds.call;
    CHECK(!h.holds.wide.ask(h.stats, next));
    h.post(32, 32, 4);  // a verdict that arrives in mid-call is for the next call
    CHECK(!h.holds.wide.ask(h.stats, next) && h.holds.wide.left == kSelectHoldBatches);
    CHECK(h.ask(h.holds.wide) && h.holds.wide.left == kSelectHoldBatches - 1);
  }
  std::printf("{");
  trace("cosine_k10", kCosine, 10, 67, false);
  trace("cosine_k20", kCosine, 20, 67, false);
  trace("euclidean_k10", kEuclidean, 10, 67, false);
  trace("sq8_cosine_k10", kSq8, 10, 67, false);
  std::printf("\"failed_checks\": %d}\n", g_fail);
  return g_fail ? 1 : 0;
}
