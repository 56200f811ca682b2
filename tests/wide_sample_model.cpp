// wide_sample_model.cpp — the WIDE selection's sample plan (velesdb_amd/csrc/vdb_wide_sample.hpp, the text the library compiles)
// walked on the CPU: the sample range is whole row tiles inside the corpus, its keys fit what wide_seed reads, the sample launch's
// block map reaches every (sample row tile, query tile) pair exactly once, and the selection launches behind it
// (gemm_schedule with kWideSampleHead) cover every row tile from row 0 exactly once.  Built and run by tests/test_wide_sample_plan_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vdb_wide_sample.hpp"

using namespace vdb;

static long g_bad = 0;
#define EXPECT(C, ...) do { if (!(C)) { if (g_bad++ < 20) { fprintf(stderr, "violation: %s: ", #C); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// the kernel's block map (sweep_gemm_bf16.hip): bid -> (query tile, row group); block (g, qt) takes the row tiles row_lo / 256 + g, + G, ...
static void walk(const Bf16GemmPlan& p, uint32_t nq, std::vector<uint8_t>& seen /* [tiles][nqt] */, uint32_t ntiles_all) {
  const uint32_t ntiles = (uint32_t)(((uint64_t)p.row_hi + kGemmTileRows - 1) / kGemmTileRows);
  EXPECT(p.row_lo % kGemmTileRows == 0, "row_lo %u", p.row_lo);
  EXPECT(p.G % 8 == 0 && p.blocks == (int)(p.G * p.nqt), "G %u blocks %d", p.G, p.blocks);
  EXPECT((uint64_t)p.qper * p.nqt >= nq && p.qper <= kGemmTileQueries, "qper %u nqt %u nq %u", p.qper, p.nqt, nq);
  for (uint32_t bid = 0; bid < (uint32_t)p.blocks; bid++) {
    const uint32_t xcd = bid & 7u, slot = bid >> 3, qt = slot % p.nqt, g = (slot / p.nqt) * 8u + xcd;
    for (uint32_t rt = p.row_lo / kGemmTileRows + g; rt < ntiles; rt += p.G) {
      EXPECT(rt < ntiles_all, "tile %u of %u", rt, ntiles_all);
      if (rt < ntiles_all) seen[(size_t)rt * p.nqt + qt]++;
    }
  }
}

int main() {
  const uint32_t nqs[] = {16, 96, 256, 1000, 1024}, ns[] = {65536, 66001, 1000000, 6250000}, ks[] = {1, 10, 32, 33, 50, 100, 128};
  const int n_cus = 256;
  long cases = 0;
  for (uint32_t nq : nqs)
    for (uint32_t n : ns)
      for (uint32_t k : ks)
        for (uint32_t tpb : {1u, 2u})
          for (uint32_t grp : {32u, 64u}) {
            cases++;
            WideSamplePlan s;
            wide_sample_plan(nq, n, k, tpb, grp, &s);
            EXPECT(s.rows > 0 && s.rows % kGemmTileRows == 0 && s.rows <= n, "rows %u n %u", s.rows, n);
            EXPECT(s.grp_rows == grp && s.ngrp * s.grp_rows == s.rows && s.ngrp <= kWideSampleMaxKeys && s.ngrp >= k, "ngrp %u rows %u k %u", s.ngrp, s.rows, k);
            EXPECT(s.bp.row_lo == 0 && s.bp.row_hi == s.rows, "sample range");
            // the sample grid does not depend on the chip: row groups = sample tiles / tiles per block
            EXPECT(s.bp.G == (s.rows / kGemmTileRows / tpb + 7) / 8 * 8, "G %u", s.bp.G);
            const uint32_t stiles = s.rows / kGemmTileRows;
            std::vector<uint8_t> seen((size_t)stiles * s.bp.nqt, 0);
            walk(s.bp, nq, seen, stiles);
            for (uint8_t c : seen) EXPECT(c == 1, "a sample tile is swept %u times (nq %u n %u k %u tpb %u)", (unsigned)c, nq, n, k, tpb);
            // the selection launches: from row 0, every row tile exactly once
            GemmSchedule sch;
            gemm_schedule(nq, 0, n, n_cus, kWideSampleHead, 0, &sch);
            EXPECT(sch.n_launch >= 1 && sch.n_launch <= 3, "launches %d", sch.n_launch);
            const uint32_t tiles = (n + kGemmTileRows - 1) / kGemmTileRows;
            std::vector<uint8_t> all((size_t)tiles * sch.bp[0].nqt, 0);
            uint32_t lo = 0;
            for (int j = 0; j < sch.n_launch; j++) {
              EXPECT(sch.bp[j].row_lo == lo && sch.bp[j].row_hi > lo, "launch %d starts at %u, expected %u", j, sch.bp[j].row_lo, lo);
              lo = sch.bp[j].row_hi;
              walk(sch.bp[j], nq, all, tiles);
            }
            EXPECT(lo == n, "the launches end at %u of %u rows", lo, n);
            for (uint8_t c : all) EXPECT(c == 1, "a row tile is swept %u times (nq %u n %u)", (unsigned)c, nq, n);
            if (nq == 96 && n <= 66001) EXPECT(sch.n_launch == 1, "96 queries over %u rows: %d launches", n, sch.n_launch);
          }
  printf("{\"ok\": %s, \"violations\": %ld, \"cases\": %ld}\n", g_bad ? "false" : "true", g_bad, cases);
  return g_bad ? 1 : 0;
}
