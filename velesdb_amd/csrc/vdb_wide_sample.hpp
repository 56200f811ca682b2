// vdb_wide_sample.hpp — the WIDE selection's seed sample as a launch of the selection kernel's SAMPLE instance (sweep_gemm_bf16.hip,
// g16_sample.inc) and the selection launches behind it: host arithmetic only, nothing of HIP in it, so that
// tests/wide_sample_model.cpp can check on the CPU that the sample is whole row tiles inside the corpus, that its keys fit what
// wide_seed reads, and that the selection launches still cover every row tile from row 0 exactly once.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "vdb_gemm_schedule.hpp"

namespace vdb {

constexpr uint32_t kWideSampleRows = 16384;       // rows of the sample up to kWideSampleSmallK: one row tile per block on 64 row groups
constexpr uint32_t kWideSampleRowsLargeK = 32768; // beyond it
constexpr uint32_t kWideSampleSmallK = 32;        // (= kWideSmallSeedMaxK, vdb_wide.hpp)
constexpr uint32_t kWideSampleGroupRows = 64;     // rows per sample key: two lanes of the kernel's accumulator layout (32: one lane)
constexpr uint32_t kWideSampleMaxKeys = 1024;     // keys per query wide_seed / wide_seed_l2 hold (= kWideSeedGroups, vdb_wide.hpp)
// tiles per row group of the selection launches behind the sample (gemm_schedule's head; the rest of the rows in one launch)
constexpr uint32_t kWideSampleHead[3] = {5, 16, 0};

struct WideSamplePlan {
  Bf16GemmPlan bp;    // the sample launch: rows [0, rows), bp.G row groups x bp.nqt query tiles
  uint32_t rows;      // whole 256-row tiles, <= n (0: no sample — a corpus below one row tile)
  uint32_t grp_rows;  // rows per key (32 or 64)
  uint32_t ngrp;      // keys per query = rows / grp_rows <= kWideSampleMaxKeys
};

// The sample does NOT depend on how many row groups the chip holds for the batch: rows / 256 / tiles_per_block row groups (whole XCD
// rounds of 8) x the batch's query tiles, `tiles_per_block` row tiles per block.
inline void wide_sample_plan(uint32_t nq, uint32_t n, uint32_t k, uint32_t tiles_per_block, uint32_t grp_rows, WideSamplePlan* s) {
  tiles_per_block = std::max(1u, tiles_per_block);
  grp_rows = grp_rows == 32 ? 32u : 64u;
  uint32_t rows = (k <= kWideSampleSmallK ? kWideSampleRows : kWideSampleRowsLargeK) * tiles_per_block;
  rows = std::min(rows, kWideSampleMaxKeys * grp_rows);
  rows = std::min(rows, n / kGemmTileRows * kGemmTileRows);
  const uint32_t tiles = rows / kGemmTileRows;
  s->rows = rows;
  s->grp_rows = grp_rows;
  s->ngrp = rows / grp_rows;
  s->bp.nqt = (nq + kGemmTileQueries - 1) / kGemmTileQueries;
  s->bp.qper = s->bp.nqt ? (nq + s->bp.nqt - 1) / s->bp.nqt : 0;
  s->bp.row_lo = 0;
  s->bp.row_hi = rows;
  s->bp.G = (std::max(1u, tiles / tiles_per_block) + 7) / 8 * 8;  // (the kernel's block map wants whole rounds of 8; a group past the tiles idles)
  s->bp.blocks = (int)(s->bp.G * s->bp.nqt);
}

}  // namespace vdb
