// fusion_model.cpp — velesdb_amd/csrc/vdb_fusion.hpp compiled for the host: the fusion rule the kernel (csrc/fusion.hip) is written
// over, driven the way the kernel drives it — records (id, list ordinal << 13 | position, score), sorted by (id, list, position), the
// head of every id run folded by fusion::fuse_run, the fused pairs sorted by (total-order score descending, id ascending).
// tests/test_fusion_cpu.py builds this with g++ -ffp-contract=off and holds it bit for bit to tests/fusion_ref.py; tools/fusion_probe.py
// uses it as the host side of its comparison.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vdb_fusion.hpp"

using namespace vdb::fusion;

extern "C" {

uint32_t fusion_model_max_vectors() { return VDB_MAX_FUSED_VECTORS; }
uint32_t fusion_model_max_records() { return VDB_FUSE_MAX_RECORDS; }
uint64_t fusion_model_overfetch(uint32_t top_k) { return overfetch(top_k); }
int fusion_model_weights_error(float a, float m, float h) { return weights_error(a, m, h); }

// one group: lists [n_lists][stride], list j holds list_n[j] records.  out_ids / out_score_bits hold max(top_k, 1) entries, padded
// as the library pads.  Returns 0, or -7 when the group holds more than VDB_FUSE_MAX_RECORDS records.
int fusion_model_fuse(int strategy, uint32_t rrf_k, const float* w, const uint64_t* ids, const float* scores, const uint32_t* list_n,
                      uint32_t n_lists, uint32_t stride, uint32_t top_k, uint64_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n) {
  std::vector<Rec> recs;
  uint32_t ord = 0;
  for (uint32_t q = 0; q < n_lists; q++) {
    for (uint32_t p = 0; p < list_n[q]; p++) {
      const uint64_t id = ids[(size_t)q * stride + p];
      recs.push_back(Rec{(ord << kPosBits) | p, f2u(scores[(size_t)q * stride + p]), (uint32_t)id, (uint32_t)(id >> 32)});
      if (recs.size() > VDB_FUSE_MAX_RECORDS) return -7;
    }
    if (list_n[q]) ord++;
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return rec_less<false>(a, b); });
  const uint32_t n = (uint32_t)recs.size();
  std::vector<Rec> fused;
  for (uint32_t i = 0; i < n;) {
    uint32_t run = 0;
    const float s = fuse_run([&](uint32_t j) { return recs[j]; }, i, n, strategy, rrf_k, n_lists, w[0], w[1], w[2], &run);
    fused.push_back(Rec{desc_key(f2u(s)), f2u(s), recs[i].z, recs[i].w});
    i += run;
  }
  std::sort(fused.begin(), fused.end(), [](const Rec& a, const Rec& b) { return rec_less<true>(a, b); });
  const uint32_t m = std::min<uint32_t>(top_k, (uint32_t)fused.size());
  for (uint32_t e = 0; e < top_k; e++) {
    out_ids[e] = e < m ? rec_id(fused[e]) : ~0ull;
    out_score_bits[e] = e < m ? fused[e].y : 0x7FC00000u;
  }
  *out_n = m;
  return 0;
}

// n_groups groups of one call (consecutive lists, group_sizes[g] each): what a caller of vdb_hip_index_search_batch does on the host today
int fusion_model_fuse_groups(int strategy, uint32_t rrf_k, const float* w, const uint64_t* ids, const float* scores, const uint32_t* list_n,
                             uint32_t stride, const uint32_t* group_sizes, uint32_t n_groups, uint32_t top_k, uint64_t* out_ids,
                             uint32_t* out_score_bits, uint32_t* out_n) {
  const size_t kk = top_k ? top_k : 1;
  uint32_t first = 0;
  for (uint32_t g = 0; g < n_groups; g++) {
    const int rc = fusion_model_fuse(strategy, rrf_k, w, ids + (size_t)first * stride, scores + (size_t)first * stride, list_n + first, group_sizes[g],
                                     stride, top_k, out_ids + g * kk, out_score_bits + g * kk, out_n + g);
    if (rc) return rc;
    first += group_sizes[g];
  }
  return 0;
}

}  // extern "C"
