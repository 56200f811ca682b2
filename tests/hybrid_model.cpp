// hybrid_model.cpp — velesdb_amd/csrc/vdb_hybrid.hpp compiled for the host: the hybrid-search rule the kernel (csrc/hybrid.hip) is
// written over, driven the way the kernel drives it — the filtered form's stable compaction of the text hits first, records
// (list << 13 | position, live, id) sorted by (id, list, position), the head of every id run folded by hybrid::fuse_run, the fused
// records sorted by (total-order score descending, id descending), the cut at k, the unfiltered form's drop of the non-live survivors.
// tests/test_hybrid_cpu.py builds this with g++ -ffp-contract=off and holds it bit for bit to tests/hybrid_ref.py;
// tools/hybrid_probe.py uses it as the host side of its comparison.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vdb_hybrid.hpp"

using namespace vdb::hybrid;
namespace fusion = vdb::fusion;

extern "C" {

uint32_t hybrid_model_max_records() { return VDB_HYBRID_MAX_RECORDS; }
uint32_t hybrid_model_default_weight_bits() { return fusion::f2u(kDefaultWeight); }
// clamp(vector_weight, 0, 1) as f32 bits; 0 = NaN (refused), 1 = valid
int hybrid_model_clamp(float w, uint32_t* out_bits) {
  if (!weight_valid(w)) return 0;
  *out_bits = fusion::f2u(clamp_weight(w));
  return 1;
}

// one user query.  text_flags: nullable (every text id live and allowed), else per text hit kTextLive | kTextAllowed.  filtered != 0:
// hybrid_search_with_filter.  out_ids / out_score_bits hold max(k, 1) entries, padded as the library pads.  Returns 0, -1 for a NaN
// weight, -7 when the two lists hold more than VDB_HYBRID_MAX_RECORDS ids.
int hybrid_model_fuse(const uint64_t* vec_ids, uint32_t nv, const uint64_t* text_ids, const uint8_t* text_flags, uint32_t nt, float weight,
                      int filtered, uint32_t k, uint64_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n) {
  if (!weight_valid(weight)) return -1;
  if ((uint64_t)nv + nt > VDB_HYBRID_MAX_RECORDS) return -7;
  const float w = clamp_weight(weight), tw = text_weight(w);
  std::vector<Rec> recs;
  for (uint32_t p = 0; p < nv; p++) recs.push_back(rec_of(0, p, true, vec_ids[p]));
  uint32_t pos = 0;
  for (uint32_t p = 0; p < nt; p++) {
    const uint32_t flags = text_flags ? text_flags[p] : (kTextLive | kTextAllowed);
    if (!text_ranked(flags, filtered != 0)) continue;
    recs.push_back(rec_of(1, pos++, (flags & kTextLive) != 0, text_ids[p]));
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return fusion::rec_less<false>(a, b); });
  const uint32_t n = (uint32_t)recs.size();
  std::vector<Rec> fused;
  for (uint32_t i = 0; i < n;) {
    uint32_t run = 0, live = 0;
    const float s = fuse_run([&](uint32_t j) { return recs[j]; }, i, n, w, tw, &run, &live);
    fused.push_back(fused_of(s, live & 1u, recs[i].z, recs[i].w));
    i += run;
  }
  std::sort(fused.begin(), fused.end(), [](const Rec& a, const Rec& b) { return fused_less(a, b); });
  const uint32_t m = std::min<uint32_t>(k, (uint32_t)fused.size());
  uint32_t o = 0;
  for (uint32_t e = 0; e < m; e++) {
    if (!fused[e].y) continue;  // (unfiltered form: behind the cut; the filtered form holds live records only)
    out_ids[o] = fusion::rec_id(fused[e]);
    out_score_bits[o] = fused_score_bits(fused[e]);
    o++;
  }
  *out_n = o;
  for (; o < k; o++) {
    out_ids[o] = ~0ull;
    out_score_bits[o] = 0x7FC00000u;
  }
  return 0;
}

// nq queries of one call, all live, no filter (lists [nq][stride]): what a caller of vdb_hip_index_search_batch does on the host today
int hybrid_model_fuse_batch(const uint64_t* vec_ids, const uint32_t* vec_n, uint32_t vec_stride, const uint64_t* text_ids, const uint32_t* text_n,
                            uint32_t text_stride, const float* weights, uint32_t nq, uint32_t k, uint64_t* out_ids, uint32_t* out_score_bits,
                            uint32_t* out_n) {
  const size_t kk = k ? k : 1;
  for (uint32_t i = 0; i < nq; i++) {
    const int rc = hybrid_model_fuse(vec_ids + (size_t)i * vec_stride, vec_n[i], text_ids + (size_t)i * text_stride, nullptr, text_n[i],
                                     weights ? weights[i] : kDefaultWeight, 0, k, out_ids + i * kk, out_score_bits + i * kk, out_n + i);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
