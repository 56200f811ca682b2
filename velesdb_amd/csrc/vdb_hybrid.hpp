// vdb_hybrid.hpp — the rule of Collection::hybrid_search / hybrid_search_with_filter (collection/search/text.rs:113-299): one vector
// list and one BM25 text list fused by a weighted Reciprocal Rank Fusion.  Written once as host / device inline functions, in the
// manner of vdb_fusion.hpp: hybrid.hip's hybrid_fuse_kernel is written over them and tests/hybrid_model.cpp compiles the very same
// text for the host, so that the CPU tier (tests/test_hybrid_cpu.py) runs the PRODUCT's rule against a numpy restatement of the
// reference.  The BM25 index is the caller's: the rule takes ids, never scores — it uses ranks only.
//
// One user query = a vector list V (ids, best first), a text list T (ids, best first), a weight.
//   w  = clamp(vector_weight, 0, 1) in f32 (f32::clamp: below 0 -> 0, above 1 -> 1, everything else as it is), default 0.5f
//   tw = 1.0f - w
//   score(id) = 0.0f, + w / ((float)r + 60.0f) for every occurrence of the id at 0-based position r of V in ascending r, then
//               + tw / ((float)r + 60.0f) for every occurrence at position r of T in ascending r.
// EVERY occurrence adds: the reference has no in-list de-duplication here (`*entry.or_insert(0.0) += rrf_score`), unlike
// FusionStrategy::fuse.  Every operation is rounded on its own (the library is built with -ffp-contract=off; no fmaf here).
// ONE sort key: fused score descending by the IEEE total order, equal scores by id DESCENDING; the first k ids under it are the
// result.  Membership at the cut is the reference's: its heap holds Reverse((OrderedFloat(score), id)) and pops the smallest
// (score, id), so among equal scores the LARGER ids survive (text.rs:166-173).  The order among equal scores is unspecified there
// (a stable sort of a heap's drain); ours is the one consistent with the membership key.  This is NOT vdb_fusion.hpp's tie rule (id
// ascending) — on purpose: FusionStrategy::fuse has no defined cut, hybrid_search has.  Ties are the common case: at w = 0.5 vector
// rank r and text rank r tie exactly, at w = 0 or 1 a whole list ties at +0.0.
// Unfiltered form: a text id the handle does not know, or whose row is removed, takes its rank, its score and its place in the
// cut and is then dropped from the output (the reference's filter_map over vector_storage.retrieve BEHIND the cut, text.rs:186-200).
// Filtered form (deviation 1, the one DESIGN 4.1g / h / j make): text hits whose row is unknown, removed or outside the filter are
// dropped BEFORE ranks are assigned, by a stable compaction; the reference ranks, fuses, sorts, post-filters and takes k.
// Deviation 2: a NaN weight is INVALID here; Rust's clamp lets NaN through and the reference then produces NaN scores.
#pragma once
#include <stdint.h>

#include "vdb_fusion.hpp"

// |V| + |T| of one user query the kernel holds in LDS: the fusion kernel's figure (16-byte records, 128 KB of the CU's 160 KB)
#define VDB_HYBRID_MAX_RECORDS VDB_FUSE_MAX_RECORDS

namespace vdb {
namespace hybrid {

using fusion::Rec;

constexpr float kDefaultWeight = 0.5f;
constexpr uint32_t kTextLive = 1u, kTextAllowed = 2u;  // flags of a text hit: its row is known and not removed; the filter holds it

VDB_FUSE_FN bool weight_valid(float w) { return w == w; }
// f32::clamp(0.0, 1.0) of a weight that is not NaN
VDB_FUSE_FN float clamp_weight(float w) {
  if (w < 0.0f) return 0.0f;
  if (w > 1.0f) return 1.0f;
  return w;
}
VDB_FUSE_FN float text_weight(float w) { return 1.0f - w; }
// what one occurrence at 0-based position r of a list of weight wl adds
VDB_FUSE_FN float term(float wl, uint32_t r) { return wl / ((float)r + 60.0f); }
// a text hit takes a rank: always in the unfiltered form, only when live and allowed in the filtered one
VDB_FUSE_FN bool text_ranked(uint32_t flags, bool filtered) { return !filtered || flags == (kTextLive | kTextAllowed); }

// Stage 1 of the kernel's LDS list: x = list << 13 | position (list 0 = V, 1 = T; positions < VDB_HYBRID_MAX_RECORDS = 2^13),
// y = 1 when the id is live, z / w = id low / high; sorted by (id, x) — fusion::rec_less<false>.
VDB_FUSE_FN Rec rec_of(uint32_t list, uint32_t pos, bool live, uint64_t id) {
  return Rec{(list << fusion::kPosBits) | pos, live ? 1u : 0u, (uint32_t)id, (uint32_t)(id >> 32)};
}
// The records [i, end of the id's run) of a stage-1 sorted list of n records, i = the head of the run: the fused score of the id.
// `at(j)` reads record j.  *run = records in the run, *live = an occurrence of the id is live.
template <class At>
VDB_FUSE_FN float fuse_run(At&& at, uint32_t i, uint32_t n, float w, float tw, uint32_t* run, uint32_t* live) {
  const Rec head = at(i);
  float s = 0.0f;
  uint32_t lv = 0, j = i;
  for (; j < n; j++) {
    const Rec r = at(j);
    if (r.z != head.z || r.w != head.w) break;
    s = s + term((r.x >> fusion::kPosBits) ? tw : w, r.x & ((1u << fusion::kPosBits) - 1u));
    lv |= r.y;
  }
  *run = j - i;
  *live = lv;
  return s;
}

// Stage 2: x = desc_key(fused score), y = live, z / w = id; sorted by (x ascending, id DESCENDING).  The score travels in x alone.
VDB_FUSE_FN Rec fused_of(float score, uint32_t live, uint32_t id_lo, uint32_t id_hi) { return Rec{fusion::desc_key(fusion::f2u(score)), live, id_lo, id_hi}; }
VDB_FUSE_FN uint32_t fused_score_bits(const Rec& r) {
  const uint32_t t = ~r.x;  // total_key of the score
  return (t >> 31) ? (t ^ 0x80000000u) : ~t;
}
VDB_FUSE_FN bool fused_less(const Rec& a, const Rec& b) {
  if (a.x != b.x) return a.x < b.x;
  if (a.w != b.w) return a.w > b.w;
  return a.z > b.z;
}
// sorts behind every fused record (no fused score is the NaN whose key is ~0: scores are sums of quotients of clamped weights)
VDB_FUSE_FN Rec fused_pad() { return Rec{0xFFFFFFFFu, 0u, 0u, 0u}; }

}  // namespace hybrid
}  // namespace vdb
