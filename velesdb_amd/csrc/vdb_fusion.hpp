// vdb_fusion.hpp — the rule of FusionStrategy::fuse (fusion/strategy.rs:138-300) and of the over-fetch in front of it
// (collection/search/batch.rs:270-275), written once as host / device inline functions: fusion.hip's fuse_lists_kernel is written
// over them, and tests/fusion_model.cpp compiles the very same text for the host, so that the CPU tier (tests/test_fusion_cpu.py)
// runs the PRODUCT's rule against a numpy restatement of the reference, not a second restatement.
//
// One group = V lists; list q holds n_q records (id u64, score f32), best first.
//   per (id, q):  best_q(id) = the maximum over the id's occurrences in list q, rank_q(id) = the 0-based position of the first one
//                 (the reference's in-query de-duplication: `query_best` / `seen`)
//   Average       sum of best_q over the lists that contain the id, ascending q, a left fold that starts at the first term, divided
//                 by (float)count
//   Maximum       the maximum over all occurrences
//   RRF{k}        0.0f + sum over the containing lists, ascending q, of 1.0f / ((float)k + (float)(rank_q + 1))
//   Weighted      (a * avg + m * mx) + h * hit: avg as above, mx = a maximum fold from -inf over best_q, hit = (float)count /
//                 (float)V — V counts empty lists too (`total_queries = results.len()`)
// Every operation is rounded on its own (the library is built with -ffp-contract=off; no fmaf here).
// Order of the fused list: descending by the IEEE total order of the fused score (`b.1.total_cmp(&a.1)`), equal scores by id
// ascending.  Deviation 1: the reference leaves the order of equal scores to HashMap iteration — every tie order is one of its
// possible outputs, ours is fixed.  Deviation 2: a NaN weight is INVALID here; the reference's `weighted()` lets NaN through (every
// comparison with NaN is false) and then produces NaN scores.
// "Maximum" is the total-order maximum everywhere in this file.  For scores that are not NaN and ids whose scores do not mix +0.0 and
// -0.0 that IS f32::max; NaN scores and mixed zeros are outside the contract (f32::max is itself unspecified for the latter).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VDB_FUSE_FN __host__ __device__ inline
#else
#define VDB_FUSE_FN inline
#endif

// MAX_VECTORS of multi_query_search (batch.rs:238)
#define VDB_MAX_FUSED_VECTORS 10
// records of one group the kernel holds in LDS: 8192 x 16 B = 128 KB of the CU's 160 KB
#define VDB_FUSE_MAX_RECORDS 8192

namespace vdb {
namespace fusion {

constexpr int kAverage = 0, kMaximum = 1, kRrf = 2, kWeighted = 3;  // enum vdb_fusion_strategy

VDB_FUSE_FN uint32_t f2u(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
VDB_FUSE_FN float u2f(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// u32 whose unsigned order is f32::total_cmp's
VDB_FUSE_FN uint32_t total_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
// sort key of a fused score: ascending key = descending score
VDB_FUSE_FN uint32_t desc_key(uint32_t bits) { return ~total_key(bits); }
VDB_FUSE_FN float max_total(float a, float b) { return total_key(f2u(b)) > total_key(f2u(a)) ? b : a; }

// overfetch_k of multi_query_search (batch.rs:270-275); 64-bit so that the caller sees a product past u32 instead of a wrapped one
VDB_FUSE_FN uint64_t overfetch(uint32_t top_k) {
  const uint64_t k = top_k;
  if (top_k <= 10) return k * 20;
  if (top_k <= 50) return k * 10;
  if (top_k <= 100) return k * 5;
  return k * 2;
}

// FusionStrategy::weighted (strategy.rs:95-122) — and NaN is refused (deviation 2).  0 = valid, 1 = a negative weight, 2 = the sum
VDB_FUSE_FN int weights_error(float a, float m, float h) {
  if (a != a || m != m || h != h) return 2;
  if (a < 0.0f || m < 0.0f || h < 0.0f) return 1;
  float d = ((a + m) + h) - 1.0f;
  if (d < 0.0f) d = -d;
  return d > 0.001f ? 2 : 0;
}

// one id's state while its lists go by in ascending q
struct Acc {
  uint32_t count;  // lists that contain the id
  float sum;       // Average / Weighted: left fold of best_q from the first term
  float mx;        // Weighted: maximum fold from -inf; Maximum: the same value (count >= 1)
  float mx_first;  // Maximum: fold that starts at the first term
  float rrf;       // RRF: fold from 0.0f
};
VDB_FUSE_FN void acc_init(Acc& a) {
  a.count = 0;
  a.sum = 0.0f;
  a.mx = u2f(0xFF800000u);
  a.mx_first = 0.0f;
  a.rrf = 0.0f;
}
// list q contains the id: best = best_q(id), rank = rank_q(id)
VDB_FUSE_FN void acc_add(Acc& a, float best, uint32_t rank, uint32_t rrf_k) {
  a.sum = a.count ? a.sum + best : best;
  a.mx_first = a.count ? max_total(a.mx_first, best) : best;
  a.mx = max_total(a.mx, best);
  a.rrf = a.rrf + 1.0f / ((float)rrf_k + (float)(rank + 1u));
  a.count++;
}
// the fused score of an id with count >= 1 in a group of V lists; w = {avg, max, hit} (WEIGHTED only)
VDB_FUSE_FN float acc_finish(const Acc& a, int strategy, uint32_t V, float w_avg, float w_max, float w_hit) {
  if (strategy == kMaximum) return a.mx_first;
  if (strategy == kRrf) return a.rrf;
  const float avg = a.sum / (float)a.count;
  if (strategy == kAverage) return avg;
  const float hit = (float)a.count / (float)V;
  const float p0 = w_avg * avg;
  const float p1 = w_max * a.mx;
  const float p2 = w_hit * hit;
  return (p0 + p1) + p2;
}

// A record of the kernel's LDS list, 16 bytes.  Stage 1 (x = list ordinal << 13 | position, y = score bits, z / w = id low / high)
// sorts by (id, x); stage 2 (x = desc_key(fused score), y = fused score bits) sorts by (x, id).
struct Rec {
  uint32_t x, y, z, w;
};
constexpr uint32_t kPosBits = 13;  // positions and list ordinals of a group are < VDB_FUSE_MAX_RECORDS = 2^13
VDB_FUSE_FN uint64_t rec_id(const Rec& r) { return ((uint64_t)r.w << 32) | r.z; }
template <bool BY_SCORE>
VDB_FUSE_FN bool rec_less(const Rec& a, const Rec& b) {
  if (BY_SCORE) {
    if (a.x != b.x) return a.x < b.x;
    if (a.w != b.w) return a.w < b.w;
    return a.z < b.z;
  }
  if (a.w != b.w) return a.w < b.w;
  if (a.z != b.z) return a.z < b.z;
  return a.x < b.x;
}

// The records [i, end of the id's run) of a stage-1 sorted list of n records, i = the head of the run: the fused score of the id.
// `at(j)` reads record j.  *run = records in the run.
template <class At>
VDB_FUSE_FN float fuse_run(At&& at, uint32_t i, uint32_t n, int strategy, uint32_t rrf_k, uint32_t V, float w_avg, float w_max, float w_hit,
                           uint32_t* run) {
  const Rec head = at(i);
  Acc acc;
  acc_init(acc);
  uint32_t q = head.x >> kPosBits, rank = head.x & ((1u << kPosBits) - 1u);
  float best = u2f(head.y);
  uint32_t j = i + 1;
  for (; j < n; j++) {
    const Rec r = at(j);
    if (r.z != head.z || r.w != head.w) break;
    const uint32_t rq = r.x >> kPosBits;
    if (rq != q) {
      acc_add(acc, best, rank, rrf_k);
      q = rq;
      rank = r.x & ((1u << kPosBits) - 1u);
      best = u2f(r.y);
    } else {
      best = max_total(best, u2f(r.y));  // (a later position of the same list: the rank stays the first one's)
    }
  }
  acc_add(acc, best, rank, rrf_k);
  *run = j - i;
  return acc_finish(acc, strategy, V, w_avg, w_max, w_hit);
}

}  // namespace fusion
}  // namespace vdb
