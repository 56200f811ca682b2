// vdb_sweep_pass.hpp — what every pass of an exact sweep does around its own kernel, written once (host side; index.hip,
// select_stage.hip, storage_modes.hip, bits_gemm.hip): the slice of a batch a pass answers, the argument struct filled from the
// handle, the timed launch and the merge of the partial lists behind it.  Plain inline functions: nothing is allocated per pass.
#pragma once
#include <string>

#include "vdb_index.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

// nq device-resident queries and where their answers go: [nq][k] ids and scores, [nq] counts
struct QuerySlice {
  const float* d_q;
  uint64_t q_stride;
  uint32_t nq, k;
  uint64_t* d_ids;
  float* d_scores;
  uint32_t* d_n;
  // queries [q0, q0 + n) of this slice
  QuerySlice sub(uint32_t q0, uint32_t n) const {
    return {d_q + (size_t)q0 * q_stride, q_stride, n, k, d_ids + (size_t)q0 * k, d_scores + (size_t)q0 * k, d_n + q0};
  }
  QuerySlice query(uint32_t i) const { return sub(i, 1); }
};

// what a tier of a dispatch ladder answers when it is asked for the front of a slice
struct Took {
  int32_t rc = VDB_OK;       // != VDB_OK: the error (fail() has recorded its text)
  uint32_t n = 0;            // queries answered from the front of the slice; 0: the tier does not take this chunk
  uint32_t handed_back = 0;  // (tier_euclid_gemm) this many queries at the front lack a proof: the exact tiles answer them
  Took() = default;
  Took(int32_t error) : rc(error) {}  // (what fail() and VDB_HIP return)
  static Took queries(uint32_t n) {
    Took t;
    t.n = n;
    return t;
  }
  bool open() const { return rc == VDB_OK && n == 0; }  // the next tier is asked
};

// no row can answer: every query's count is 0
static inline int32_t zero_results(const QuerySlice& s, hipStream_t st) {
  VDB_HIP(hipMemsetAsync(s.d_n, 0, (size_t)s.nq * 4, st));
  return VDB_OK;
}

// the f32 rows of the handle under the mask this call honours; the caller sets part_keys (part_cnt), nq and k
static inline SweepArgs sweep_args(const vdb_hip_index* ix, const QuerySlice& s) {
  SweepArgs a{};
  a.rows = ix->rows.as<float>();
  a.norms = ix->norms.as<float>();
  a.alive = search_alive(ix);
  a.queries = s.d_q;
  a.row_stride = ix->row_stride;
  a.q_stride = s.q_stride;
  a.n_rows = (uint32_t)ix->n_rows;
  a.dim = ix->dim;
  return a;
}

// one launch (or one schedule of launches) of a sweep family: its bit in last_kernels, a HIP event pair around it when kernel timing is
// on, a launch error as the call's error.  launch() returns hipError_t; `what` is the site's text in front of HIP's.
template <class F>
static inline int32_t timed_launch(vdb_hip_index* ix, uint32_t kernel_bits, hipStream_t st, const char* what, F&& launch) {
  ix->last_kernels |= kernel_bits;
  EventPair* ev = next_events(ix);
  if (ev) (void)hipEventRecord(ev->a, st);
  const hipError_t e = launch();
  if (ev) (void)hipEventRecord(ev->b, st);
  if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return VDB_OK;
}

// the partial lists of a pass [s.nq][n_lists][s.k] -> the slice's answers.  ext_ids = nullptr: internal rows (a merge into scratch)
static inline void merge_pass(bool higher_is_better, const uint64_t* part_keys, const uint32_t* part_cnt, uint32_t n_lists, const QuerySlice& s,
                              hipStream_t st, const uint64_t* ext_ids) {
  MergeArgs m{};
  m.part_keys = part_keys;
  m.part_cnt = part_cnt;
  m.ext_ids = ext_ids;
  m.out_ids = s.d_ids;
  m.out_scores = s.d_scores;
  m.out_n = s.d_n;
  m.n_lists = n_lists;
  m.k = s.k;
  launch_merge(higher_is_better, m, s.nq, st);
}
static inline void merge_pass(const vdb_hip_index* ix, bool higher_is_better, const uint64_t* part_keys, const uint32_t* part_cnt, uint32_t n_lists,
                              const QuerySlice& s, hipStream_t st) {
  merge_pass(higher_is_better, part_keys, part_cnt, n_lists, s, st, ix->ext_ids.as<uint64_t>());
}

// The packed-bit path of brute_dev (Hamming / Jaccard indexes) and of the Binary storage mode are one function (index.hip
// brute_bits_dev); this is everything the two differ in
struct BitsSource {
  const uint32_t* bits;  // [n_rows][words]: the packed rows, or the sign-bit codes
  // packs the slice's queries into qbits [nq][words] the way the rows were packed
  void (*pack_queries)(const vdb_hip_index* ix, const QuerySlice& s, uint32_t* qbits, hipStream_t st);
  int metric;            // the index's bit metric, or VDB_HAMMING between sign-bit codes
  // the four-bit image of `bits` for the matrix cores (bits_gemm.hip) and where it leaves the image and the rows' bit counts
  int32_t (*ensure_image)(vdb_hip_index* ix, hipStream_t st);
  DevBuf vdb_hip_index::*img;
  DevBuf vdb_hip_index::*cnt;
  uint32_t sign_rule;    // BitsFusedArgs::sign_rule of the one-launch kernel
  bool higher_is_better;
  const char* what_fused;  // error texts of the two launches
  const char* what_sweep;
};
int32_t brute_bits_dev(vdb_hip_index* ix, const BitsSource& src, const QuerySlice& s, hipStream_t st);

}  // namespace vdb
