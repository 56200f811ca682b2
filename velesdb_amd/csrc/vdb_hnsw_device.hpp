// vdb_hnsw_device.hpp — device building blocks shared by the traversal (hnsw_kernels.hip) and
// construction (hnsw_build.hip) kernels: the sorted candidate/result list in LDS, the block-wide
// distance phase (DistanceEngine::distance, native/distance.rs:75-85, canonical arithmetic) and small
// wave-uniform helpers; and the walk itself (hnsw_walk_body), one text for the f32 / packed-bit rows
// (hnsw_kernels.hip) and the f16 / bf16 images (hnsw_half.hip).
#pragma once
#include "vdb_device.hpp"
#include "vdb_kernels.hpp"

namespace vdb {

// what the distance phase needs to know about the vector storage
struct DistCtx {
  const float* rows;
  const float* norms;
  const uint32_t* bits;
  uint64_t row_stride;
  uint32_t dim, words;
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float rflf(float v) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v)));
}
__device__ __forceinline__ uint64_t lt_mask(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ float key_dist(uint64_t key) { return asc_key_inv((uint32_t)(key >> 32)); }

// R per-lane partials per lane in a[0..R); afterwards lane l holds in a[0] the canonical 64-lane sum
// of partial index l % R (stages 32..R are plain butterflies, stages R/2..1 are transposed).
template <int R, int S>
struct PlainStages {  // butterfly stages S, S/2, ... R applied to all R values (every lane keeps every index)
  static __device__ __forceinline__ void run(float* a) {
#pragma unroll
    for (int i = 0; i < R; i++) a[i] = add_xor<S>(a[i]);
    if (S > R) PlainStages<R, (S > R ? S / 2 : S)>::run(a);
  }
};
template <int R>
__device__ __forceinline__ void reduce_rows(float* a, int lane) {
  PlainStages<R, 32>::run(a);
  TReduce<R, R / 2>::run(a, lane);
}

// Sorted list insert with per-entry flags.  Wave-uniform arguments, all 64 lanes participate.
// If the list is at capacity its last entry is dropped and reported (key + flag).
__device__ __forceinline__ void list_insert(lds_vu64* keys, lds_vu8* flags, uint32_t& cnt,
                                            uint32_t cap, uint64_t key, int lane, uint64_t& dropped,
                                            uint32_t& dropped_flag) {
  dropped = kKeyInvalid;
  dropped_flag = 1;
  uint32_t pos = 0;
  for (uint32_t c = 0; c < cnt; c += 64) {
    const uint32_t e = c + lane;
    const bool less = e < cnt && keys[e] < key;
    pos += (uint32_t)__popcll(__ballot(less));
  }
  if (pos >= cap) {
    dropped = key;
    dropped_flag = 0;
    return;
  }
  if (cnt == cap) {
    dropped = keys[cap - 1];
    dropped_flag = flags[cap - 1];
  }
  const uint32_t newcnt = cnt < cap ? cnt + 1 : cap;
  if (newcnt - 1 > pos) {
    const uint32_t span = newcnt - 1 - pos;
    for (int32_t c = (int32_t)((span - 1) / 64) * 64; c >= 0; c -= 64) {
      const uint32_t e = pos + (uint32_t)c + lane;
      const bool mv = e < newcnt - 1;
      const uint64_t v = mv ? keys[e] : 0;
      const uint8_t f = mv ? flags[e] : (uint8_t)0;
      if (mv) {
        keys[e + 1] = v;
        flags[e + 1] = f;
      }
    }
  }
  if (lane == 0) {
    keys[pos] = key;
    flags[pos] = 0;
  }
  cnt = newcnt;
}

// The scan of a greedy step on the upper layers (graph.rs:413-421): sequential with strict `<` == the first index of nb_d[0..m)
// attaining the minimum, if that is below best_d; 0xFFFFFFFF when no neighbour improves.  Wave-uniform result.
// UD: nb_d and best_d carry u32 bit patterns (the int8 walk's integer distances, dual_precision.rs:422-433) and are ordered as such.
template <bool UD = false>
__device__ __forceinline__ uint32_t greedy_scan(lds_vf32* nb_d, uint32_t m, float best_d, int lane) {
  if constexpr (UD) {
    const uint32_t best_u = __float_as_uint(best_d);
    uint32_t mn = 0, besti = 0xFFFFFFFFu;
    for (uint32_t base = 0; base < m; base += 64) {
      const uint32_t t = base + lane;
      const uint32_t d = t < m ? __float_as_uint(nb_d[t]) : 0xFFFFFFFFu;
      const bool ok = t < m && d < best_u;
      const uint64_t okm = __ballot(ok);
      if (okm) {
        uint32_t v = ok ? d : 0xFFFFFFFFu;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, s, 64));
        v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
        if (besti == 0xFFFFFFFFu || v < mn) {
          const uint64_t eq = __ballot(ok && d == v);
          besti = base + (uint32_t)__ffsll((long long)eq) - 1;
          mn = v;
        }
      }
    }
    return besti;
  }
  float mn = 0.0f;
  uint32_t besti = 0xFFFFFFFFu;
  for (uint32_t base = 0; base < m; base += 64) {
    const uint32_t t = base + lane;
    const float d = t < m ? nb_d[t] : 0.0f;
    const bool ok = t < m && d < best_d;  // raw compare: NaN never improves
    const uint64_t okm = __ballot(ok);
    if (okm) {
      float v = ok ? d : __uint_as_float(0x7F800000u);
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) v = fminf(v, shx(v, s));
      v = rflf(v);
      if (besti == 0xFFFFFFFFu || v < mn) {
        const uint64_t eq = __ballot(ok && d == v);
        besti = base + (uint32_t)__ffsll((long long)eq) - 1;
        mn = v;
      }
    }
  }
  return besti;
}

// The dynamic LDS of a walk block: keys[cap] u64 | nb_id[nbmax] | nb_d[nbmax] | ctl[4] | flags[cap] u8 (padded to 16) | the query
// scratch of the distance phase.  These are the offsets walk_lds_base (hnsw_kernels.hip) adds up: change both together.
struct WalkLds {
  lds_vu64* keys;
  lds_vu32* nb_id;
  lds_vf32* nb_d;
  lds_vu32* ctl;
  lds_vu8* flags;
  unsigned char* query;
  __device__ __forceinline__ WalkLds(unsigned char* smem, uint32_t cap, uint32_t nbmax) {
    const size_t lists = (size_t)cap * 8 + (size_t)nbmax * 8;
    keys = (lds_vu64*)(lds_void_p)(smem);
    nb_id = (lds_vu32*)(lds_void_p)(smem + (size_t)cap * 8);
    nb_d = (lds_vf32*)(lds_void_p)(smem + (size_t)cap * 8 + (size_t)nbmax * 4);
    ctl = (lds_vu32*)(lds_void_p)(smem + lists);
    flags = (lds_vu8*)(lds_void_p)(smem + lists + 16);
    query = smem + lists + 16 + (((size_t)cap + 15) & ~(size_t)15);
  }
};

// ---- exact visited set in LDS (round 3): open addressing over node id + 1 (0 = empty), linear probing, one LDS compare-
// and-swap per probe.  The HBM bitmap costs a dependent memory round trip per expansion (atomicOr on a line that is rarely
// in L2: 125 KB of bitmap per query in flight) between the neighbour ids and their rows; this costs ~100 cycles.  Exact: a
// node is reported new exactly once.  The kernels stop a query (overflow flag -> the caller re-runs it on the bitmap) before
// the table passes 3/4 of its entries, so a probe sequence always ends.
struct VisSet {
  uint32_t* tab;   // LDS, `mask + 1` entries
  uint32_t mask;   // entries - 1 (a power of two)
  uint32_t shift;  // 32 - log2(entries)
  __device__ __forceinline__ bool test_and_set(uint32_t id) const {  // true: newly inserted (HashSet::insert, graph.rs:499)
    const uint32_t key = id + 1u;
    uint32_t h = (id * 0x9E3779B1u) >> shift;
    for (;;) {
      const uint32_t old = atomicCAS(&tab[h], 0u, key);
      if (old == 0u) return true;
      if (old == key) return false;
      h = (h + 1u) & mask;
    }
  }
  __device__ __forceinline__ void clear(uint32_t tid, uint32_t nthreads) const {  // every thread of the block
    uint4* t4 = reinterpret_cast<uint4*>(tab);
    for (uint32_t i = tid; i < (mask + 1u) / 4u; i += nthreads) t4[i] = uint4{0u, 0u, 0u, 0u};
  }
};

// distance domain of a key: f32 (total-order bits, compared as raw floats like the reference does) or u32 (the
// integer L2^2 of the int8 traversal, dual_precision.rs:336)
template <bool UD>
__device__ __forceinline__ bool key_dist_gt(uint64_t a, uint64_t b) {
  if (UD) return (uint32_t)(a >> 32) > (uint32_t)(b >> 32);
  return key_dist(a) > key_dist(b);
}

// ... and what a walk whose distance phase says which domain it works in (DIST::UD) builds and asks with it: the key of
// (distance, node), a key's distance as the bound of an admission test, and "distance d is below the bound" — the raw compare of
// graph.rs:503 / dual_precision.rs:359.  With UD a float is only the carrier of the u32 bit pattern nb_d holds: never compared or
// converted as a number.
template <bool UD>
__device__ __forceinline__ uint64_t walk_key(float d, uint32_t node) {
  if (UD) return ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)node;
  return make_key<false>(d, node);
}
template <bool UD>
__device__ __forceinline__ float key_bound(uint64_t key) {
  if (UD) return __uint_as_float((uint32_t)(key >> 32));
  return key_dist(key);
}
template <bool UD>
__device__ __forceinline__ bool dist_lt(float d, float bound) {
  if (UD) return __float_as_uint(d) < __float_as_uint(bound);
  return d < bound;
}

// entries past ef stay only up to the last one the termination test could still expand
template <bool UD = false>
__device__ __forceinline__ void list_truncate(lds_vu64* keys, uint32_t& cnt, uint32_t ef, int lane) {
  if (cnt <= ef) return;
  const uint64_t wk = keys[ef - 1];
  uint32_t last = ef - 1;
  for (uint32_t c = ef; c < cnt; c += 64) {
    const uint32_t e = c + lane;
    const bool alive = e < cnt && !key_dist_gt<UD>(keys[e], wk);  // negation of graph.rs:474's raw compare
    const uint64_t mask = __ballot(alive);
    if (mask) last = c + 63u - (uint32_t)__clzll((long long)mask);
  }
  cnt = last + 1;
}

// ---- int8 traversal distances (DualPrecisionHnsw, native/quantization.rs:42-91): integer L2^2 between u8 codes
// = qsq + rsq[row] - 2 * sum(q_i * r_i), every term an exact integer (v_dot4_u32_u8), so the result is the
// reference's u32 bit for bit whatever the summation order.
template <int S>
__device__ __forceinline__ uint32_t add_xor_u32(uint32_t v) {
  if (S == 32) {
    auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return r[0] + r[1];
  } else if (S == 16) {
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return r[0] + r[1];
  } else {
    return v + __float_as_uint(lane_xor<S>(__uint_as_float(v)));
  }
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v = add_xor_u32<32>(v);
  v = add_xor_u32<16>(v);
  v = add_xor_u32<8>(v);
  v = add_xor_u32<4>(v);
  v = add_xor_u32<2>(v);
  v = add_xor_u32<1>(v);
  return v;
}
struct CodeCtx {
  const uint32_t* codes;  // [n_rows][code_words] packed u8 codes, zero padded
  const uint32_t* rsq;    // [n_rows] sum of squared codes
  uint32_t code_words;    // words per row (multiple of 4)
};
// nb_id[0..m) -> nb_d[0..m) as u32 bit patterns.  qw: this lane's query words (word w = lane + 64*j), QW of them.
template <int QW, int WAVES = 4>
__device__ __forceinline__ void dist_phase_int8(const CodeCtx& c, const uint32_t (&qw)[QW], uint32_t qsq, uint32_t m,
                                                lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib) {
  constexpr int R = 8;
  for (uint32_t j0 = (uint32_t)wib * R; j0 < m; j0 += WAVES * R) {
    uint32_t dot[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t j = j0 + r < m ? j0 + r : m - 1;
      const uint32_t* p = c.codes + (size_t)nb_id[j] * c.code_words + lane;
      uint32_t w[QW];
#pragma unroll
      for (int t = 0; t < QW; t++) w[t] = ((uint32_t)lane + 64u * t < c.code_words) ? p[64 * t] : 0u;
      uint32_t acc = 0;
#pragma unroll
      for (int t = 0; t < QW; t++) acc = __builtin_amdgcn_udot4(qw[t], w[t], acc, false);
      dot[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < R; r++) dot[r] = wave_sum_u32(dot[r]);
    // lane r finishes row j0 + r
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < R; r++) mine = (lane == r) ? dot[r] : mine;
    const uint32_t j = j0 + (uint32_t)lane;
    if (lane < R && j < m) {
      const uint32_t d = qsq + c.rsq[nb_id[j]] - 2u * mine;
      nb_d[j] = __uint_as_float(d);
    }
  }
}

// ---- the candidate/result list behind one interface ---------------------------------------------
// Two implementations with identical semantics (the reference's two heaps, see hnsw_kernels.hip):
//   CandList<0>   sorted keys + flags in LDS (any capacity that fits LDS)
//   CandList<NS>  NS*64 entries held in REGISTERS of the leader wave: entry e lives in lane e%64, slot e/64,
//                 sorted ascending, empty slots = ~0.  An insert is one DPP wave_shr:1 per slot (the lane
//                 below hands its entry up; mapping verified with tools/probes/wave_shr_check.hip) + selects:
//                 ~12 VALU instructions per slot, no LDS traffic and no loops — the LDS version spends
//                 hundreds of cycles per admitted neighbour, and admission is the serial part of a step.
// External key = (total-order(dist) << 32 | node).  The register form shifts the node up by one bit and keeps
// the "expanded" flag in bit 0 (node ids < 2^31).
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

template <int NS, bool UD = false>
struct CandList {
  uint64_t k[NS];
  uint32_t cnt;
  static constexpr uint32_t CAP = NS * 64;

  static __device__ __forceinline__ uint64_t enc(uint64_t ext) {
    return (ext & 0xFFFFFFFF00000000ull) | ((ext & 0xFFFFFFFFull) << 1);
  }
  static __device__ __forceinline__ uint64_t dec(uint64_t in) {
    return (in & 0xFFFFFFFF00000000ull) | ((in & 0xFFFFFFFFull) >> 1);
  }
  // lane l receives v of lane l-1; lane 0 receives `carry` (wave-uniform)
  static __device__ __forceinline__ uint64_t shr1(uint64_t v, uint64_t carry) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)carry, (int)(uint32_t)v, 0x138, 0xf, 0xf, false);
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(carry >> 32), (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
  }
  __device__ __forceinline__ void init(lds_vu64*, lds_vu8*, uint32_t) { reset(); }
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int s = 0; s < NS; s++) k[s] = ~0ull;
    cnt = 0;
  }
  __device__ __forceinline__ uint32_t size() const { return cnt; }
  __device__ __forceinline__ void insert(uint64_t ext, int lane, uint32_t& overflow) {
    const uint64_t key = enc(ext);
    const uint64_t last = readlane64(k[NS - 1], 63);
    uint64_t nk[NS];
#pragma unroll
    for (int s = NS - 1; s >= 0; s--) {
      const uint64_t carry = s > 0 ? readlane64(k[s > 0 ? s - 1 : 0], 63) : 0ull;
      const uint64_t prev = shr1(k[s], carry);
      const bool ge = !(k[s] < key);
      const bool pl = (s == 0 && lane == 0) ? true : (prev < key);
      nk[s] = ge ? (pl ? key : prev) : k[s];
    }
#pragma unroll
    for (int s = 0; s < NS; s++) k[s] = nk[s];
    if (last != ~0ull) {  // the list was full: its last entry (or the key itself, if it is the largest) fell off
      const uint64_t dropped = (last < key) ? key : last;
      if ((dropped & 1ull) == 0) overflow = 1;
    } else {
      cnt += 1;
    }
  }
  // Admission of a whole chunk of evaluated neighbours at once (round 3; the sequential loop of P_Z_ADMIT cost 2.6 us of a
  // 7-us expansion: ~0.4 us per admitted neighbour).  `mask` = the lanes whose neighbour passed the chunk-start test of
  // graph.rs:503 (d < furthest || len < ef), d / nb = the lane's distance and node.  Without exact distance ties the
  // sequential process ends with the ef smallest keys of (list U candidates): a candidate among them is below the furthest
  // distance at its turn whatever came before it (the furthest only falls, and removing one of the ef smallest leaves an
  // ef-th that is strictly larger), and every other one is cut by the truncation behind its insert or rejected outright.
  // So: every accepted key's rank among the old entries (two ballots) and among the candidates, every old entry shifted by
  // the number of candidates below it, one scatter through LDS, one truncate.  Returns false — nothing changed — when the
  // caller has to walk the chunk one by one: an exact tie of distances between a candidate and anything (the reference's
  // strict compare decides those in arrival order; equal distances are neighbours in the merged order, so the test looks at
  // neighbours after the scatter), a NaN distance, or more keys than the list holds.
  __device__ __forceinline__ bool admit_batch(uint64_t mask, float d, uint32_t nb, int lane, uint32_t ef, lds_vu64* scratch_v,
                                              lds_vu8*) {
    const uint32_t n_acc = (uint32_t)__popcll(mask);
    const uint32_t total = cnt + n_acc;
    if (total > CAP) return false;
    const bool mine = ((mask >> lane) & 1ull) != 0;
    if (__ballot(mine && !(d == d))) return false;
    const uint64_t mykey = mine ? enc(make_key<false>(d, nb)) : ~0ull;
    uint32_t shift[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) shift[s] = 0;
    uint32_t mypos = 0;
    for (uint64_t rest = mask; rest; rest &= rest - 1) {
      const int j = __ffsll((long long)rest) - 1;
      const uint64_t kj = readlane64(mykey, j);
      uint32_t r = (uint32_t)__popcll(__ballot(mine && mykey < kj));
#pragma unroll
      for (int s = 0; s < NS; s++)
        if ((uint32_t)s * 64u < cnt) {  // (wave-uniform: slots past the list hold nothing)
          const bool lt = k[s] < kj;    // keys are distinct (a node enters the list once): kj < k[s] is its negation
          r += (uint32_t)__popcll(__ballot(lt));
          shift[s] += lt ? 0u : 1u;     // (empty places, ~0, are shifted too: they are not written)
        }
      if (lane == j) mypos = r;
    }
    // Scatter through LDS — plain accesses (a volatile one waits for its own round trip: 20 of them were 3 us), ordered by
    // the wave's in-order LDS queue and the compiler barriers: old entries behind the candidates below them, candidates at old
    // rank + candidate rank; then everything is read back in one go, and every candidate looks at its two neighbours in the
    // merged order (equal distances are neighbours there).
    __attribute__((address_space(3))) uint64_t* scratch = (__attribute__((address_space(3))) uint64_t*)scratch_v;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int s = 0; s < NS; s++)
      if ((uint32_t)s * 64u < cnt && k[s] != ~0ull) scratch[(uint32_t)s * 64u + (uint32_t)lane + shift[s]] = k[s];  // < total <= CAP
    if (mine) scratch[mypos] = mykey;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint64_t nk[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const uint32_t e = (uint32_t)s * 64u + (uint32_t)lane;
      nk[s] = ((uint32_t)s * 64u < total && e < total) ? scratch[e] : ~0ull;
    }
    const uint64_t below = (mine && mypos > 0) ? scratch[mypos - 1] : ~0ull;
    const uint64_t above = (mine && mypos + 1 < total) ? scratch[mypos + 1] : ~0ull;
    asm volatile("" ::: "memory");
    const bool tie = mine && ((below != ~0ull && key_dist(dec(below)) == d) || (above != ~0ull && key_dist(dec(above)) == d));
    if (__ballot(tie)) return false;  // (k, cnt untouched)
#pragma unroll
    for (int s = 0; s < NS; s++) k[s] = nk[s];
    cnt = total;
    truncate(ef, lane);
    return true;
  }
  __device__ __forceinline__ uint32_t first_unexpanded(int) const {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const uint64_t un = __ballot((k[s] & 1ull) == 0);  // empty slots are ~0: bit 0 set
      if (un) return (uint32_t)s * 64 + (uint32_t)__ffsll((long long)un) - 1;
    }
    return kNoIndex;
  }
  __device__ __forceinline__ uint64_t key_at(uint32_t idx, int) const {  // idx wave-uniform
    // (mask-and-or instead of a select chain: the compiler turns the chain into a dynamically indexed load,
    // which forces the whole list into scratch memory)
    const uint32_t slot = idx >> 6;
    uint64_t v = 0;
#pragma unroll
    for (int s = 0; s < NS; s++) v |= k[s] & ((slot == (uint32_t)s) ? ~0ull : 0ull);
    return dec(readlane64(v, (int)(idx & 63)));
  }
  __device__ __forceinline__ void mark_expanded(uint32_t idx, int lane) {
    const uint32_t slot = idx >> 6, l = idx & 63;
#pragma unroll
    for (int s = 0; s < NS; s++) k[s] |= (slot == (uint32_t)s && (uint32_t)lane == l) ? 1ull : 0ull;
  }
  __device__ __forceinline__ void truncate(uint32_t ef, int lane) {
    if (cnt <= ef) return;
    const uint64_t wk = enc(key_at(ef - 1, lane));
    uint32_t last = ef - 1;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const uint32_t e = (uint32_t)s * 64 + lane;
      const bool alive = e >= ef && e < cnt && !key_dist_gt<UD>(k[s], wk);  // negation of graph.rs:474's raw compare
      const uint64_t mask = __ballot(alive);
      if (mask) last = (uint32_t)s * 64 + 63u - (uint32_t)__clzll((long long)mask);
    }
    cnt = last + 1;
#pragma unroll
    for (int s = 0; s < NS; s++)
      if ((uint32_t)s * 64 + lane >= cnt) k[s] = ~0ull;
  }
  // external key of entry base + lane (base a multiple of 64, wave-uniform); meaningless beyond size()
  __device__ __forceinline__ uint64_t chunk_key(uint32_t base, int) const {
    const uint32_t slot = base >> 6;
    uint64_t v = 0;
#pragma unroll
    for (int s = 0; s < NS; s++) v |= k[s] & ((slot == (uint32_t)s) ? ~0ull : 0ull);
    return dec(v);
  }
  // copy the first n entries to LDS as external keys (construction: select_neighbors works on LDS arrays)
  __device__ __forceinline__ void dump(lds_vu64* keys, uint32_t n, int lane) const {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const uint32_t e = (uint32_t)s * 64 + lane;
      if (e < n) keys[e] = dec(k[s]);
    }
  }
};

template <bool UD>
struct CandList<0, UD> {
  lds_vu64* keys;
  lds_vu8* flags;
  uint32_t cnt, cap;
  __device__ __forceinline__ void init(lds_vu64* k_, lds_vu8* f_, uint32_t cap_) {
    keys = k_;
    flags = f_;
    cap = cap_;
    cnt = 0;
  }
  __device__ __forceinline__ void reset() { cnt = 0; }
  __device__ __forceinline__ uint32_t size() const { return cnt; }
  __device__ __forceinline__ void insert(uint64_t ext, int lane, uint32_t& overflow) {
    uint64_t dr;
    uint32_t df;
    list_insert(keys, flags, cnt, cap, ext, lane, dr, df);
    if (dr != kKeyInvalid && df == 0) overflow = 1;  // an unexpanded candidate fell off the list
  }
  __device__ __forceinline__ bool admit_batch(uint64_t, float, uint32_t, int, uint32_t, lds_vu64*, lds_vu8*) { return false; }  // (LDS list: one by one)
  __device__ __forceinline__ uint32_t first_unexpanded(int lane) const {
    for (uint32_t c = 0; c < cnt; c += 64) {
      const uint32_t e = c + lane;
      const uint64_t un = __ballot(e < cnt && flags[e] == 0);
      if (un) return c + (uint32_t)__ffsll((long long)un) - 1;
    }
    return kNoIndex;
  }
  __device__ __forceinline__ uint64_t key_at(uint32_t idx, int) const { return keys[idx]; }
  __device__ __forceinline__ void mark_expanded(uint32_t idx, int lane) {
    if (lane == 0) flags[idx] = 1;
  }
  __device__ __forceinline__ void truncate(uint32_t ef, int lane) { list_truncate<UD>(keys, cnt, ef, lane); }
  __device__ __forceinline__ uint64_t chunk_key(uint32_t base, int lane) const { return keys[base + lane]; }
  __device__ __forceinline__ void dump(lds_vu64*, uint32_t, int) const {}
};

__device__ __forceinline__ float transform_score_dev(int metric, float d) {  // backend_adapter.rs:160-168
  if (metric == kCosine) {
    float s = 1.0f - d;
    if (s < 0.0f) s = 0.0f;
    if (s > 1.0f) s = 1.0f;
    return s;
  }
  if (metric == kDot) return -d;
  return d;
}

// ---- distance evaluation of nb_id[0..m) -> nb_d[0..m): DistanceEngine::distance (native/distance.rs:75-85)
template <int METRIC, int CPL, int WAVES = 4, int R = 8>
__device__ __forceinline__ void dist_phase_f32(const DistCtx& a, const float4* q, float qnorm,
                                               const float* qgen, uint32_t m, lds_vu32* nb_id,
                                               lds_vf32* nb_d, int lane, int wib, bool raw = false) {
  constexpr int OP = (METRIC == kEuclidean) ? kOpL2 : kOpDot;
  const int d4 = (int)((a.dim + 3) / 4);
  for (uint32_t j0 = (uint32_t)wib * R; j0 < m; j0 += WAVES * R) {
    float acc[R];
    // the row's norm (cosine) travels with the rows: requested behind the reduction it was a second dependent round trip
    const uint32_t jn = j0 + (uint32_t)(lane & (R - 1));
    float vnorm_early = 1.0f;
    if (METRIC == kCosine && lane < R && jn < m) vnorm_early = a.norms[nb_id[jn]];
    if (CPL > 0) {
      float4 v[R][CPL > 0 ? CPL : 1];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t j = j0 + r < m ? j0 + r : m - 1;
        const float* p = a.rows + (size_t)nb_id[j] * a.row_stride + (size_t)lane * 4;
#pragma unroll
        for (int c = 0; c < CPL; c++) v[r][c] = ld4(p + c * 256);
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < CPL; c++) s = chain4<OP>(s, q[c], v[r][c]);
        acc[r] = s;
      }
    } else {
      const float* rp[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t j = j0 + r < m ? j0 + r : m - 1;
        rp[r] = a.rows + (size_t)nb_id[j] * a.row_stride;
        acc[r] = 0.0f;
      }
      for (int c = lane; c < d4; c += 64) {
        const float4 qq = ld4(qgen + c * 4);
        const int nv = (int)a.dim - c * 4;
#pragma unroll
        for (int r = 0; r < R; r++) {
          const float4 x = ld4(rp[r] + c * 4);
          acc[r] = nv >= 4 ? chain4<OP>(acc[r], qq, x) : chain4_tail<OP>(acc[r], qq, x, nv);
        }
      }
    }
    reduce_rows<R>(acc, lane);
    const uint32_t j = j0 + (uint32_t)(lane & (R - 1));
    if (lane < R && j < m) {
      const float vnorm = vnorm_early;
      const float s = finish_score<METRIC>(acc[0], qnorm, vnorm);
      // raw = HnswIndex::compute_distance (search.rs:30-38), otherwise DistanceEngine::distance
      nb_d[j] = raw ? s : ((METRIC == kCosine) ? 1.0f - s : ((METRIC == kDot) ? -s : s));
    }
  }
}

// ---- half-precision rows (VectorData::F16 / BF16, half_precision.rs:94-101): IEEE f16 or bf16 images of the rows, the query
// rounded the same way (VectorData::from_f32_slice) and kept as f32.  Both conversions to f32 are exact.
template <bool F16>
__device__ __forceinline__ float round_to_half(float f) {  // f32 -> half (round to nearest even) -> f32
  if (F16) return (float)(_Float16)f;  // v_cvt_f16_f32 / v_cvt_f32_f16: overflow to +-inf, gradual underflow, NaN stays NaN
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return __uint_as_float((u | 0x00400000u) & 0xFFFF0000u);  // NaN stays NaN (quiet)
  u += 0x7FFFu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xFFFF0000u);
}
template <bool F16>
__device__ __forceinline__ float4 round_to_half4(const float4& v) {
  return float4{round_to_half<F16>(v.x), round_to_half<F16>(v.y), round_to_half<F16>(v.z), round_to_half<F16>(v.w)};
}
// four consecutive half elements (8 bytes, element 0 in the low half of w.x) as f32
template <bool F16>
__device__ __forceinline__ float4 half4_to_f32(const uint2& w) {
  if (F16) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 lo = __builtin_bit_cast(f16x2, w.x), hi = __builtin_bit_cast(f16x2, w.y);
    return float4{(float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y};
  }
  return float4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u), __uint_as_float(w.y << 16),
                __uint_as_float(w.y & 0xFFFF0000u)};
}
__device__ __forceinline__ uint2 ld_half4(const uint16_t* p) { return *reinterpret_cast<const uint2*>(p); }
template <bool F16>
__device__ __forceinline__ float half1_to_f32(uint16_t h) {  // one half element as f32 (exact)
  if (F16) return (float)__builtin_bit_cast(_Float16, h);
  return __uint_as_float((uint32_t)h << 16);
}

// nb_id[0..m) -> nb_d[0..m) over the half image: half_precision::dot_product / cosine_similarity / euclidean_distance
// (half_precision.rs:199-287) as DistanceEngine::distance reports them (-dot, 1 - cosine, the root).  The summation order is
// dist_phase_f32's, unchanged — element i in 4-element chunk i / 4, chunk c in lane c % 64, one fmaf chain per lane, the xor
// butterfly — so over image H the results are bit for bit dist_phase_f32's over the f32 rows dequant(H) with the same (rounded)
// query: a lane loads 8 bytes per chunk (512 B per wave instruction) and converts in registers.  a.rows = the image
// (uint16_t elements), a.row_stride = its stride in elements (a multiple of 8, the padding zero), a.norms = the norms of the
// ROUNDED rows.  q / qgen hold the rounded query.
template <int METRIC, int CPL, int WAVES, int R, bool F16>
__device__ __forceinline__ void dist_phase_half(const DistCtx& a, const float4* q, float qnorm, const float* qgen, uint32_t m,
                                                lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib) {
  constexpr int OP = (METRIC == kEuclidean) ? kOpL2 : kOpDot;
  const uint16_t* rows = reinterpret_cast<const uint16_t*>(a.rows);
  const int d4 = (int)((a.dim + 3) / 4);
  for (uint32_t j0 = (uint32_t)wib * R; j0 < m; j0 += WAVES * R) {
    float acc[R];
    const uint32_t jn = j0 + (uint32_t)(lane & (R - 1));
    float vnorm = 1.0f;  // (requested with the rows: behind the reduction it is a second dependent round trip)
    if (METRIC == kCosine && lane < R && jn < m) vnorm = a.norms[nb_id[jn]];
    if (CPL > 0) {
      uint2 v[R][CPL > 0 ? CPL : 1];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t j = j0 + r < m ? j0 + r : m - 1;
        const uint16_t* p = rows + (size_t)nb_id[j] * a.row_stride + (size_t)lane * 4;
#pragma unroll
        for (int c = 0; c < CPL; c++) v[r][c] = ld_half4(p + c * 256);
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < CPL; c++) s = chain4<OP>(s, q[c], half4_to_f32<F16>(v[r][c]));
        acc[r] = s;
      }
    } else {
      const uint16_t* rp[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t j = j0 + r < m ? j0 + r : m - 1;
        rp[r] = rows + (size_t)nb_id[j] * a.row_stride;
        acc[r] = 0.0f;
      }
      for (int c = lane; c < d4; c += 64) {  // (4 * d4 <= row_stride: the last chunk's load stays inside the row)
        const float4 qq = ld4(qgen + c * 4);
        const int nv = (int)a.dim - c * 4;
#pragma unroll
        for (int r = 0; r < R; r++) {
          const float4 x = half4_to_f32<F16>(ld_half4(rp[r] + c * 4));
          acc[r] = nv >= 4 ? chain4<OP>(acc[r], qq, x) : chain4_tail<OP>(acc[r], qq, x, nv);
        }
      }
    }
    reduce_rows<R>(acc, lane);
    if (lane < R && jn < m) {
      float d;
      if (METRIC == kCosine) d = 1.0f - finish_score_half<kCosine>(acc[0], qnorm, vnorm);  // half_precision.rs:237-253
      else if (METRIC == kEuclidean) d = finish_score<kEuclidean>(acc[0], 0.0f, 0.0f);     // :257-287
      else d = -acc[0];                                                                    // :199-225
      nb_d[jn] = d;
    }
  }
}

template <int METRIC>
__device__ __forceinline__ void dist_phase_bits(const DistCtx& a, const uint32_t* qbits, uint32_t m,
                                                lds_vu32* nb_id, lds_vf32* nb_d, bool raw = false) {
  const uint32_t W = a.words;
  for (uint32_t t = threadIdx.x; t < m; t += 256) {
    const uint4* p = reinterpret_cast<const uint4*>(a.bits + (size_t)nb_id[t] * W);
    uint32_t ham = 0, inter = 0, uni = 0;
    for (uint32_t w = 0; w < W; w += 4) {
      const uint4 x = p[w / 4];
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t qq = qbits[w + e];
        if (METRIC == kHamming) {
          ham += __popc(xs[e] ^ qq);
        } else {
          inter += __popc(xs[e] & qq);
          uni += __popc(xs[e] | qq);
        }
      }
    }
    if (METRIC == kHamming) {
      nb_d[t] = (float)ham;  // simd_explicit.rs:234-287 on the exact re-encoding bit = (x > 0.5)
    } else {
      const float sim = (uni == 0) ? 1.0f : (float)inter / (float)uni;  // simd_explicit.rs:431-442
      nb_d[t] = raw ? sim : 1.0f - sim;                                  // native/distance.rs:83
    }
  }
}


// ---- the graph walk shared by the traversal kernels (hnsw_kernels.hip: f32 rows and packed bits; hnsw_half.hip: the f16 / bf16
// images): NativeHnsw::search, statement for statement — see the head of hnsw_kernels.hip.  DIST is the distance phase: it owns the
// query (registers, or the LDS scratch behind the lists for dimensions that are no multiple of 256) and evaluates nb_id[0..m) ->
// nb_d[0..m) with all waves of the block; everything else — phases, lists, visited set, counters, result mapping — is the same text
// for every row format, so the formats cannot drift apart.
enum WalkPhase : int {
  P_START = 0,   // evaluate dist(q, cur) on `layer`
  P_G_ENTRY,     // consume it as best_dist (graph.rs:407)
  P_G_LOAD,      // load neighbours of best (graph.rs:410)
  P_G_SCAN,      // scan them with strict < (graph.rs:413-421)
  P_G_DONE,      // no improvement: next layer down
  P_Z_ENTRY,     // layer 0: push the entry point (graph.rs:464-469)
  P_Z_POP,       // pop nearest candidate, termination test, gather unvisited neighbours (:471-499)
  P_Z_ADMIT,     // admission of the evaluated neighbours in list order (:500-511)
  P_FINISH,
  P_R_DONE       // rerank: raw scores of the candidates are in nb_d
};

// the f32 rows (Cosine / Euclidean / DotProduct, canonical arithmetic) and the packed bits (Hamming / Jaccard)
template <int METRIC, int CPL, int WAVES, int R>
struct WalkDistF32 {
  static constexpr bool UD = false;       // f32 distances, ordered as the reference's raw compares order them
  static constexpr bool RESCORE = false;  // the walk's own distances are the answer's
  static constexpr bool BITS = (METRIC == kHamming || METRIC == kJaccard);
  static constexpr int TPB = WAVES * 64;
  DistCtx dc;
  float* qgen;
  uint32_t* qbits;
  float4 q[CPL > 0 ? CPL : 1];
  float qnorm;
  __device__ __forceinline__ void init(const HnswSearchArgs& a, unsigned char* qscratch) {
    dc = DistCtx{a.rows, a.norms, a.bits, a.row_stride, a.dim, a.words};
    qgen = reinterpret_cast<float*>(qscratch);
    qbits = reinterpret_cast<uint32_t*>(qscratch);
  }
  // every thread of the block; the caller's barrier follows
  __device__ __forceinline__ void load_query(const float* qp, int lane) {
    const int d4 = (int)((dc.dim + 3) / 4);
    qnorm = 0.0f;
    if (BITS) {
      for (uint32_t w = threadIdx.x; w < dc.words; w += TPB) {
        uint32_t bitsw = 0;
        for (uint32_t e = 0; e < 32; e++) {
          const uint32_t i = w * 32 + e;
          if (i < dc.dim && qp[i] > 0.5f) bitsw |= 1u << e;
        }
        qbits[w] = bitsw;
      }
    } else if (CPL > 0) {
      float nacc = 0.0f;
#pragma unroll
      for (int c = 0; c < CPL; c++) {
        q[c] = ld4(qp + (size_t)(c * 64 + lane) * 4);
        nacc = chain4<kOpDot>(nacc, q[c], q[c]);
      }
      if (METRIC == kCosine) qnorm = sqrtf(butterfly_all(nacc));
    } else {
      const int qlen = d4 * 4;
      for (int i = threadIdx.x; i < qlen; i += TPB) qgen[i] = i < (int)dc.dim ? qp[i] : 0.0f;
      __syncthreads();
      if (METRIC == kCosine) {
        float nacc = 0.0f;
        for (int c = lane; c < d4; c += 64) {
          const float4 x = ld4(qgen + c * 4);
          const int nv = (int)dc.dim - c * 4;
          nacc = nv >= 4 ? chain4<kOpDot>(nacc, x, x) : chain4_tail<kOpDot>(nacc, x, x, nv);
        }
        qnorm = sqrtf(butterfly_all(nacc));
      }
    }
  }
  __device__ __forceinline__ void eval(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib, bool raw) const {
    if (BITS)
      dist_phase_bits<METRIC>(dc, qbits, m, nb_id, nb_d, raw);
    else
      dist_phase_f32<METRIC, CPL, WAVES, R>(dc, q, qnorm, qgen, m, nb_id, nb_d, lane, wib, raw);
  }
};

// the f16 / bf16 image of the rows (hnsw_half.hip): the query is rounded once here, the Cosine query norm is the canonical chain
// over the ROUNDED query
template <int METRIC, int CPL, int WAVES, int R, bool F16>
struct WalkDistHalf {
  static constexpr bool UD = false, RESCORE = false;
  static constexpr int TPB = WAVES * 64;
  DistCtx dc;  // rows = the image, row_stride in half elements, norms of the rounded rows
  float* qgen;
  float4 q[CPL > 0 ? CPL : 1];
  float qnorm;
  __device__ __forceinline__ void init(const HnswSearchArgs& a, unsigned char* qscratch) {
    dc = DistCtx{a.rows, a.norms, nullptr, a.row_stride, a.dim, 0};
    qgen = reinterpret_cast<float*>(qscratch);
  }
  __device__ __forceinline__ void load_query(const float* qp, int lane) {
    const int d4 = (int)((dc.dim + 3) / 4);
    qnorm = 0.0f;
    if (CPL > 0) {
      float nacc = 0.0f;
#pragma unroll
      for (int c = 0; c < CPL; c++) {
        q[c] = round_to_half4<F16>(ld4(qp + (size_t)(c * 64 + lane) * 4));
        nacc = chain4<kOpDot>(nacc, q[c], q[c]);
      }
      if (METRIC == kCosine) qnorm = sqrtf(butterfly_all(nacc));
    } else {
      const int qlen = d4 * 4;
      for (int i = threadIdx.x; i < qlen; i += TPB) qgen[i] = i < (int)dc.dim ? round_to_half<F16>(qp[i]) : 0.0f;
      __syncthreads();
      if (METRIC == kCosine) {
        float nacc = 0.0f;
        for (int c = lane; c < d4; c += 64) {
          const float4 x = ld4(qgen + c * 4);
          const int nv = (int)dc.dim - c * 4;
          nacc = nv >= 4 ? chain4<kOpDot>(nacc, x, x) : chain4_tail<kOpDot>(nacc, x, x, nv);
        }
        qnorm = sqrtf(butterfly_all(nacc));
      }
    }
  }
  __device__ __forceinline__ void eval(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib, bool) const {
    dist_phase_half<METRIC, CPL, WAVES, R, F16>(dc, q, qnorm, qgen, m, nb_id, nb_d, lane, wib);
  }
};

// the u8 codes of DualPrecisionHnsw (hnsw_int8.hip; the filtered walk of hnsw_filtered.hip): the query quantised once
// per query (quantizer.quantize(query), dual_precision.rs:235), every distance the integer L2^2 of dist_phase_int8 — a u32 bit
// pattern in nb_d, ordered as an integer (UD).  The walk ends with a re-score of its best candidates by the exact f32 engine
// distance (RESCORE): `exact` is the f32 phase, its query loaded only then (load_exact), so no f32 query register lives through the
// walk.  Query scratch: f32 query (generic dims) | code words [code_words] | re-score output [nbmax] u64 — hnsw_int8_lds_bytes.
// codes / min_vals / scales / cand_k are set by the kernel before init.
template <int METRIC, int CPL, int WAVES, int R>
struct WalkDistInt8 {
  static constexpr bool UD = true, RESCORE = true;
  static constexpr int TPB = WAVES * 64;
  static constexpr int QW = 4;  // code words per lane: dims up to 1024
  WalkDistF32<METRIC, CPL, WAVES, R> exact;
  CodeCtx codes;
  const float* min_vals;  // [dim]
  const float* scales;    // [dim]
  uint32_t cand_k;        // k * oversampling
  uint32_t* qcw;
  lds_vu64* outp;
  uint32_t qw[QW];
  uint32_t qsq;
  __device__ __forceinline__ void init(const HnswSearchArgs& a, unsigned char* qscratch) {
    exact.init(a, qscratch);
    const size_t qgen_bytes = CPL > 0 ? 0 : (size_t)((a.dim + 3) / 4) * 16;
    qcw = reinterpret_cast<uint32_t*>(qscratch + qgen_bytes);
    outp = (lds_vu64*)(lds_void_p)(qscratch + ((qgen_bytes + (size_t)codes.code_words * 4 + 15) & ~(size_t)15));
  }
  // every thread of the block; the caller's barrier follows
  __device__ __forceinline__ void load_query(const float* qp, int lane) {
    const uint32_t CW = codes.code_words, dim = exact.dc.dim;
    for (uint32_t w = threadIdx.x; w < CW; w += TPB) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t i = w * 4 + e;
        if (i < dim) {
          float v = roundf((qp[i] - min_vals[i]) * scales[i]);
          v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
          word |= ((v != v) ? 0u : (uint32_t)v) << (8 * e);
        }
      }
      qcw[w] = word;
    }
    __syncthreads();
    qsq = 0;
#pragma unroll
    for (int t = 0; t < QW; t++) {
      qw[t] = ((uint32_t)lane + 64u * t < CW) ? qcw[lane + 64 * t] : 0u;
      qsq = __builtin_amdgcn_udot4(qw[t], qw[t], qsq, false);
    }
    qsq = wave_sum_u32(qsq);
  }
  __device__ __forceinline__ void eval(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib, bool) const {
    dist_phase_int8<QW, WAVES>(codes, qw, qsq, m, nb_id, nb_d, lane, wib);
  }
  // the re-score: the f32 query (every thread of the block; the caller's barrier follows) and the exact engine distances
  __device__ __forceinline__ void load_exact(const float* qp, int lane) { exact.load_query(qp, lane); }
  __device__ __forceinline__ void eval_exact(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib) const {
    exact.eval(m, nb_id, nb_d, lane, wib, false);
  }
};

// the f16 / bf16 image for the walk and the f32 rows behind it (the filtered walk of hnsw_filtered.hip): every distance
// of the walk is WalkDistHalf's — the rounded query against the row's image, f32 values ordered by the raw compares — and the walk
// ends with a re-score of its best candidates by the exact f32 engine distance between the UNROUNDED query and the f32 row
// (RESCORE): `exact` is the f32 phase over a.rows / a.norms, its query loaded only then (load_exact), when the rounded one is dead —
// the two query register sets are never live together.  Query scratch: the query (generic dims: the rounded one during the walk,
// the unrounded one during the re-score) | re-score output [nbmax] u64 — hnsw_half_rescore_lds_bytes.
// image / image_norms / image_stride / cand_k are set by the kernel before init.
// R / RX: rows per group of the walk's phase and of the re-score's (neither changes a bit, reduce_rows).
template <int METRIC, int CPL, int WAVES, int R, bool F16, int RX = R>
struct WalkDistHalfRescore {
  static constexpr bool UD = false, RESCORE = true;
  WalkDistHalf<METRIC, CPL, WAVES, R, F16> walk;
  WalkDistF32<METRIC, CPL, WAVES, RX> exact;
  const float* image;        // [n][image_stride] half elements
  const float* image_norms;  // of the rounded rows
  uint32_t image_stride;     // in half elements
  uint32_t cand_k;           // k * oversampling
  lds_vu64* outp;
  __device__ __forceinline__ void init(const HnswSearchArgs& a, unsigned char* qscratch) {
    exact.init(a, qscratch);
    walk.dc = DistCtx{image, image_norms, nullptr, image_stride, a.dim, 0};
    walk.qgen = reinterpret_cast<float*>(qscratch);
    const size_t qgen_bytes = CPL > 0 ? 0 : (size_t)((a.dim + 3) / 4) * 16;
    outp = (lds_vu64*)(lds_void_p)(qscratch + qgen_bytes);
  }
  // every thread of the block; the caller's barrier follows
  __device__ __forceinline__ void load_query(const float* qp, int lane) { walk.load_query(qp, lane); }
  __device__ __forceinline__ void eval(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib, bool raw) const {
    walk.eval(m, nb_id, nb_d, lane, wib, raw);
  }
  // the re-score: the unrounded f32 query (every thread of the block, behind the barrier that ends the walk's last phase: the
  // generic-dimension scratch is rewritten; the caller's barrier follows) and the exact engine distances
  __device__ __forceinline__ void load_exact(const float* qp, int lane) { exact.load_query(qp, lane); }
  __device__ __forceinline__ void eval_exact(uint32_t m, lds_vu32* nb_id, lds_vf32* nb_d, int lane, int wib) const {
    exact.eval(m, nb_id, nb_d, lane, wib, false);
  }
};

template <int METRIC, int CPL, int NS, bool LAT, bool VIS, bool RAWEF, class DIST>
__device__ __forceinline__ void hnsw_walk_body(const HnswSearchArgs& a) {
  constexpr int WAVES = LAT ? 16 : 4, TPB = WAVES * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = (int)rfl(threadIdx.x >> 6);
  const uint32_t cap = a.cap, nbmax = a.nbmax;
  const uint32_t ef_launch = a.ef;
  uint32_t ef_query = a.ef;  // RAWEF only (wave-uniform)
#define ef (RAWEF ? ef_query : ef_launch)
  const auto [keys, nb_id, nb_d, ctl, flags, qscratch] = WalkLds(smem, cap, nbmax);

  uint32_t* vis = a.visited + (size_t)blockIdx.x * a.vis_words;
  uint32_t* vlog = a.vlog + (size_t)blockIdx.x * a.vlog_cap;
  // VIS: the exact visited set in LDS (zero between queries); a query stops with the overflow flag before it is 3/4 full
  const VisSet vs{reinterpret_cast<uint32_t*>(smem + a.vis_off), (1u << a.vis_log2) - 1u, 32u - a.vis_log2};
  const uint32_t vis_limit = VIS ? (3u << a.vis_log2) / 4u : 0xFFFFFFFFu;
  if (VIS) {
    vs.clear(threadIdx.x, TPB);
    __syncthreads();
  }
  DIST dist;
  dist.init(a, qscratch);

  for (uint32_t qi = blockIdx.x; qi < a.nq; qi += gridDim.x) {
    const float* qp = a.queries + (size_t)qi * a.q_stride;
    dist.load_query(qp, lane);
    __syncthreads();

    // ---- leader state (meaningful in wave 0 only; every value is wave-uniform) ----
    CandList<NS> list;
    list.init(keys, flags, cap);
    uint32_t n_dist = 0, n_expand = 0, logn = 0, overflow = 0, m_prev = 0, rr_m = 0;
    bool spec = false;        // LAT: the distance phase in flight evaluates ALL neighbours of the expanded node ...
    uint64_t spec_mask = 0;   // ... and these lanes' neighbours were unvisited (known behind that phase)
    // the neighbour list of the PREDICTED next pop — the nearest unexpanded candidate left behind by this pop — requested with this
    // pop's own list: when the admission puts nothing in front of it (most expansions once the beam has settled), the next pop finds
    // its ids in registers and the walk is one dependent memory round trip shorter.  A wrong guess costs 260 bytes.  Not counted:
    // n_dist / n_expand are what the reference's loop counts (graph.rs:471-511).
    uint32_t pf_node = 0xFFFFFFFFu, pf_nb = 0, pf_cnt = 0, pf_hits = 0;
    // (latency-mode instances only: the throughput instances sit at the 128-register line that lets four walks share a CU, and the
    // three registers this needs across the distance phase put 20 of theirs into scratch)
    const bool PF = LAT && a.pf_ids != 0;
    int phase = P_START;
    int layer = (int)a.max_layer;
    uint32_t cur = a.entry_point;
    float best_d = 0.0f;

    for (;;) {
      if (wib == 0) {
        bool ready = false;
        uint32_t m = 0, done = 0, raw = 0;
        while (!ready) {
          if (phase == P_START) {
            if (lane == 0) nb_id[0] = cur;
            m = 1;
            if (layer == 0 && a.extra_eps) {  // search_multi_entry: the drawn ids that are not yet entry points (graph.rs:335-338)
              uint32_t e0 = cur, e1 = 0xFFFFFFFFu, e2 = 0xFFFFFFFFu;
              for (uint32_t j = 0; j < 3; j++) {
                const uint32_t id = a.extra_eps[(size_t)qi * 3 + j];
                if (id == 0xFFFFFFFFu || id == e0 || id == e1 || id == e2) continue;
                if (lane == 0) nb_id[m] = id;
                if (m == 1) e1 = id; else e2 = id;  // (a third new id has nothing behind it to be compared with)
                m++;
              }
            }
            // graph.rs:463-468 pushes EVERY entry point into `results` with no cut, and graph.rs:503-509 pops at most one entry per
            // push: with more entry points than ef_search the result set simply stays at that size — which is what a search with
            // ef = the number of entry points does from its first step (results full from the start: same admission test
            // `dist < furthest`, same single pop, same stop rule `len >= ef`).  Only NativeHnsw-level calls get here with ef < m:
            // search_multi_entry with ef_search < 4 and several probes, or ef_search = 0 (which therefore acts as 1).
            if (RAWEF && layer == 0) ef_query = max(ef_launch, m);
            ready = true;
            phase = layer > 0 ? P_G_ENTRY : P_Z_ENTRY;
          } else if (phase == P_G_ENTRY) {
            best_d = rflf(nb_d[0]);
            n_dist += 1;
            phase = P_G_LOAD;
          } else if (phase == P_G_LOAD) {
            const HnswLayerRef L = a.layers[layer];
            uint32_t nc = rfl(L.cnt[cur]);
            nc = min(nc, min(L.stride, nbmax));
            for (uint32_t base = 0; base < nc; base += 64) {
              const uint32_t t = base + lane;
              if (t < nc) nb_id[t] = L.nbr[(size_t)cur * L.stride + t];
            }
            if (nc == 0) {
              phase = P_G_DONE;
            } else {
              m = nc;
              ready = true;
              phase = P_G_SCAN;
            }
          } else if (phase == P_G_SCAN) {
            n_dist += m_prev;
            const uint32_t besti = greedy_scan(nb_d, m_prev, best_d, lane);
            if (besti != 0xFFFFFFFFu) {
              cur = rfl(nb_id[besti]);
              best_d = rflf(nb_d[besti]);
              phase = P_G_LOAD;
            } else {
              phase = P_G_DONE;
            }
          } else if (phase == P_G_DONE) {
            layer -= 1;
            phase = P_START;
          } else if (phase == P_Z_ENTRY) {
            // graph.rs:463-468: every entry point is evaluated, pushed to both heaps and marked visited (one unless search_multi_entry)
            for (uint32_t t = 0; t < m_prev; t++) {
              const float d = rflf(nb_d[t]);
              const uint32_t ep = rfl(nb_id[t]);
              n_dist += 1;
              list.insert(make_key<false>(d, ep), lane, overflow);
              if (lane == 0) {
                if (VIS) {
                  (void)vs.test_and_set(ep);
                } else {
                  atomicOr(&vis[ep >> 5], 1u << (ep & 31));
                  if (a.vlog_cap) vlog[t] = ep;
                }
              }
            }
            logn = m_prev;
            phase = P_Z_POP;
          } else if (phase == P_Z_POP) {
            const uint32_t idx = list.first_unexpanded(lane);
            if (idx == kNoIndex) {
              phase = P_FINISH;  // candidates empty (graph.rs:471)
            } else {
              const uint64_t ckey = list.key_at(idx, lane);
              bool stop = false;
              if (list.size() >= ef) stop = key_dist(ckey) > key_dist(list.key_at(ef - 1, lane));  // graph.rs:474
              if (!stop && VIS && logn + nbmax > vis_limit) {  // the LDS set could pass 3/4: the caller re-runs on the bitmap
                overflow = 1;
                stop = true;
              }
              if (stop) {
                phase = P_FINISH;
              } else {
                list.mark_expanded(idx, lane);
                n_expand += 1;
                const uint32_t cnode = (uint32_t)ckey;
                const HnswLayerRef L = a.layers[0];
                // the neighbour ids are requested together with the count (one memory round trip instead of two)
                const uint32_t lim = min(L.stride, nbmax);
                uint32_t nb0 = 0, ncv = 0;
                if (PF && pf_node == cnode) {
                  nb0 = pf_nb;
                  ncv = pf_cnt;
                  pf_hits += 1;
                } else {
                  if ((uint32_t)lane < lim) nb0 = L.nbr[(size_t)cnode * L.stride + lane];
                  ncv = L.cnt[cnode];
                }
                uint32_t nc = rfl(ncv);
                nc = min(nc, lim);
                if (PF) {
                  // (behind the wait for this pop's own list: where the two paths above join, the compiler waits for EVERY load in
                  // flight — requested in front of that, the prediction's round trip was paid by every pop: 2 % slower than none)
                  const uint32_t idx2 = list.first_unexpanded(lane);
                  pf_node = 0xFFFFFFFFu;
                  if (idx2 != kNoIndex) {
                    pf_node = (uint32_t)list.key_at(idx2, lane);
                    if ((uint32_t)lane < lim) pf_nb = L.nbr[(size_t)pf_node * L.stride + lane];
                    pf_cnt = L.cnt[pf_node];
                  }
                }
                if (LAT && a.lat_spec) {  // (nc <= 64, host) every neighbour is evaluated; the visited verdicts follow with the distances
                  if ((uint32_t)lane < nc) nb_id[lane] = nb0;
                  m = nc;
                  spec = nc != 0;
                } else {
                for (uint32_t base = 0; base < nc; base += 64) {
                    const uint32_t t = base + lane;
                    const bool valid = t < nc;
                    uint32_t nb = nb0;
                    bool newly = false;
                    if (valid) {
                      if (base != 0) nb = L.nbr[(size_t)cnode * L.stride + t];
                      const uint32_t bit = 1u << (nb & 31);
                      newly = VIS ? vs.test_and_set(nb) : (atomicOr(&vis[nb >> 5], bit) & bit) == 0;  // visited.insert (graph.rs:499)
                    }
                    const uint64_t mask = __ballot(newly);
                    const uint32_t before = (uint32_t)__popcll(mask & lt_mask(lane));
                    if (newly) {
                      nb_id[m + before] = nb;
                      if (!VIS && logn + before < a.vlog_cap) vlog[logn + before] = nb;
                    }
                    m += (uint32_t)__popcll(mask);
                    logn += (uint32_t)__popcll(mask);
                  }
                }
                if (m != 0) {
                  ready = true;
                  phase = P_Z_ADMIT;
                }
              }
            }
          } else if (phase == P_Z_ADMIT) {
            if (LAT && a.lat_spec) {  // the unvisited ones of the evaluated neighbours, in list order: counters and the undo log
              n_dist += (uint32_t)__popcll(spec_mask);
              if (!VIS && (spec_mask >> lane & 1ull)) {
                const uint32_t pos = logn + (uint32_t)__popcll(spec_mask & lt_mask(lane));
                if (pos < a.vlog_cap) vlog[pos] = nb_id[lane];
              }
              logn += (uint32_t)__popcll(spec_mask);
            } else {
              n_dist += m_prev;
            }
            for (uint32_t base = 0; base < m_prev; base += 64) {
              const uint32_t t = base + lane;
              const float d = t < m_prev ? nb_d[t] : 0.0f;
              uint32_t size = list.size() < ef ? list.size() : ef;
              float far = key_dist(list.key_at(size - 1, lane));
              // pre-filter against the furthest distance at chunk start: it only decreases while the
              // result set is full, so a neighbour rejected now would be rejected at its turn too
              uint64_t mask = __ballot(t < m_prev && (d < far || size < ef));
              if (LAT && a.lat_spec) mask &= spec_mask;
              // two or more to admit: all at once (vdb_hnsw_device.hpp admit_batch) unless distances tie exactly
              if (NS > 0 && (mask & (mask - 1)) != 0ull &&
                  list.admit_batch(mask, d, t < m_prev ? nb_id[t] : 0u, lane, ef, keys, flags))
                mask = 0ull;
              while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float dj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(d), src));
                size = list.size() < ef ? list.size() : ef;
                far = key_dist(list.key_at(size - 1, lane));
                if (dj < far || size < ef) {  // graph.rs:503
                  const uint32_t nbj = nb_id[base + src];
                  list.insert(make_key<false>(dj, nbj), lane, overflow);
                  list.truncate(ef, lane);
                }
              }
            }
            phase = P_Z_POP;
          } else if (phase == P_FINISH) {
            if (a.rerank_k == 0) {
              done = 1;
              ready = true;
            } else {
              // search_with_rerank (search.rs:118-160): candidates = the search result for k = rerank_k (soft-deleted
              // rows dropped, search.rs:86-91); their rows are re-scored with the raw compute_distance
              const uint32_t size = list.size() < ef ? list.size() : ef;
              const uint32_t kk = a.rerank_k < size ? a.rerank_k : size;
              for (uint32_t base = 0; base < kk; base += 64) {
                const uint32_t e = base + lane;
                const bool v = e < kk;
                const uint32_t node = v ? (uint32_t)list.chunk_key(base, lane) : 0;
                bool al = v;
                if (v && a.alive) al = a.alive[node] != 0;
                const uint64_t mask = __ballot(al);
                if (al) nb_id[m + (uint32_t)__popcll(mask & lt_mask(lane))] = node;
                m += (uint32_t)__popcll(mask);
              }
              raw = 1;
              rr_m = m;
              phase = P_R_DONE;
              if (m == 0) done = 1;
              ready = true;
            }
          } else {  // P_R_DONE
            done = 1;
            ready = true;
          }
        }
        if (lane == 0) {
          ctl[0] = m;
          ctl[1] = done;
          ctl[2] = logn;
          ctl[3] = raw;
        }
        m_prev = m;
      }
      __syncthreads();
      const uint32_t m = ctl[0];
      if (ctl[1]) break;
      const bool raw = ctl[3] != 0;
      uint32_t spec_old = 0, spec_bit = 0;
      const bool spec_lane = LAT && wib == 0 && spec && (uint32_t)lane < m;
      if (spec_lane) {  // visited.insert (graph.rs:499) for every neighbour, in flight beside the row fetches below
        const uint32_t nb = nb_id[lane];
        spec_bit = 1u << (nb & 31);
        spec_old = VIS ? (vs.test_and_set(nb) ? 0u : spec_bit) : atomicOr(&vis[nb >> 5], spec_bit);
      }
      dist.eval(m, nb_id, nb_d, lane, wib, raw);
      if (LAT && wib == 0) {
        spec_mask = spec ? __ballot(spec_lane && (spec_old & spec_bit) == 0) : 0ull;
        spec = false;
      }
      __syncthreads();
    }

    // ---- rerank results: stable sort of the re-scored candidates in the metric's order (distance.rs:95-103),
    // cut to k.  sort key = (order-key(score) << 32 | candidate position): unique, rank = #smaller keys ----
    if (a.rerank_k != 0) {
      if (wib == 0) {
        const uint32_t m = rr_m;  // candidates re-scored in the last distance phase (0 if none)
        constexpr bool HIB = higher_is_better(METRIC);
        const uint32_t outn = m < a.k ? m : a.k;
        for (uint32_t i = lane; i < m; i += 64) keys[i] = make_key<HIB>(nb_d[i], i);
        for (uint32_t i = lane; i < m; i += 64) {
          const uint64_t mine = keys[i];
          uint32_t rank = 0;
          for (uint32_t j = 0; j < m; j++) rank += keys[j] < mine ? 1u : 0u;
          if (rank < a.k) {
            const uint32_t node = nb_id[i];
            a.out_ids[(size_t)qi * a.k + rank] = a.ext_ids ? a.ext_ids[node] : (uint64_t)node;
            a.out_scores[(size_t)qi * a.k + rank] = nb_d[i];
          }
        }
        for (uint32_t e = outn + lane; e < a.k; e += 64) {
          a.out_ids[(size_t)qi * a.k + e] = ~0ull;
          a.out_scores[(size_t)qi * a.k + e] = __uint_as_float(0x7FC00000u);
        }
        if (lane == 0) {
          a.out_n[qi] = overflow ? 0xFFFFFFFFu : outn;
          if (a.stats) {
            atomicAdd(&a.stats[0], (unsigned long long)n_dist);
            atomicAdd(&a.stats[1], (unsigned long long)n_expand);
            if (pf_hits) atomicAdd(&a.stats[2], (unsigned long long)pf_hits);
          }
        }
      }
    } else
    // ---- results: first k of the sorted result set, soft-deleted rows dropped after the cut
    // (search.rs:86-91), scores through transform_score ----
    if (wib == 0) {
      const uint32_t size = list.size() < ef ? list.size() : ef;
      const uint32_t kk = a.k < size ? a.k : size;
      uint32_t outn = 0;
      for (uint32_t base = 0; base < kk; base += 64) {
        const uint32_t e = base + lane;
        const bool v = e < kk;
        const uint64_t key = v ? list.chunk_key(base, lane) : 0;
        const uint32_t node = (uint32_t)key;
        bool al = v;
        if (v && a.alive) al = a.alive[node] != 0;
        const uint64_t mask = __ballot(al);
        const uint32_t p = outn + (uint32_t)__popcll(mask & lt_mask(lane));
        if (al) {
          a.out_ids[(size_t)qi * a.k + p] = a.ext_ids ? a.ext_ids[node] : (uint64_t)node;
          a.out_scores[(size_t)qi * a.k + p] = transform_score_dev(METRIC, key_dist(key));
        }
        outn += (uint32_t)__popcll(mask);
      }
      for (uint32_t e = outn + lane; e < a.k; e += 64) {
        a.out_ids[(size_t)qi * a.k + e] = ~0ull;
        a.out_scores[(size_t)qi * a.k + e] = __uint_as_float(0x7FC00000u);
      }
      if (lane == 0) {
        a.out_n[qi] = overflow ? 0xFFFFFFFFu : outn;
        if (a.stats) {
          atomicAdd(&a.stats[0], (unsigned long long)n_dist);
          atomicAdd(&a.stats[1], (unsigned long long)n_expand);
          if (pf_hits) atomicAdd(&a.stats[2], (unsigned long long)pf_hits);
        }
      }
    }
    // ---- undo the visited bits of this query ----
    const uint32_t nlog = ctl[2];
    if (VIS) {
      __syncthreads();  // (ctl[2] read by everybody before the next query's leader rewrites it)
      vs.clear(threadIdx.x, TPB);
    } else if (nlog <= a.vlog_cap) {
      for (uint32_t i = threadIdx.x; i < nlog; i += TPB) vis[vlog[i] >> 5] = 0;
    } else {
      for (uint64_t i = threadIdx.x; i < a.vis_words; i += TPB) vis[i] = 0;
    }
    __syncthreads();
  }
#undef ef
}

}  // namespace vdb
