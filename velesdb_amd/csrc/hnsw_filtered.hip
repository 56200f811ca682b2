// hnsw_filtered.hip — filtered graph search (vdb_hip_index_search_graph_filtered / _filters): NativeHnsw::search
// (native/graph.rs:251-270) with an id allow-list consulted where a node enters the RESULT set.
//
// Semantics.  allowed(r) = r < the filter's row count, its bit r set, row r alive now.  The greedy descent (graph.rs:405-428) is
// unchanged: rejected nodes navigate.  Layer 0 is search_layer (graph.rs:438-520) with one change — `results` receives allowed
// nodes only; `candidates` and `visited` receive what they receive today.  With every row allowed this IS VDB_SEARCH_HNSW: ids,
// score bits, out_n, n_dist and n_expand.
//
// Single-list form.  The sorted LDS list of hnsw_walk_body (vdb_hnsw_device.hpp) holds candidates and results together; the flag
// byte of an entry gets a second bit, "allowed", set at insert from the filter bitmap AND the alive flags (one dword load per
// admitted neighbour).  results = the first ef allowed entries; the ef-th one is the PIVOT: `furthest` is its distance,
// "results.len() < ef" is "no pivot".  Behind an insert the entries whose distance is greater than the pivot's are dropped (ties
// stay, list_truncate's raw compare): whatever the reference pops behind them fails graph.rs:474 at once.  Nothing is dropped while
// there is no pivot — so a selective filter makes the list long, and it is bounded: an entry that falls off a full list and that
// the two-heap form still needs (an unexpanded candidate; or an allowed entry while the results are not full) sets the overflow
// flag, the query finishes anyway and reports out_n = 0xFFFFFFFF; the host re-runs it with more room or answers it exactly.
//
// filters_rank_kernel is that exact answer: top-k of the allowed live rows by (total-order(distance), row), the distances from the
// walk's own DIST::eval — bit for bit what the walk reports for the same row.
//
// One kernel family, one host path.  hnsw_search_filters_kernel / filters_rank_kernel take every query's filter from a per-slot
// descriptor (vdb_hip_index_search_graph_filters, DESIGN 4.1i: one filter per query); a launch's LDS layout follows its PHYSICAL
// list capacity, every query's list logic its own LOGICAL one, so queries with lists of different sizes share launches and each
// computes what it computes alone.  The one-filter call (vdb_hip_index_search_graph_filtered) is that path with a table of one
// filter and every query on it: search_graph_filtered_to_device at the end of the file.
//
// Over the half-precision images (vdb_hip_index_search_graph_filters_half): hnsw_search_filters_half_kernel /
// filters_rank_half_kernel are the same two bodies with the half walk's distance phase (WalkDistHalf,
// hnsw_half.hip) — the query rounded to the precision against the row's f16 / bf16 image, n_dist * (2 * stride [+ 4 Cosine]) row bytes.
//
// Over the u8 codes of the trained scalar quantiser (vdb_hip_index_search_graph_filters_int8):
// hnsw_search_filters_int8_kernel is the walk body with WalkDistInt8 — integer distances, ordered as integers (DIST::UD), ef widened
// over k * oversampling — and, behind the walk, the re-score of the k * oversampling best allowed candidates by the exact f32 engine
// distance (DIST::RESCORE), as hnsw_search_int8_kernel (hnsw_int8.hip) ends; its exact pass is filters_rank_kernel itself.
//
// Over a half image with exact answers (vdb_hip_index_search_graph_filters_half_rescore):
// hnsw_search_filters_half_rescore_kernel is the walk body with WalkDistHalfRescore — the half walk's distances over the image at ef
// widened over k * oversampling, then the same re-score over the f32 rows with the unrounded query; its exact pass is
// filters_rank_kernel itself, so a row has the same score bits on either route.
//
// Algorithmic HBM bytes per query: walk n_dist * dim * 4 + n_expand * M0 * 4 + (admitted neighbours) * 4 for the bitmap words;
// exact pass matched * (dim * 4 + 4).  Measured once, at one shape, f16 beside f32: tools/filter_probe.py has the graph leg.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vdb_filter_route.hpp"
#include "vdb_hnsw_device.hpp"
#include "vdb_index.hpp"
#include "vdb_walk_launch.hpp"

namespace vdb {

// The filters of a call: a table of n_filters + 1 descriptors — the last one is "no filter": null bitmap and list, rows = count = the
// index's rows now — and one FiltersSlot (vdb_filter_route.hpp) per launch slot
struct FilterDesc {
  const uint32_t* bitmap;
  const uint32_t* list;
  uint32_t rows, count;
};
struct HnswFiltersArgs {
  HnswSearchArgs s;           // (s.nq = the slots of THIS launch; s.cap = its PHYSICAL list capacity: the LDS layout)
  const FilterDesc* descs;    // [n_filters + 1]
  const FiltersSlot* slots;   // [s.nq]
  unsigned long long* qstats; // [nq][2]: the walk WRITES a query's n_dist / n_expand, the exact pass ADDS its rows to n_dist
};

constexpr uint32_t kFlagExpanded = 1u, kFlagAllowed = 2u;

// What a workgroup knows about the query of its launch slot: the filter, the query's index in the call and the LOGICAL capacity of
// its list (<= the launch's physical s.cap; all list logic of the query runs on it).  Every field is wave-uniform.
// (the two arrays as global-memory pointers by type: a pointer that was LOADED — the descriptor's — is a generic one to the
// compiler, and reads through it would take the flat path)
typedef const __attribute__((address_space(1))) uint32_t* glb_u32_p;
struct SlotFilter {
  glb_u32_p bitmap;
  glb_u32_p list;
  uint32_t rows, count, qi, cap;
};
__device__ __forceinline__ glb_u32_p uniform_ptr(const uint32_t* p) {
  const uint64_t v = (uint64_t)p;
  return (glb_u32_p)(((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | (uint64_t)rfl((uint32_t)v));
}
// the slot's descriptor, loaded once per query into scalar registers (rfl as for wib): the per-neighbour bitmap test stays one dword
// load from a scalar base.  A null bitmap / list = every row below `rows`.
__device__ __forceinline__ SlotFilter load_slot_filter(const HnswFiltersArgs& fa, uint32_t slot) {
  const FiltersSlot s = fa.slots[slot];
  const uint32_t fi = rfl(s.filter);
  const FilterDesc d = fa.descs[fi];
  SlotFilter f;
  f.bitmap = uniform_ptr(d.bitmap);
  f.list = uniform_ptr(d.list);
  f.rows = rfl(d.rows);
  f.count = rfl(d.count);
  f.qi = rfl(s.query);
  f.cap = min(rfl(s.cap), fa.s.cap);  // (never past the layout, whatever the table says)
  return f;
}

// list_insert (vdb_hnsw_device.hpp) with the new entry's flag given and the lost entry reported: lost = 1 when an entry fell off
// (the key itself when it sorts behind a full list), lost_flag = its flags
__device__ __forceinline__ void flist_insert(lds_vu64* keys, lds_vu8* flags, uint32_t& cnt, uint32_t cap, uint64_t key, uint32_t flag,
                                             int lane, uint32_t& lost, uint32_t& lost_flag) {
  lost = 0;
  lost_flag = 0;
  uint32_t pos = 0;
  for (uint32_t c = 0; c < cnt; c += 64) {
    const uint32_t e = c + lane;
    const bool less = e < cnt && keys[e] < key;
    pos += (uint32_t)__popcll(__ballot(less));
  }
  if (pos >= cap) {
    lost = 1;
    lost_flag = flag;
    return;
  }
  if (cnt == cap) {
    lost = 1;
    lost_flag = flags[cap - 1];
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
    flags[pos] = (uint8_t)flag;
  }
  cnt = newcnt;
}

// position of the ef-th allowed entry (ef >= 1), kNoIndex while there are fewer
__device__ __forceinline__ uint32_t find_pivot(lds_vu8* flags, uint32_t cnt, uint32_t ef, int lane) {
  uint32_t seen = 0;
  for (uint32_t c = 0; c < cnt; c += 64) {
    const uint32_t e = c + lane;
    const uint64_t m = __ballot(e < cnt && (flags[e] & kFlagAllowed) != 0);
    const uint32_t n = (uint32_t)__popcll(m);
    if (seen + n >= ef) {
      const uint32_t need = ef - seen - 1;  // set bits in front of the one we want
      const uint64_t hit = __ballot(((m >> lane) & 1ull) != 0 && (uint32_t)__popcll(m & lt_mask(lane)) == need);
      return c + (uint32_t)__ffsll((long long)hit) - 1;
    }
    seen += n;
  }
  return kNoIndex;
}

// entries behind the pivot stay only up to the last one whose distance is not greater than the pivot's (UD: key_dist_gt's domain)
template <bool UD>
__device__ __forceinline__ void pivot_truncate(lds_vu64* keys, uint32_t& cnt, uint32_t pivot, int lane) {
  if (pivot == kNoIndex || cnt <= pivot + 1) return;
  const uint64_t wk = keys[pivot];
  uint32_t last = pivot;
  for (uint32_t c = pivot + 1; c < cnt; c += 64) {
    const uint32_t e = c + lane;
    const bool stay = e < cnt && !key_dist_gt<UD>(keys[e], wk);  // negation of graph.rs:474's raw compare
    const uint64_t mask = __ballot(stay);
    if (mask) last = c + 63u - (uint32_t)__clzll((long long)mask);
  }
  cnt = last + 1;
}

__device__ __forceinline__ uint32_t row_allowed(const SlotFilter& f, const uint8_t* alive, uint32_t r) {  // r wave-uniform
  if (r >= f.rows) return 0u;
  if (f.bitmap != nullptr && ((f.bitmap[r >> 5] >> (r & 31)) & 1u) == 0u) return 0u;
  if (alive && alive[r] == 0) return 0u;
  return kFlagAllowed;
}

// R rows per wave and distance step: 8; 4 at four 256-dimension chunks per lane and for Euclidean at three (the half walk's lever,
// hnsw_half.hip: with 8 the Euclidean 768-dimension walk kept 20 bytes per lane in scratch memory; the group size does not change
// a bit, reduce_rows)
template <int METRIC, int CPL>
using FiltDist = WalkDistF32<METRIC, CPL, 4, ((CPL == 4 || (CPL == 3 && METRIC == kEuclidean)) ? 4 : 8)>;
// ... and over the f16 / bf16 image (vdb_hip_index_search_graph_filters_half): the half walk's distance phase
// (hnsw_half.hip) under the same two bodies.  A row group holds R x CPL x 2 registers, half of FiltDist's: 8 rows everywhere but
// at four chunks per lane, hnsw_half.hip's own rule (DESIGN 4.1k has the resource table)
template <int METRIC, int CPL>
constexpr int kFiltHalfRows = (CPL == 4 ? 4 : 8);
template <int METRIC, int CPL, bool F16>
using FiltDistHalf = WalkDistHalf<METRIC, CPL, 4, kFiltHalfRows<METRIC, CPL>, F16>;
// ... and over the u8 codes (vdb_hip_index_search_graph_filters_int8): dist_phase_int8 for the walk; the re-score is
// one FiltDist phase, so a row has the score bits the f32 exact pass gives it
template <int METRIC, int CPL>
using FiltDistInt8 = WalkDistInt8<METRIC, CPL, 4, ((CPL == 4 || (CPL == 3 && METRIC == kEuclidean)) ? 4 : 8)>;
// ... and over the f16 / bf16 image with the re-score over the f32 rows (vdb_hip_index_search_graph_filters_half_rescore):
// FiltDistHalf's phase for the walk with its rows per group, and one f32 phase (FiltDist's arithmetic) for the re-score at 4 rows
// per group: the re-score is one phase per query, and with 8 rows the bf16 Cosine 768-dimension instance spilled 13 vector registers
// and the generic Euclidean / DotProduct ones reserved 36 bytes of scratch per lane (the group size does not change a bit)
template <int METRIC, int CPL, bool F16>
using FiltDistHalfRescore = WalkDistHalfRescore<METRIC, CPL, 4, kFiltHalfRows<METRIC, CPL>, F16, 4>;

// The walk of the kernel families below (LDS: WalkLds, vdb_hnsw_device.hpp); DIST says which rows the distances are taken over, in
// which domain they are ordered (DIST::UD: f32 raw compares, or the int8 walk's integers — walk_key / key_bound / dist_lt /
// key_dist_gt / greedy_scan, vdb_hnsw_device.hpp) and whether the best candidates are re-scored behind the walk (DIST::RESCORE).
// `dist` arrives with whatever its init cannot take from HnswSearchArgs already set.
template <int METRIC, int CPL, class DIST>
__device__ __forceinline__ void filtered_walk_body(const HnswFiltersArgs& fa, DIST& dist) {
  constexpr bool UD = DIST::UD;
  const HnswSearchArgs& a = fa.s;
  unsigned long long* qstats = fa.qstats;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = (int)rfl(threadIdx.x >> 6);
  const uint32_t cap = a.cap, nbmax = a.nbmax, ef = a.ef;  // cap: the launch's physical capacity, the layout only
  const auto [keys, nb_id, nb_d, ctl, flags, qscratch] = WalkLds(smem, cap, nbmax);
  uint32_t* vis = a.visited + (size_t)blockIdx.x * a.vis_words;
  uint32_t* vlog = a.vlog + (size_t)blockIdx.x * a.vlog_cap;
  dist.init(a, qscratch);

  for (uint32_t slot = blockIdx.x; slot < a.nq; slot += gridDim.x) {
    const SlotFilter f = load_slot_filter(fa, slot);
    const uint32_t qi = f.qi;
    dist.load_query(a.queries + (size_t)qi * a.q_stride, lane);
    __syncthreads();

    // ---- leader state (wave 0; wave-uniform) ----
    uint32_t cnt = 0, pivot = kNoIndex;
    uint32_t n_dist = 0, n_expand = 0, logn = 0, overflow = 0, m_prev = 0;
    int phase = P_START;
    int layer = (int)a.max_layer;
    uint32_t cur = a.entry_point;
    float best_d = 0.0f;

    // one admitted node: flag, insert, pivot, what fell off, truncation
    // (keys = keys: a structured binding cannot be captured in C++17)
    auto admit = [&, keys = keys, flags = flags](float d, uint32_t node) {
      uint32_t lost, lost_flag;
      flist_insert(keys, flags, cnt, f.cap, walk_key<UD>(d, node), row_allowed(f, a.alive, node), lane, lost, lost_flag);
      pivot = find_pivot(flags, cnt, ef, lane);
      if (lost && ((lost_flag & kFlagExpanded) == 0 || ((lost_flag & kFlagAllowed) != 0 && pivot == kNoIndex))) overflow = 1;
      pivot_truncate<UD>(keys, cnt, pivot, lane);
    };

    for (;;) {
      if (wib == 0) {
        bool ready = false;
        uint32_t m = 0, done = 0;
        while (!ready) {
          if (phase == P_START) {
            if (lane == 0) nb_id[0] = cur;
            m = 1;
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
            const uint32_t besti = greedy_scan<UD>(nb_d, m_prev, best_d, lane);
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
            // graph.rs:463-468: the entry point is evaluated, pushed to candidates, marked visited — and to results only if allowed
            const float d = rflf(nb_d[0]);
            const uint32_t ep = rfl(nb_id[0]);
            n_dist += 1;
            admit(d, ep);
            if (lane == 0) {
              atomicOr(&vis[ep >> 5], 1u << (ep & 31));
              if (a.vlog_cap) vlog[0] = ep;
            }
            logn = 1;
            phase = P_Z_POP;
          } else if (phase == P_Z_POP) {
            uint32_t idx = kNoIndex;
            for (uint32_t c = 0; c < cnt; c += 64) {
              const uint32_t e = c + lane;
              const uint64_t un = __ballot(e < cnt && (flags[e] & kFlagExpanded) == 0);
              if (un) {
                idx = c + (uint32_t)__ffsll((long long)un) - 1;
                break;
              }
            }
            if (idx == kNoIndex) {
              phase = P_FINISH;  // candidates empty (graph.rs:471)
            } else {
              const uint64_t ckey = keys[idx];
              // graph.rs:474 with furthest = the pivot's distance and results.len() >= ef = "there is a pivot"
              if (pivot != kNoIndex && key_dist_gt<UD>(ckey, keys[pivot])) {
                phase = P_FINISH;
              } else {
                if (lane == 0) flags[idx] = (uint8_t)(flags[idx] | kFlagExpanded);
                n_expand += 1;
                const uint32_t cnode = (uint32_t)ckey;
                const HnswLayerRef L = a.layers[0];
                const uint32_t lim = min(L.stride, nbmax);
                uint32_t nc = rfl(L.cnt[cnode]);
                nc = min(nc, lim);
                for (uint32_t base = 0; base < nc; base += 64) {
                  const uint32_t t = base + lane;
                  const bool valid = t < nc;
                  uint32_t nb = 0;
                  bool newly = false;
                  if (valid) {
                    nb = L.nbr[(size_t)cnode * L.stride + t];
                    const uint32_t bit = 1u << (nb & 31);
                    newly = (atomicOr(&vis[nb >> 5], bit) & bit) == 0;  // visited.insert (graph.rs:499)
                  }
                  const uint64_t mask = __ballot(newly);
                  const uint32_t before = (uint32_t)__popcll(mask & lt_mask(lane));
                  if (newly) {
                    nb_id[m + before] = nb;  // (m + before < nc <= nbmax)
                    if (logn + before < a.vlog_cap) vlog[logn + before] = nb;
                  }
                  m += (uint32_t)__popcll(mask);
                  logn += (uint32_t)__popcll(mask);
                }
                if (m != 0) {
                  ready = true;
                  phase = P_Z_ADMIT;
                }
              }
            }
          } else if (phase == P_Z_ADMIT) {
            n_dist += m_prev;
            for (uint32_t base = 0; base < m_prev; base += 64) {
              const uint32_t t = base + lane;
              const float d = t < m_prev ? nb_d[t] : 0.0f;
              // pre-filter against the bound at chunk start: it only falls while the result set is full (there is a pivot), so a
              // neighbour rejected now would be rejected at its turn too
              const float far0 = pivot != kNoIndex ? key_bound<UD>(keys[pivot]) : 0.0f;
              uint64_t mask = __ballot(t < m_prev && (pivot == kNoIndex || dist_lt<UD>(d, far0)));
              while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float dj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(d), src));
                if (pivot == kNoIndex || dist_lt<UD>(dj, key_bound<UD>(keys[pivot]))) admit(dj, nb_id[base + src]);  // graph.rs:503
              }
            }
            phase = P_Z_POP;
          } else {  // P_FINISH
            done = 1;
            ready = true;
          }
        }
        if (lane == 0) {
          ctl[0] = m;
          ctl[1] = done;
          ctl[2] = logn;
        }
        m_prev = m;
      }
      __syncthreads();
      const uint32_t m = ctl[0];
      if (ctl[1]) break;
      dist.eval(m, nb_id, nb_d, lane, wib, false);
      __syncthreads();
    }

    if constexpr (DIST::RESCORE) {
      // ---- re-score (dual_precision.rs:377-383, 267-281): the coarse candidates = the first min(cand_k, allowed) allowed entries in
      // list order; their exact f32 engine distances in one phase (the f32 query is loaded only now); a stable sort by total_cmp —
      // sort key = (total-order(dist) << 32 | coarse position), unique, rank = the smaller keys — and the cut to k.  No alive test:
      // allowed means alive.  n_dist does not count these rows (hnsw_search_int8_kernel does not either). ----
      if (wib == 0) {
        const uint32_t want = min(dist.cand_k, nbmax);  // (the host rounds nbmax over cand_k)
        uint32_t rr = 0;
        for (uint32_t base = 0; base < cnt && rr < want; base += 64) {
          const uint32_t e = base + lane;
          const bool al = e < cnt && (flags[e] & kFlagAllowed) != 0;
          const uint64_t mask = __ballot(al);
          const uint32_t p = rr + (uint32_t)__popcll(mask & lt_mask(lane));
          if (al && p < want) nb_id[p] = (uint32_t)keys[e];
          rr = min(want, rr + (uint32_t)__popcll(mask));
        }
        if (lane == 0) ctl[3] = rr;
      }
      dist.load_exact(a.queries + (size_t)qi * a.q_stride, lane);
      __syncthreads();
      const uint32_t m = ctl[3];
      dist.eval_exact(m, nb_id, nb_d, lane, wib);
      __syncthreads();
      if (wib == 0) {
        lds_vu64* outp = dist.outp;
        for (uint32_t i = lane; i < m; i += 64) keys[i] = make_key<false>(nb_d[i], i);  // (m <= cnt: the list has the room)
        for (uint32_t i = lane; i < m; i += 64) {
          const uint64_t mine = keys[i];
          uint32_t rank = 0;
          for (uint32_t j = 0; j < m; j++) rank += keys[j] < mine ? 1u : 0u;
          outp[rank] = ((uint64_t)nb_id[i] << 32) | (uint64_t)__float_as_uint(nb_d[i]);  // (rank < m <= nbmax)
        }
        const uint32_t outn = m < a.k ? m : a.k;
        for (uint32_t e = lane; e < outn; e += 64) {
          const uint64_t pk = outp[e];
          const uint32_t node = (uint32_t)(pk >> 32);
          a.out_ids[(size_t)qi * a.k + e] = a.ext_ids ? a.ext_ids[node] : (uint64_t)node;
          a.out_scores[(size_t)qi * a.k + e] = transform_score_dev(METRIC, __uint_as_float((uint32_t)pk));
        }
        for (uint32_t e = outn + lane; e < a.k; e += 64) {
          a.out_ids[(size_t)qi * a.k + e] = ~0ull;
          a.out_scores[(size_t)qi * a.k + e] = __uint_as_float(0x7FC00000u);
        }
        if (lane == 0) {
          a.out_n[qi] = overflow ? 0xFFFFFFFFu : outn;
          qstats[(size_t)qi * 2] = n_dist;
          qstats[(size_t)qi * 2 + 1] = n_expand;
        }
      }
    } else
    // ---- results: the first k allowed entries in list order (all of them are alive: the flag says so), scores through
    // transform_score; NaN / ~0 padding and out_n as the unfiltered walk ----
    if (wib == 0) {
      uint32_t outn = 0;
      for (uint32_t base = 0; base < cnt && outn < a.k; base += 64) {
        const uint32_t e = base + lane;
        const bool al = e < cnt && (flags[e] & kFlagAllowed) != 0;
        const uint64_t mask = __ballot(al);
        const uint32_t p = outn + (uint32_t)__popcll(mask & lt_mask(lane));
        if (al && p < a.k) {
          const uint64_t key = keys[e];
          const uint32_t node = (uint32_t)key;
          a.out_ids[(size_t)qi * a.k + p] = a.ext_ids ? a.ext_ids[node] : (uint64_t)node;
          a.out_scores[(size_t)qi * a.k + p] = transform_score_dev(METRIC, key_dist(key));
        }
        outn = min(a.k, outn + (uint32_t)__popcll(mask));
      }
      for (uint32_t e = outn + lane; e < a.k; e += 64) {
        a.out_ids[(size_t)qi * a.k + e] = ~0ull;
        a.out_scores[(size_t)qi * a.k + e] = __uint_as_float(0x7FC00000u);
      }
      if (lane == 0) {
        a.out_n[qi] = overflow ? 0xFFFFFFFFu : outn;
        qstats[(size_t)qi * 2] = n_dist;
        qstats[(size_t)qi * 2 + 1] = n_expand;
      }
    }
    // ---- undo the visited bits of this query ----
    const uint32_t nlog = ctl[2];
    if (nlog <= a.vlog_cap) {
      for (uint32_t i = threadIdx.x; i < nlog; i += 256) vis[vlog[i] >> 5] = 0;
    } else {
      for (uint64_t i = threadIdx.x; i < a.vis_words; i += 256) vis[i] = 0;
    }
    __syncthreads();
  }
}

template <int METRIC, int CPL>
__global__ __launch_bounds__(256, 4) void hnsw_search_filters_kernel(HnswFiltersArgs fa) {
  FiltDist<METRIC, CPL> dist;
  filtered_walk_body<METRIC, CPL>(fa, dist);
}
// ... over the half image: a.rows = the image, a.row_stride in half elements, a.norms of the rounded rows; the queries stay f32 and
// are rounded at load
template <int METRIC, int CPL, bool F16>
__global__ __launch_bounds__(256, 4) void hnsw_search_filters_half_kernel(HnswFiltersArgs fa) {
  FiltDistHalf<METRIC, CPL, F16> dist;
  filtered_walk_body<METRIC, CPL>(fa, dist);
}
// ... over the u8 codes of DualPrecisionHnsw (vdb_hip_index_search_graph_filters_int8): the same body with the int8
// walk's integer distances (WalkDistInt8: ordered as integers) and the re-score of the k * oversampling best allowed candidates by the
// exact f32 engine distance behind it.  a.rows / a.norms stay the f32 rows (the re-score); a.ef = max(ef_search, k * oversampling).
struct HnswFiltersInt8Args {
  HnswFiltersArgs f;
  CodeCtx codes;
  const float* min_vals;  // [dim]
  const float* scales;    // [dim]
  uint32_t cand_k;        // k * oversampling (<= f.s.nbmax)
};
template <int METRIC, int CPL>
__global__ __launch_bounds__(256, 4) void hnsw_search_filters_int8_kernel(HnswFiltersInt8Args A) {
  FiltDistInt8<METRIC, CPL> dist;
  dist.codes = A.codes;
  dist.min_vals = A.min_vals;
  dist.scales = A.scales;
  dist.cand_k = A.cand_k;
  filtered_walk_body<METRIC, CPL>(A.f, dist);
}
// ... over the f16 / bf16 image with exact f32 answers (vdb_hip_index_search_graph_filters_half_rescore): the same body
// with the half walk's distances over the image and the re-score of the k * oversampling best allowed candidates over the f32 rows
// behind it.  a.rows / a.norms / a.row_stride stay the f32 rows (the re-score); a.ef = max(ef_search, k * oversampling).
struct HnswFiltersHalfRescoreArgs {
  HnswFiltersArgs f;
  const float* image;        // the f16 / bf16 image of the rows, [n][image_stride] half elements
  const float* image_norms;  // [n], of the rounded rows
  uint32_t image_stride;     // in half elements
  uint32_t cand_k;           // k * oversampling (<= f.s.nbmax)
};
template <int METRIC, int CPL, bool F16>
__global__ __launch_bounds__(256, 4) void hnsw_search_filters_half_rescore_kernel(HnswFiltersHalfRescoreArgs A) {
  FiltDistHalfRescore<METRIC, CPL, F16> dist;
  dist.image = A.image;
  dist.image_norms = A.image_norms;
  dist.image_stride = A.image_stride;
  dist.cand_k = A.cand_k;
  filtered_walk_body<METRIC, CPL>(A.f, dist);
}

// The exact pass: one block per query over the filter's ascending row list in chunks of nbmax — dead rows skipped, distances by
// the walk's DIST::eval, the k best by (total-order(distance), row) in the same LDS list (a.cap >= k entries), results in the
// walk's format.  Adds the rows it evaluated to the query's n_dist.
template <int METRIC, int CPL, class DIST = FiltDist<METRIC, CPL>>
__device__ __forceinline__ void filter_rank_body(const HnswFiltersArgs& fa) {
  const HnswSearchArgs& a = fa.s;
  unsigned long long* qstats = fa.qstats;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wib = (int)rfl(threadIdx.x >> 6);
  const uint32_t cap = a.cap, nbmax = a.nbmax, k = a.k;
  const auto [keys, nb_id, nb_d, ctl, flags, qscratch] = WalkLds(smem, cap, nbmax);
  DIST dist;
  dist.init(a, qscratch);

  for (uint32_t slot = blockIdx.x; slot < a.nq; slot += gridDim.x) {
    const SlotFilter f = load_slot_filter(fa, slot);
    const uint32_t qi = f.qi;
    dist.load_query(a.queries + (size_t)qi * a.q_stride, lane);
    __syncthreads();
    uint32_t cnt = 0, n_eval = 0, at = 0, m_prev = 0;  // leader state (wave 0; wave-uniform)
    for (;;) {
      if (wib == 0) {
        // the chunk evaluated last: keys below the k-th best (or anything while the list is short) enter in row order
        for (uint32_t base = 0; base < m_prev; base += 64) {
          const uint32_t t = base + lane;
          const uint64_t key = t < m_prev ? make_key<false>(nb_d[t], nb_id[t]) : kKeyInvalid;
          uint64_t mask = __ballot(t < m_prev && (cnt < k || key < keys[k - 1]));
          while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const uint64_t kj = readlane64(key, src);
            if (cnt < k || kj < keys[k - 1]) {
              uint32_t lost, lost_flag;
              flist_insert(keys, flags, cnt, k, kj, 0u, lane, lost, lost_flag);
            }
          }
        }
        n_eval += m_prev;
        // the next chunk: up to nbmax list entries, the live ones compacted in order
        uint32_t m = 0;
        while (m == 0 && at < f.count) {
          const uint32_t lim = min(nbmax, f.count - at);
          for (uint32_t base = 0; base < lim; base += 64) {
            const uint32_t t = base + lane;
            uint32_t row = 0;
            bool ok = false;
            if (t < lim) {
              row = f.list == nullptr ? at + t : f.list[at + t];  // (no filter: the rows themselves)
              ok = row < a.n_rows && (!a.alive || a.alive[row] != 0);
            }
            const uint64_t mask = __ballot(ok);
            if (ok) nb_id[m + (uint32_t)__popcll(mask & lt_mask(lane))] = row;  // (< lim <= nbmax)
            m += (uint32_t)__popcll(mask);
          }
          at += lim;
        }
        if (lane == 0) {
          ctl[0] = m;
          ctl[1] = m == 0 ? 1u : 0u;
        }
        m_prev = m;
      }
      __syncthreads();
      const uint32_t m = ctl[0];
      if (ctl[1]) break;
      dist.eval(m, nb_id, nb_d, lane, wib, false);
      __syncthreads();
    }
    if (wib == 0) {
      for (uint32_t e = lane; e < k; e += 64) {
        uint64_t id = ~0ull;
        float sc = __uint_as_float(0x7FC00000u);
        if (e < cnt) {
          const uint64_t key = keys[e];
          const uint32_t node = (uint32_t)key;
          id = a.ext_ids ? a.ext_ids[node] : (uint64_t)node;
          sc = transform_score_dev(METRIC, key_dist(key));
        }
        a.out_ids[(size_t)qi * k + e] = id;
        a.out_scores[(size_t)qi * k + e] = sc;
      }
      if (lane == 0) {
        a.out_n[qi] = cnt;
        qstats[(size_t)qi * 2] += n_eval;
      }
    }
    __syncthreads();  // (ctl, the list: read by everybody before the next query's leader rewrites them)
  }
}

template <int METRIC, int CPL>
__global__ __launch_bounds__(256, 4) void filters_rank_kernel(HnswFiltersArgs fa) {
  filter_rank_body<METRIC, CPL>(fa);
}
template <int METRIC, int CPL, bool F16>
__global__ __launch_bounds__(256, 4) void filters_rank_half_kernel(HnswFiltersArgs fa) {
  filter_rank_body<METRIC, CPL, FiltDistHalf<METRIC, CPL, F16>>(fa);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// (ROWS: FiltersRows — the f32 rows and packed bits, or one of the half images)
template <bool RANK, int METRIC, int CPL, int ROWS>
static auto kernel_of() {
  if constexpr (ROWS == kFiltersF32)
    return RANK ? filters_rank_kernel<METRIC, CPL> : hnsw_search_filters_kernel<METRIC, CPL>;
  else
    return RANK ? filters_rank_half_kernel<METRIC, CPL, ROWS == kFiltersF16> : hnsw_search_filters_half_kernel<METRIC, CPL, ROWS == kFiltersF16>;
}

// one launch of the walk (RANK = false) or the exact pass over the f32 rows and packed bits, or over a half image (Cosine, Euclidean
// and DotProduct: there is no image of packed bits — refused in front of the call)
template <bool RANK, int ROWS = kFiltersF32>
static hipError_t launch_filtered(const HnswFiltersArgs& fa, int slots, size_t lds, hipStream_t st) {
  return walk_dispatch<ROWS == kFiltersF32 ? BitMetrics::kTaken : BitMetrics::kRefused>(fa.s.metric, fa.s.dim, [&](auto M, auto C) {
    return launch_walk_blocks(kernel_of<RANK, M(), C(), ROWS>(), fa, fa.s.n_cus, slots, lds, st);
  });
}
// ... over the rows the call names
template <bool RANK>
static hipError_t launch_filters_rows(const HnswFiltersArgs& fa, int rows, int slots, size_t lds, hipStream_t st) {
  if (rows == kFiltersF16) return launch_filtered<RANK, kFiltersF16>(fa, slots, lds, st);
  if (rows == kFiltersBF16) return launch_filtered<RANK, kFiltersBF16>(fa, slots, lds, st);
  return launch_filtered<RANK>(fa, slots, lds, st);
}
// ... the walk over the u8 codes (three metrics: refused in front of the call otherwise)
static hipError_t launch_filters_int8(const HnswFiltersInt8Args& A, int slots, size_t lds, hipStream_t st) {
  return walk_dispatch<BitMetrics::kRefused>(A.f.s.metric, A.f.s.dim, [&](auto M, auto C) {
    return launch_walk_blocks(hnsw_search_filters_int8_kernel<M(), C()>, A, A.f.s.n_cus, slots, lds, st);
  });
}
// ... the walk over a half image with the re-score over the f32 rows (three metrics: refused in front of the call otherwise)
template <bool F16>
static hipError_t launch_filters_half_rescore(const HnswFiltersHalfRescoreArgs& A, int slots, size_t lds, hipStream_t st) {
  return walk_dispatch<BitMetrics::kRefused>(A.f.s.metric, A.f.s.dim, [&](auto M, auto C) {
    return launch_walk_blocks(hnsw_search_filters_half_rescore_kernel<M(), C(), F16>, A, A.f.s.n_cus, slots, lds, st);
  });
}

// the largest list (entries) whose launch stays inside 160 KB of LDS at this nbmax: hnsw_search_prepare's limit
// (lds_of: the call's layout — hnsw_lds_bytes, or hnsw_int8_lds_bytes for the walk over the codes)
template <class LdsOf>
static uint32_t largest_list(LdsOf&& lds_of) {
  uint64_t cap = kFgLdsBudget / 9 / 64 * 64;
  while (cap && lds_of((uint32_t)cap) > kFgLdsBudget) cap -= 64;
  return (uint32_t)cap;
}

// What a filtered call does with the rows it names (FiltersRows, vdb_index.hpp): filled once, read by everything below.
enum WalkRows : int { kWalkF32, kWalkF16, kWalkBF16, kWalkCodes };
enum WalkLdsRule : int { kLdsWalk, kLdsInt8, kLdsHalfRescore };  // hnsw_lds_bytes / hnsw_int8_lds_bytes / hnsw_half_rescore_lds_bytes
struct FiltersMode {
  WalkRows walk;                  // the rows the walk's distances are taken over
  bool rescore;                   // behind the walk, the k * ratio best allowed candidates are re-scored over the f32 rows
  bool vdb_hip_index::*enabled;   // what the index must have been given for it (null: nothing) ...
  const char* enable_first;       // ... and the status that says so (those of the plain walks: hnsw_search_half_dev, hnsw_search_int8_dev)
  const char* what;               // the text the metric and ratio statuses start with
  uint32_t walk_kernels;          // VDB_KERNEL_* bits of a round of walk launches ...
  uint32_t exact_kernels;         // ... and of the exact pass
  WalkLdsRule lds;                // the layout of a walk launch
  int exact_rows;                 // the rows of the exact pass (FiltersRows): the walk's own, or f32 behind a re-score — scored in f32 anyway
};
static FiltersMode filters_mode(int rows) {
  constexpr uint32_t W = VDB_KERNEL_HNSW_FILTERED, X = VDB_KERNEL_FILTER_RANK, H = VDB_KERNEL_HNSW_HALF, F = VDB_KERNEL_F16;
  switch (rows) {
    case kFiltersF16:
      return {kWalkF16, false, &vdb_hip_index::f16_enabled, "f16 filtered graph search: call vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) first",
              "half-precision filtered graph search", W | H | F, X | H | F, kLdsWalk, kFiltersF16};
    case kFiltersBF16:
      return {kWalkBF16, false, &vdb_hip_index::bf16_enabled, "bf16 filtered graph search: call vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16) first",
              "half-precision filtered graph search", W | H, X | H, kLdsWalk, kFiltersBF16};
    case kFiltersInt8:
      return {kWalkCodes, true, &vdb_hip_index::quantizer_trained, "int8 filtered graph search: call vdb_hip_index_train_quantizer first",
              "int8 filtered graph search", W | VDB_KERNEL_HNSW_INT8, X, kLdsInt8, kFiltersF32};
    case kFiltersF16Rescore:
      return {kWalkF16, true, &vdb_hip_index::f16_enabled,
              "f16 filtered graph search with re-score: call vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) first",
              "half-precision filtered graph search with re-score", W | H | VDB_KERNEL_HALF_RESCORE | F, X, kLdsHalfRescore, kFiltersF32};
    case kFiltersBF16Rescore:
      return {kWalkBF16, true, &vdb_hip_index::bf16_enabled,
              "bf16 filtered graph search with re-score: call vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16) first",
              "half-precision filtered graph search with re-score", W | H | VDB_KERNEL_HALF_RESCORE, X, kLdsHalfRescore, kFiltersF32};
    default: return {kWalkF32, false, nullptr, nullptr, "filtered graph search", W, X, kLdsWalk, kFiltersF32};
  }
}

// vdb_hip_index_search_graph_filters on a leased context (ix->mu shared, by the caller): one filter per query.  The
// queries go up, every query gets its own plan (filter_graph_route on ITS filter), climbs its own ladder of capacities and takes the
// exact pass behind it if the largest list could not hold it; the result block comes back in ix->h_out (reserve_out's layout).
// Queries only share launches: filters_walk_ladders (vdb_filter_route.hpp) groups every round into at most four launches by LDS
// footprint, and every exact pass of the call is one launch — so query i computes what it computes in a call of its own.
// filters: [n_filters] handles, non-null; fq: [nq] values in 0..n_filters, n_filters = no filter; routes: host, [nq].
int32_t search_graph_filters_to_device(vdb_hip_index* ix, const RowFilter* const* filters, uint32_t n_filters, const uint32_t* fq,
                                       const float* queries, uint32_t nq, uint32_t k, uint32_t ef, int32_t route, uint32_t max_list,
                                       uint32_t* routes, int rows, uint32_t ratio) {
  int32_t rc;
  const FiltersMode m = filters_mode(rows);
  const bool int8 = m.walk == kWalkCodes, f16 = m.walk == kWalkF16;
  // the ratio's status comes last for the walk over the codes and first for a half image with the re-score
  const bool bad_ratio = m.rescore && (ratio == 0 || ratio > 64);
  if (bad_ratio && !int8) return fail(VDB_ERR_INVALID_ARG, std::string(m.what) + ": oversampling ratio 1..64");
  if (m.enabled && !(ix->*m.enabled)) return fail(VDB_ERR_STATE, m.enable_first);
  if (m.walk != kWalkF32 && ix->metric != VDB_COSINE && ix->metric != VDB_DOT && ix->metric != VDB_EUCLIDEAN)
    return fail(VDB_ERR_UNSUPPORTED, std::string(m.what) + ": Cosine, DotProduct and Euclidean only");
  if (bad_ratio) return fail(VDB_ERR_INVALID_ARG, std::string(m.what) + ": oversampling ratio 1..64");
  for (uint32_t j = 0; j < n_filters; j++)
    if ((rc = filter_check(ix, filters[j])) != VDB_OK) return rc;
  if (!ix->graph_valid) return fail(VDB_ERR_STATE, "HNSW graph not built for all rows (use the exact filtered search or build it)");
  hipStream_t st = ix->stream;
  ix->ev_used = 0;
  ix->sel_ev_used = 0;
  ix->last_select_level = 0;
  ix->split_flags_n = 0;
  ix->last_kernels = 0;
  ix->last_n_dist = ix->last_n_expand = ix->last_pf_hits = 0;
  ix->stats_pending = false;
  const size_t kk = std::max<uint32_t>(k, 1);
  rc = reserve_out(ix, nq, kk, st);
  if (rc != VDB_OK) return rc;
  if (ix->h_out.reserve(ix->s_out_bytes) != hipSuccess) return fail(VDB_ERR_OOM, "pinned result staging");
  uint32_t* d_n = ix->s_out_n.as<uint32_t>();
  unsigned char* h_base = ix->h_out.as<unsigned char>();
  uint32_t* h_n = reinterpret_cast<uint32_t*>(h_base + (size_t)((unsigned char*)ix->s_out_n.p - (unsigned char*)ix->s_out.p));
  std::memset(routes, 0, (size_t)nq * 4);
  // a query nothing runs for (an empty filter; k = 0; an empty graph): out_n = 0 and padding, written on the host at the end
  auto blank = [&]() {
    uint64_t* h_ids = reinterpret_cast<uint64_t*>(h_base);
    uint32_t* h_sc = reinterpret_cast<uint32_t*>(h_base + (size_t)nq * kk * 8);
    for (uint32_t i = 0; i < nq; i++) {
      if (routes[i] != 0) continue;
      h_n[i] = 0;
      for (size_t e = 0; e < (size_t)k; e++) {
        h_ids[(size_t)i * k + e] = ~0ull;
        h_sc[(size_t)i * k + e] = 0x7FC00000u;
      }
    }
  };
  // graph.rs:252-255: no entry point => empty; k = 0 or filters that are all empty cannot answer either — no launch
  bool matched_any = false;
  for (uint32_t i = 0; i < nq; i++) matched_any |= fq[i] == n_filters ? ix->n_rows != 0 : filters[fq[i]]->count != 0;
  if (!matched_any || k == 0 || ix->n_rows == 0 || ix->entry_point < 0 || ix->graph_nodes == 0) {
    blank();
    return VDB_OK;
  }
  if (ix->layers.size() > (size_t)kMaxLayers) return fail(VDB_ERR_UNSUPPORTED, "more than 16 graph layers");
  if (ef == 0) ef = std::max<uint32_t>(128, k * 4);  // Balanced, params.rs:313
  ef = std::max(ef, k);                               // SearchQuality::Custom(ef) = max(ef, k), params.rs:317
  // the walk over the codes or a half image with the re-score: cand_k = k * ratio coarse candidates, ef widened over them
  // (dual_precision.rs:334) — the plans take it
  const uint64_t cand_k = m.rescore ? (uint64_t)k * ratio : 0;
  if (m.rescore) ef = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ef, cand_k), 0xFFFFFFFFull);

  HnswFiltersInt8Args fa8{};
  HnswFiltersArgs& fa = fa8.f;
  HnswSearchArgs& a = fa.s;
  // (the re-score gathers its cand_k candidates into the nb arrays: rounded over both, as hnsw_search_int8_dev)
  const uint32_t longest = walk_args_graph(ix, a);
  const uint32_t nbmax = (uint32_t)std::min<uint64_t>((std::max<uint64_t>(longest, cand_k) + 63) / 64 * 64, 0xFFFFFFC0ull);
  const uint32_t nbmax_exact = (longest + 63) / 64 * 64;  // (the exact pass has no candidates to gather: the f32 call's chunks)
  // the walk's layout and the exact pass's (always the f32 one)
  auto lds_of = [&](uint32_t cap) -> uint64_t {
    if (m.lds == kLdsInt8) return hnsw_int8_lds_bytes(cap, nbmax, ix->dim, ix->code_words);
    if (m.lds == kLdsHalfRescore) return hnsw_half_rescore_lds_bytes(cap, nbmax, ix->dim);
    return hnsw_lds_bytes(cap, nbmax, ix->dim, ix->words, ix->metric);
  };
  auto lds_of_exact = [&](uint32_t cap) -> uint64_t { return hnsw_lds_bytes(cap, nbmax_exact, ix->dim, ix->words, ix->metric); };
  uint32_t cap_max = largest_list(lds_of);
  if (max_list) cap_max = std::min(cap_max, max_list);
  const std::string limits = " (route " + std::to_string(route) + ", max_list " + std::to_string(max_list) + ", ef " + std::to_string(ef) + ")";

  // the descriptor table (the last entry: no filter) and every query's own plan
  std::vector<FilterDesc> descs(n_filters + 1);
  for (uint32_t j = 0; j < n_filters; j++)
    descs[j] = FilterDesc{filters[j]->bitmap.as<uint32_t>(), filters[j]->list.as<uint32_t>(), (uint32_t)filters[j]->n_rows, (uint32_t)filters[j]->count};
  descs[n_filters] = FilterDesc{nullptr, nullptr, (uint32_t)ix->n_rows, (uint32_t)ix->n_rows};
  std::vector<FilterGraphPlan> plans(descs.size());  // (a plan depends on the filter alone: one per table entry, not one per query)
  for (size_t j = 0; j < descs.size(); j++) plans[j] = filter_graph_route(route, ef, descs[j].count, ix->n_rows, cap_max);
  std::vector<FiltersSlot> first, exact;
  first.reserve(nq);
  for (uint32_t i = 0; i < nq; i++) {
    if (descs[fq[i]].count == 0) continue;  // (route 0: nothing runs for this query)
    const FilterGraphPlan plan = plans[fq[i]];
    if (plan.route == kFgRefuse)
      return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: the smallest candidate list does not fit the largest list allowed" + limits);
    if (plan.route == kFgWalk) {
      first.push_back(FiltersSlot{i, fq[i], plan.cap, 0});
      routes[i] = kFgWalk;
    } else {
      exact.push_back(FiltersSlot{i, fq[i], 0, 0});
    }
  }

  // The queries go up through pinned staging, and the descriptor table and the slot table of the coming launches travel behind them:
  // same staging buffer, same device buffer, so the first upload of the call is ONE copy (what a call costs before its first launch
  // shows in the one-query case) and no later one starts from pageable memory.  Whole staging rows, so the tables stay aligned.
  const size_t row_bytes = (size_t)ix->row_stride * 4, q_bytes = (size_t)nq * row_bytes, qs_bytes = (size_t)nq * 16;
  const size_t desc_bytes = descs.size() * sizeof(FilterDesc), slot_bytes = (size_t)nq * sizeof(FiltersSlot);
  const uint32_t table_rows = (uint32_t)((desc_bytes + slot_bytes + row_bytes - 1) / row_bytes);
  rc = stage_queries(ix, queries, 0, nq, nq + table_rows);
  if (rc != VDB_OK) return rc;
  if (ix->s_queries.reserve(q_bytes + table_rows * row_bytes, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "search scratch");
  if (ix->s_fgraph.reserve(qs_bytes, false, st) != hipSuccess) return fail(VDB_ERR_OOM, "filtered graph scratch");
  VDB_HIP(hipMemsetAsync(ix->s_fgraph.p, 0, qs_bytes, st));
  unsigned char* h_up = ix->h_in.as<unsigned char>();
  unsigned char* d_up = ix->s_queries.as<unsigned char>();
  std::memcpy(h_up + q_bytes, descs.data(), desc_bytes);
  FiltersSlot* d_slots = reinterpret_cast<FiltersSlot*>(d_up + q_bytes + desc_bytes);
  size_t sent = 0;  // bytes of [queries | descriptors | slots] the device holds
  // the slot table of the next launches (the staging copy of the last ones is free: their round was fetched)
  auto slots_up = [&](const FiltersSlot* slots, size_t n) -> int32_t {
    std::memcpy(h_up + q_bytes + desc_bytes, slots, n * sizeof(FiltersSlot));
    const size_t from = sent ? q_bytes + desc_bytes : 0, to = q_bytes + desc_bytes + n * sizeof(FiltersSlot);
    VDB_HIP(hipMemcpyAsync(d_up + from, h_up + from, to - from, hipMemcpyHostToDevice, st));
    sent = to;
    return VDB_OK;
  };
  walk_args_index(ix, a);
  a.queries = ix->s_queries.as<float>();
  a.q_stride = ix->row_stride;
  a.out_ids = ix->s_out_ids.as<uint64_t>();
  a.out_scores = ix->s_out_scores.as<float>();
  a.out_n = d_n;
  a.k = k;
  a.ef = ef;
  a.nbmax = nbmax;
  if (m.walk != kWalkF32) a.bits = nullptr;
  if (int8) {  // the codes beside the f32 rows, which the re-score and the exact pass read
    fa8.codes = CodeCtx{ix->codes.as<uint32_t>(), ix->codes_sq.as<uint32_t>(), ix->code_words};
    fa8.min_vals = ix->sq_min.as<float>();
    fa8.scales = ix->sq_scale.as<float>();
    fa8.cand_k = (uint32_t)cand_k;  // (<= nbmax <= 2^32 - 64, or the lists did not fit and no walk is planned)
  }
  HnswFiltersHalfRescoreArgs hr{};  // (its .f is copied from fa at every launch)
  if (m.walk == kWalkF16 || m.walk == kWalkBF16) {
    const float* image = reinterpret_cast<const float*>(f16 ? ix->rows_f16.as<uint16_t>() : ix->rows_bf16.as<uint16_t>());
    const float* image_norms = f16 ? ix->norms_f16.as<float>() : ix->norms_bf16.as<float>();
    if (m.rescore) {  // the image beside the f32 rows, which the re-score and the exact pass read
      hr.image = image;
      hr.image_norms = image_norms;
      hr.image_stride = (uint32_t)ix->bf16_stride;
      hr.cand_k = (uint32_t)cand_k;  // (<= nbmax, as above)
    } else {  // the image instead of the f32 rows, as hnsw_search_half_dev: same fields, the stride in half elements
      a.rows = image;
      a.norms = image_norms;
      a.row_stride = ix->bf16_stride;
    }
  }
  // one walk launch of the call's mode
  auto launch_walk = [&](int slots_l, size_t lds) -> hipError_t {
    if (int8) return launch_filters_int8(fa8, slots_l, lds, st);
    if (!m.rescore) return launch_filters_rows<false>(fa, rows, slots_l, lds, st);
    hr.f = fa;
    return f16 ? launch_filters_half_rescore<true>(hr, slots_l, lds, st) : launch_filters_half_rescore<false>(hr, slots_l, lds, st);
  };
  fa.descs = reinterpret_cast<const FilterDesc*>(d_up + q_bytes);
  fa.qstats = ix->s_fgraph.as<unsigned long long>();

  auto fetch = [&]() -> int32_t {
    VDB_HIP(hipMemcpyAsync(ix->h_out.p, ix->s_out.p, ix->s_out_bytes, hipMemcpyDeviceToHost, st));
    VDB_HIP(hipStreamSynchronize(st));
    return VDB_OK;
  };
  // one round of walks: its slot table up, its launches behind each other, one fetch
  auto run_round = [&](const FiltersSlot* slots, uint32_t n, const FiltersLaunch* launches, uint32_t n_launches, unsigned char* over) -> int {
    int32_t r = slots_up(slots, n);
    if (r != VDB_OK) return r;
    int most = 0;
    for (uint32_t l = 0; l < n_launches; l++)
      most = std::max(most, (int)std::min<int64_t>((int64_t)launches[l].count, (int64_t)ix->n_cus * (int64_t)launches[l].per_cu));
    r = ensure_traversal_scratch(ix, st, most);  // (once, in front of the round: the launches share the bitmaps in stream order)
    if (r != VDB_OK) return r;
    a.visited = ix->s_visited.as<uint32_t>();
    a.vlog = ix->s_vlog.as<uint32_t>();
    a.vis_words = ix->vis_words;
    for (uint32_t l = 0; l < n_launches; l++) {
      const FiltersLaunch& L = launches[l];
      a.cap = L.cap;
      a.nq = L.count;
      fa.slots = d_slots + L.begin;
      const size_t lds = lds_of(a.cap);
      if (lds > kFgLdsBudget) return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: candidate list beyond the LDS" + limits);
      const int slots_l = (int)std::min<int64_t>((int64_t)L.count, (int64_t)ix->n_cus * (int64_t)L.per_cu);
      const hipError_t e = launch_walk(slots_l, lds);
      if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("filtered hnsw_search launch: ") + hipGetErrorString(e));
    }
    ix->last_kernels |= m.walk_kernels;
    r = fetch();
    if (r != VDB_OK) return r;
    for (uint32_t i = 0; i < n; i++) over[i] = h_n[slots[i].query] == 0xFFFFFFFFu;
    return VDB_OK;
  };
  std::vector<FiltersSlot> left;
  rc = filters_walk_ladders(first, cap_max, lds_of, run_round, &left);
  if (rc != VDB_OK) return rc;
  if (!left.empty() && route == kFgWalk)
    return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: " + std::to_string(left.size()) + " queries overflow the largest candidate list (" +
                                         std::to_string(cap_max) + " entries)" + limits);
  if (!left.empty()) {  // (`exact` is in query order so far)
    exact.insert(exact.end(), left.begin(), left.end());
    std::sort(exact.begin(), exact.end(), [](const FiltersSlot& x, const FiltersSlot& y) { return x.query < y.query; });
  }
  if (!exact.empty()) {  // every exact pass of the call in one launch: the whole-route ones and what the largest list could not hold
    a.cap = (uint32_t)fg_round64(k);
    a.nbmax = nbmax_exact;
    for (FiltersSlot& s : exact) s.cap = a.cap;
    const size_t lds = lds_of_exact(a.cap);
    if (lds > kFgLdsBudget) return fail(VDB_ERR_UNSUPPORTED, "filtered graph search: k too large for the LDS-resident result list");
    rc = slots_up(exact.data(), exact.size());
    if (rc != VDB_OK) return rc;
    a.nq = (uint32_t)exact.size();
    fa.slots = d_slots;
    const int slots_l = (int)std::min<int64_t>((int64_t)a.nq, (int64_t)ix->n_cus * 4);
    const hipError_t e = launch_filters_rows<true>(fa, m.exact_rows, slots_l, lds, st);
    if (e != hipSuccess) return fail(VDB_ERR_HIP, std::string("filters_rank launch: ") + hipGetErrorString(e));
    ix->last_kernels |= m.exact_kernels;
    rc = fetch();
    if (rc != VDB_OK) return rc;
    for (const FiltersSlot& s : exact) routes[s.query] = kFgExact;
  }
  blank();
  // the call's counters: every query's last walk attempt plus the rows its exact pass evaluated
  std::vector<unsigned long long> qs((size_t)nq * 2);
  VDB_HIP(hipMemcpyAsync(qs.data(), ix->s_fgraph.p, qs_bytes, hipMemcpyDeviceToHost, st));
  VDB_HIP(hipStreamSynchronize(st));
  for (uint32_t i = 0; i < nq; i++) {
    ix->last_n_dist += qs[(size_t)i * 2];
    ix->last_n_expand += qs[(size_t)i * 2 + 1];
  }
  return VDB_OK;
}

// vdb_hip_index_search_graph_filtered: one filter for the whole call = a table of that filter with every query on it.
// routes: host, [nq], nullable (multi_query_direct, search_front.hip, has no use for them).
int32_t search_graph_filtered_to_device(vdb_hip_index* ix, const RowFilter* f, const float* queries, uint32_t nq, uint32_t k, uint32_t ef,
                                        int32_t route, uint32_t max_list, uint32_t* routes) {
  const std::vector<uint32_t> fq(nq, 0u);
  std::vector<uint32_t> r(nq, 0u);
  const int32_t rc = search_graph_filters_to_device(ix, &f, 1, fq.data(), queries, nq, k, ef, route, max_list, r.data(), kFiltersF32);
  if (rc == VDB_OK && routes) std::copy(r.begin(), r.end(), routes);
  return rc;
}

}  // namespace vdb
