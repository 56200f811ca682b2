// sq8_sweep_body.inc — the body of sweep_topk_sq8<METRIC, B>, sweep_topk_sq8_listed<METRIC, B> and sweep_topk_sq8_listed_groups<METRIC, B>
// (storage_modes.hip, which explains why it is shared as text).  In scope where it is included: METRIC, B, `constexpr bool LISTED`,
// `constexpr bool GROUPED`, `a` (Sq8Args), and — read only when LISTED — `list`, `count`, `per_block`, and — read only when GROUPED
// (which implies LISTED: `list` / `count` are the item's chunk, swept whole from unit 0; DESIGN 4.1q) — `it` (the block's
// ListedGroupItem), `nq_item` and `lists_per_q`.  (The item's `units` is not read: a unit is a 64-row group here, so it is
// ceil(count / 64), computed below anyway.)
  constexpr bool HIB = METRIC != kEuclidean;  // cosine / dot similarity: larger is better; squared L2: smaller
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t k = a.k, dim = a.dim;
  const uint32_t dpad = (dim + 3u) & ~3u;
  // LDS: queries [dpad][B] f32 | per-wave tiles [4][64][80] | lists [B][k] | cnt[B] | lock[B] | qsum[B] | qnsq[B]
  float* qs = reinterpret_cast<float*>(smem);
  unsigned char* tiles = smem + (size_t)dpad * B * 4;
  unsigned char* tile = tiles + (size_t)wib * 64 * kSq8TileStride;
  unsigned char* tail = tiles + (size_t)4 * 64 * kSq8TileStride;
  lds_vu64* lists = (lds_vu64*)(lds_void_p)(tail);
  lds_vu32* cnts = (lds_vu32*)(lds_void_p)(tail + (size_t)B * k * 8);
  uint32_t* locks = reinterpret_cast<uint32_t*>(tail + (size_t)B * k * 8 + B * 4);
  float* qsum = reinterpret_cast<float*>(tail + (size_t)B * k * 8 + B * 8);
  float* qnsq = reinterpret_cast<float*>(tail + (size_t)B * k * 8 + B * 12);

  uint32_t nq_here = GROUPED ? nq_item : a.nq, slot0 = 0;
  if (!LISTED && a.qmap) {
    const uint32_t listed = *a.qcount;
    slot0 = blockIdx.y * (uint32_t)B;
    if (slot0 >= listed) return;  // (uniform per block)
    nq_here = min((uint32_t)B, listed - slot0);
  }
  for (uint32_t i = tid; i < dpad * B; i += 256) {
    const uint32_t d = i / B, b = i % B;
    uint32_t qrow = (!LISTED && a.qmap && b < nq_here) ? a.qmap[slot0 + b] : b;
    if constexpr (GROUPED) qrow = b < nq_here ? it->q[b] : 0u;  // (the pass's queries: positions in the call)
    qs[i] = (d < dim && b < nq_here) ? a.queries[(size_t)qrow * a.q_stride + d] : 0.0f;
  }
  if (tid < B) {
    cnts[tid] = 0;
    locks[tid] = 0;
  }
  __syncthreads();
  if (tid < B) {  // per query: sum(q) (constant-vector branch, :332-334) and sum(q*q) (:528), left to right
    float s = 0.0f, n2 = 0.0f;
    for (uint32_t d = 0; d < dim; d++) {
      const float x = qs[d * B + tid];
      s = __fadd_rn(s, x);
      n2 = __fadd_rn(n2, __fmul_rn(x, x));
    }
    qsum[tid] = s;
    qnsq[tid] = n2;
  }
  __syncthreads();

  const uint32_t n_here = LISTED ? count : a.n_rows;  // rows of the sweep: positions of the list, or rows of the index
  const uint32_t ngroups = (n_here + 63) / 64;
  const uint32_t g_end = GROUPED ? ngroups : (LISTED ? min(ngroups, (blockIdx.x + 1) * per_block) : ngroups);  // listed: the block's chunk of the list
  for (uint32_t g = GROUPED ? (uint32_t)wib : (LISTED ? blockIdx.x * per_block + (uint32_t)wib : blockIdx.x * 4 + wib); g < g_end;
       g += LISTED ? 4u : gridDim.x * 4) {
    const uint32_t pos = g * 64 + lane;
    const bool valid = pos < n_here;
    const uint32_t posc = valid ? pos : n_here - 1;
    const uint32_t row = LISTED ? list[posc] : pos;   // (listed: the tail re-reads the list's last row, masked below)
    const uint32_t rowc = LISTED ? row : posc;
    uint32_t srow[4];  // listed: the rows whose pieces this lane stages (position 16 j + lane / 4 of the group)
    if constexpr (LISTED) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t sp = g * 64 + 16 * j + (lane >> 2);
        srow[j] = list[sp < n_here ? sp : n_here - 1];
      }
    }
    const float mn = a.vmin[rowc];
    const float range = __fsub_rn(a.vmax[rowc], mn);
    const bool flat = range < kF32Eps;
    const float scale = __fdiv_rn(range, 255.0f);
    float acc[B];
#pragma unroll
    for (int b = 0; b < B; b++) acc[b] = 0.0f;
    // query elements: LDS, dimension-major [dim][B] — one broadcast ds_read_b128 brings element i of all 4 queries as two
    // adjacent pairs, the operands of the packed multiplies below
    // staging loads run one 64-byte column chunk ahead of the arithmetic (registers), so their latency hides
    // behind the previous chunk's ~700 VALU instructions
    // (the loads are RAW — clamped address, always in bounds — and the rows / columns past the end are zeroed where the staged value
    // is USED, one chunk later: with the select beside the load, as rounds 1-4 had it, the compiler waited for the four loads
    // (vmcnt) right where it had issued them, and every chunk paid the codes' trip from HBM in full — half of every wave's time,
    // profiles/r05k_*: SQ_WAIT_ANY 0.51)
    uint4 stg[4];
    auto stage_load = [&](uint32_t c0) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t rr = g * 64 + 16 * j + (lane >> 2);
        const uint32_t off = c0 + (lane & 3) * 16;
        uint32_t rc = rr < n_here ? rr : n_here - 1;
        if constexpr (LISTED) rc = srow[j];
        const uint32_t oc = off < a.code_stride ? off : 0u;
        stg[j] = *reinterpret_cast<const uint4*>(a.codes + (size_t)rc * a.code_stride + oc);
      }
    };
    stage_load(0);
    for (uint32_t c0 = 0; c0 < dim; c0 += 64) {
      // stage 64 rows x 64 B: lane l moves 16 B of row 16 j + l/4, part l%4
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool ok = g * 64 + 16 * j + (lane >> 2) < n_here && c0 + (lane & 3) * 16 < a.code_stride;
        *reinterpret_cast<uint4*>(tile + (16 * j + (lane >> 2)) * kSq8TileStride + (lane & 3) * 16) =
            make_uint4(ok ? stg[j].x : 0u, ok ? stg[j].y : 0u, ok ? stg[j].z : 0u, ok ? stg[j].w : 0u);
      }
      if (c0 + 64 < dim) stage_load(c0 + 64);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      uint4 w4[4];
#pragma unroll
      for (int j = 0; j < 4; j++) w4[j] = *reinterpret_cast<const uint4*>(tile + lane * kSq8TileStride + j * 16);
      __builtin_amdgcn_wave_barrier();  // tile reads done before the next chunk overwrites it
      const uint32_t wds[16] = {w4[0].x, w4[0].y, w4[0].z, w4[0].w, w4[1].x, w4[1].y, w4[1].z, w4[1].w,
                                w4[2].x, w4[2].y, w4[2].z, w4[2].w, w4[3].x, w4[3].y, w4[3].z, w4[3].w};
      if ((B == 4 || B == 8) && c0 + 64 <= dim) {  // full chunk, 4 or 8 queries: grouped query reads, one word ahead
        if constexpr (B == 4 || B == 8) {
          const uint32_t qaddr = (uint32_t)(size_t)(lds_void_p)smem + c0 * (uint32_t)B * 4u;  // (qs starts the dynamic LDS; uniform)
          sq8_f32x4 qa[4][B / 4], qb[4][B / 4];
          sq8_read_word<B, 0>(qa, qaddr);
          sq8_lds_wait(qa);
          sq8_word_pair<METRIC, B, 0>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 2>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 4>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 6>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 8>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 10>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 12>(acc, wds, scale, mn, qaddr, qa, qb);
          sq8_word_pair<METRIC, B, 14>(acc, wds, scale, mn, qaddr, qa, qb);
        }
      } else if (c0 + 64 <= dim) {  // full chunk: no bounds tests => ONE basic block, the scheduler overlaps the LDS reads of
                             // later groups with the arithmetic of earlier ones (per-group branches pinned them)
  #pragma unroll
        for (int wi = 0; wi < 16; wi++) {
          const uint32_t i0 = c0 + wi * 4;
          const uint32_t w = wds[wi];
          float dq[4];
  #pragma unroll
          for (int e = 0; e < 4; e++) dq[e] = __fadd_rn(__fmul_rn((float)((w >> (8 * e)) & 0xFFu), scale), mn);
          // Two queries per instruction where B is even (v_pk_mul_f32 / v_pk_add_f32: each half is the same IEEE
          // operation as the scalar form, so the bits do not change; a plain f32 VALU op runs at half the packed rate).
          constexpr int P = B / 2;  // query pairs
          if (METRIC == kEuclidean) {
            if (true) {  // a full group of four: sum += ((f0^2 + f1^2) + f2^2) + f3^2 (:495-507)
  #pragma unroll
              for (int p = 0; p < P; p++) {
                f32x2 t = {0.f, 0.f};
  #pragma unroll
                for (int e = 0; e < 4; e++) {
                  const f32x2 f = f32x2{qs[(size_t)(i0 + e) * B + (2 * p)], qs[(size_t)(i0 + e) * B + (2 * p + 1)]} - f32x2{dq[e], dq[e]};
                  t = e == 0 ? f * f : t + f * f;
                }
                acc[2 * p] = __fadd_rn(acc[2 * p], t.x);
                acc[2 * p + 1] = __fadd_rn(acc[2 * p + 1], t.y);
              }
              if (B & 1) {
                const int b = B - 1;
                const float f0 = __fsub_rn(qs[(size_t)(i0 + 0) * B + (b)], dq[0]), f1 = __fsub_rn(qs[(size_t)(i0 + 1) * B + (b)], dq[1]);
                const float f2 = __fsub_rn(qs[(size_t)(i0 + 2) * B + (b)], dq[2]), f3 = __fsub_rn(qs[(size_t)(i0 + 3) * B + (b)], dq[3]);
                const float t = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(f0, f0), __fmul_rn(f1, f1)), __fmul_rn(f2, f2)),
                                          __fmul_rn(f3, f3));
                acc[b] = __fadd_rn(acc[b], t);
              }
            } else {  // remainder: one element at a time (:510-515)
  #pragma unroll
              for (int e = 0; e < 4; e++) {
                if (true) {
  #pragma unroll
                  for (int b = 0; b < B; b++) {
                    const float f = __fsub_rn(qs[(size_t)(i0 + e) * B + (b)], dq[e]);
                    acc[b] = __fadd_rn(acc[b], __fmul_rn(f, f));
                  }
                }
              }
            }
          } else {  // dot chain (:452-466), also the numerator of the cosine
  #pragma unroll
            for (int e = 0; e < 4; e++) {
              if (true) {
  #pragma unroll
                for (int p = 0; p < P; p++) {
                  const f32x2 r = f32x2{acc[2 * p], acc[2 * p + 1]} +
                                  f32x2{qs[(size_t)(i0 + e) * B + (2 * p)], qs[(size_t)(i0 + e) * B + (2 * p + 1)]} * f32x2{dq[e], dq[e]};
                  acc[2 * p] = r.x;
                  acc[2 * p + 1] = r.y;
                }
                if (B & 1) acc[B - 1] = __fadd_rn(acc[B - 1], __fmul_rn(qs[(size_t)(i0 + e) * B + (B - 1)], dq[e]));
              }
            }
          }
        }
      } else {
  #pragma unroll
        for (int wi = 0; wi < 16; wi++) {
          const uint32_t i0 = c0 + wi * 4;
          if (i0 >= dim) break;  // uniform
          const uint32_t w = wds[wi];
          float dq[4];
  #pragma unroll
          for (int e = 0; e < 4; e++) dq[e] = __fadd_rn(__fmul_rn((float)((w >> (8 * e)) & 0xFFu), scale), mn);
          // Two queries per instruction where B is even (v_pk_mul_f32 / v_pk_add_f32: each half is the same IEEE
          // operation as the scalar form, so the bits do not change; a plain f32 VALU op runs at half the packed rate).
          constexpr int P = B / 2;  // query pairs
          if (METRIC == kEuclidean) {
            if (i0 + 3 < dim) {  // a full group of four: sum += ((f0^2 + f1^2) + f2^2) + f3^2 (:495-507)
  #pragma unroll
              for (int p = 0; p < P; p++) {
                f32x2 t = {0.f, 0.f};
  #pragma unroll
                for (int e = 0; e < 4; e++) {
                  const f32x2 f = f32x2{qs[(size_t)(i0 + e) * B + (2 * p)], qs[(size_t)(i0 + e) * B + (2 * p + 1)]} - f32x2{dq[e], dq[e]};
                  t = e == 0 ? f * f : t + f * f;
                }
                acc[2 * p] = __fadd_rn(acc[2 * p], t.x);
                acc[2 * p + 1] = __fadd_rn(acc[2 * p + 1], t.y);
              }
              if (B & 1) {
                const int b = B - 1;
                const float f0 = __fsub_rn(qs[(size_t)(i0 + 0) * B + (b)], dq[0]), f1 = __fsub_rn(qs[(size_t)(i0 + 1) * B + (b)], dq[1]);
                const float f2 = __fsub_rn(qs[(size_t)(i0 + 2) * B + (b)], dq[2]), f3 = __fsub_rn(qs[(size_t)(i0 + 3) * B + (b)], dq[3]);
                const float t = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(f0, f0), __fmul_rn(f1, f1)), __fmul_rn(f2, f2)),
                                          __fmul_rn(f3, f3));
                acc[b] = __fadd_rn(acc[b], t);
              }
            } else {  // remainder: one element at a time (:510-515)
  #pragma unroll
              for (int e = 0; e < 4; e++) {
                if (i0 + e < dim) {
  #pragma unroll
                  for (int b = 0; b < B; b++) {
                    const float f = __fsub_rn(qs[(size_t)(i0 + e) * B + (b)], dq[e]);
                    acc[b] = __fadd_rn(acc[b], __fmul_rn(f, f));
                  }
                }
              }
            }
          } else {  // dot chain (:452-466), also the numerator of the cosine
  #pragma unroll
            for (int e = 0; e < 4; e++) {
              if (i0 + e < dim) {
  #pragma unroll
                for (int p = 0; p < P; p++) {
                  const f32x2 r = f32x2{acc[2 * p], acc[2 * p + 1]} +
                                  f32x2{qs[(size_t)(i0 + e) * B + (2 * p)], qs[(size_t)(i0 + e) * B + (2 * p + 1)]} * f32x2{dq[e], dq[e]};
                  acc[2 * p] = r.x;
                  acc[2 * p + 1] = r.y;
                }
                if (B & 1) acc[B - 1] = __fadd_rn(acc[B - 1], __fmul_rn(qs[(size_t)(i0 + e) * B + (B - 1)], dq[e]));
              }
            }
          }
        }
      }
    }
    // constant-vector rows (range < EPSILON) take the reference's other branch; rare, so a divergent redo
    if (__ballot(valid && flat)) {
      if (valid && flat) {
#pragma unroll
        for (int b = 0; b < B; b++) {
          if (METRIC == kEuclidean) {  // sum((q - value)^2), left to right (:357-361)
            float s = 0.0f;
            for (uint32_t d = 0; d < dim; d++) {
              const float f = __fsub_rn(qs[d * B + b], mn);
              s = __fadd_rn(s, __fmul_rn(f, f));
            }
            acc[b] = s;
          } else {
            acc[b] = __fmul_rn(qsum[b], mn);  // sum(q) * value (:330-334)
          }
        }
      }
    }
    const float vn2 = (METRIC == kCosine) ? a.nsq[rowc] : 0.0f;
    uint64_t taus[B];  // the lists' bounds, read together (vdb_device.hpp list_tau_relaxed)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < B; b++) taus[b] = list_tau_relaxed(lists, cnts, (uint32_t)b, k);
#pragma unroll
    for (int b = 0; b < B; b++) {
      float score = acc[b];
      if (METRIC == kCosine) {  // :548-553
        const float denom = sqrtf(__fmul_rn(qnsq[b], vn2));
        score = denom < kF32Eps ? 0.0f : __fdiv_rn(acc[b], denom);
      }
      const bool ok = valid && (uint32_t)b < nq_here;
      const uint64_t key = ok ? make_key<HIB>(score, row) : kKeyInvalid;
      uint64_t mask = __ballot(key < taus[b]);
      while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t kk = readlane64(key, src);
        if (a.alive && a.alive[key_row(kk)] == 0) continue;
        shared_list_offer(lists + (size_t)b * k, cnts + b, locks + b, k, kk, lane);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = wib; b < nq_here && b < (uint32_t)B; b += 4) {
    const uint32_t c = cnts[b];
    uint64_t* out = a.part_keys + ((size_t)(slot0 + b) * gridDim.x + blockIdx.x) * k;
    // (grouped: list it->slot of the lists_per_q the query at position it->q[b] owns; both read here, not kept across the sweep)
    if constexpr (GROUPED) out = a.part_keys + ((size_t)it->q[b] * lists_per_q + (uint32_t)__builtin_amdgcn_readfirstlane((int)it->slot)) * k;
    for (uint32_t e = lane; e < k; e += 64) out[e] = e < c ? lists[(size_t)b * k + e] : kKeyInvalid;
  }
