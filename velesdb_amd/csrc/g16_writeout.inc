// g16_writeout.inc — textually included by the kernels of sweep_gemm_bf16.hip behind the last row tile: final compaction and
// the block's partial list per query; WIDE: the flush of the block's stash into the queries' global lists.
// Needs: a, wib, nq_t, k, q0, g, cnts, cand, tauk, qn, compact(), WAVES, CAP.
  if constexpr (WIDE) {
  // one device-scope atomicAdd per query that has stash entries (its count, at most CAP: what went past the stash was counted where it
  // went), then the keys, a query's run of CAP slots on consecutive lanes.  Entries past the list's capacity are dropped; the count
  // above it tells sweep_wide.hip the query is unproven
  __syncthreads();  // every wave's stash entries are in
  uint32_t* wbase = reinterpret_cast<uint32_t*>(qn);  // (the query norms are not read again) position of the block's run per query
  const uint32_t t_o = (uint32_t)wib * 64u + lane_now();
  if (t_o < nq_t) {
    const uint32_t n = min(cnts[t_o], (uint32_t)CAP);
    wbase[t_o] = n ? atomicAdd(&a.wide_cnt[q0 + t_o], n) : 0u;
  }
  __syncthreads();
  for (uint32_t i = t_o; i < nq_t * (uint32_t)CAP; i += (uint32_t)WAVES * 64u) {
    const uint32_t b = i / (uint32_t)CAP, e = i - b * (uint32_t)CAP;
    const uint32_t pos = wbase[b] + e;
    if (e < cnts[b] && pos < a.wide_cap) a.wide_keys[(size_t)(q0 + b) * a.wide_cap + pos] = cand[i];
  }
  }
  if constexpr (!WIDE) {
  __syncthreads();
  compact();  // every buffer still holding more than k keys
  __syncthreads();
  const uint32_t lane_o = lane_now();
  for (uint32_t b = wib; b < nq_t; b += WAVES) {
    const uint32_t c = min(cnts[b], k);  // <= k entries, whatever order (the merge kernel scans them all)
    uint64_t* out = a.part_keys + ((size_t)(q0 + b) * a.list_stride + a.list_off + g) * k;
    for (uint32_t e = lane_o; e < k; e += 64) out[e] = e < c ? cand[(size_t)b * CAP + e] : kKeyInvalid;
    if (a.blk_tau && lane_o == 0) a.blk_tau[(size_t)(q0 + b) * a.list_stride + a.list_off + g] = tauk[b];
  }
  }
