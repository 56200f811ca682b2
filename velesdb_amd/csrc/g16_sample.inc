// g16_sample.inc — the SAMPLE instance's epilogue (sweep_gemm_bf16.hip gemm16_pp_body), textually included at the end of a row tile in
// place of g16_quicktest*.inc + g16_protocol.inc, once every wave of the block has passed the same number of barriers and the wave's
// accumulators acc[8][4] hold its 128 rows x 64 queries of dot products (DotProduct-form selections only: the product IS the score).
// A lane reduces its 32 accumulators per query column to their maximum — the quick test's v_max3 chain, nothing compared with it —
// and the maximum becomes one sample key of the kind seed_scores_bf16 writes ("the best of a group of rows"): keys[q * ngrp + group],
// the layout wide_seed_kernel / wide_seed_l2_kernel read.  A lane's rows are 16 rf + 4 (lane >> 4) + r of the wave's 128 (rf < 8,
// r < 4); sample_grp == 64 joins the lanes (lane >> 4) = 2 j, 2 j + 1 (one v_permlane16_swap) into groups of 64 rows.
// Validity: a key reflects only rows that exist (row < n_rows: rows past the end read as zero products) and are alive; a group without
// one is kKeyInvalid.  A NaN product drops out of the maximum (v_max3 / fmaxf: maxNum) — the sample need not hold every row — and so
// does -inf; +inf stays and closes the query's bound (wide_tau_key: not ok -> the gathered exact pass answers the query).
// The key's low word is the group's first live row: only the score half is read downstream, the row keeps the keys of a query unique
// (block_kth_hi_256 ranks whole keys).
// Needs: a, acc, rt, wr, wq, nq_t, q0, BM, mfma_drain(), lane_now().
    mfma_drain();  // the matrix pipe has written every accumulator before the vector ALU reads one
    {
      const uint32_t ln_s = lane_now();
      const uint32_t kk_s = ln_s >> 4;
      const uint32_t row_s = rt * (uint32_t)BM + (uint32_t)(wr * 128) + 4u * kk_s;  // the lane's first row
      const bool pair_s = a.sample_grp == 64u;                                         // (uniform)
      const uint32_t grp_s = pair_s ? (rt - a.row_tile0) * 4u + (uint32_t)wr * 2u + (kk_s >> 1) : (rt - a.row_tile0) * 8u + (uint32_t)wr * 4u + kk_s;
      const bool slow_s = a.alive != nullptr || a.n_rows - rt * (uint32_t)BM < (uint32_t)BM;  // (block-uniform) dead rows / the corpus' ragged tile
      uint32_t live_s = 0xFFFFFFFFu;  // bit 4 rf + r: the lane's row 16 rf + r counts
      uint32_t first_s = row_s;       // the lane's first live row (0xFFFFFFFF: none)
      if (slow_s) {
        live_s = 0u;
#pragma unroll
        for (int e = 0; e < 32; e++) {
          const uint32_t row = row_s + (uint32_t)((e >> 2) * 16 + (e & 3));
          bool lv = row < a.n_rows;
          if (lv && a.alive) lv = a.alive[row] != 0;
          live_s |= lv ? 1u << e : 0u;
        }
        const uint32_t e0 = live_s ? (uint32_t)__builtin_ctz(live_s) : 0u;
        first_s = live_s ? row_s + (e0 >> 2) * 16u + (e0 & 3u) : 0xFFFFFFFFu;
      }
      if (pair_s) {  // (every lane of a pair ends with the pair's first live row)
        auto r_ = __builtin_amdgcn_permlane16_swap(first_s, first_s, false, false);
        first_s = min((uint32_t)r_[0], (uint32_t)r_[1]);
      }
      // (volatile: the reads of the accumulators keep their place behind mfma_drain)
#define VDB_SMP_MAX3(M, A, B, C) asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(M) : "v"(A), "v"(B), "v"(C))
#pragma unroll
      for (int t = 0; t < 4; t++) {
        float mx;
        if (!slow_s) {  // the plain chain: 16 v_max3 over the lane's 32 accumulators of the column
          float m_[8];
#pragma unroll
          for (int rf = 0; rf < 8; rf++) VDB_SMP_MAX3(m_[rf], acc[rf][t][0], acc[rf][t][1], acc[rf][t][2]);
#pragma unroll
          for (int j = 0; j < 4; j++) VDB_SMP_MAX3(m_[j], m_[2 * j], m_[2 * j + 1], acc[2 * j][t][3]);
          VDB_SMP_MAX3(m_[0], m_[0], m_[1], acc[1][t][3]);
          VDB_SMP_MAX3(m_[2], m_[2], m_[3], acc[3][t][3]);
          VDB_SMP_MAX3(m_[0], m_[0], m_[2], acc[5][t][3]);
          VDB_SMP_MAX3(mx, m_[0], acc[7][t][3], acc[7][t][3]);
        } else {  // element by element under the lane's row mask
          mx = __uint_as_float(0xFF800000u);
#pragma unroll
          for (int e = 0; e < 32; e++) {
            float x;
            asm volatile("v_mov_b32 %0, %1" : "=v"(x) : "v"(acc[e >> 2][t][e & 3]));
            if ((live_s >> e) & 1u) mx = fmaxf(mx, x);
          }
        }
        if (pair_s) {
          auto r_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
          mx = fmaxf(__uint_as_float(r_[0]), __uint_as_float(r_[1]));
        }
        // (NaN and -inf: no key; a group without a live row has -inf)
        const uint64_t key = (mx > __uint_as_float(0xFF800000u) && first_s != 0xFFFFFFFFu) ? make_key<true>(mx, first_s) : kKeyInvalid;
        const uint32_t b = (uint32_t)(wq * 64 + t * 16) + (ln_s & 15u);
        if (b < nq_t && grp_s < a.list_stride && !(pair_s && (kk_s & 1u))) a.part_keys[(size_t)(q0 + b) * a.list_stride + grp_s] = key;
      }
#undef VDB_SMP_MAX3
    }
    // the one barrier the k-tile protocol needs: the last k-tile's closing barrier (as the WIDE instance's epilogue, g16_protocol.inc)
    __syncthreads();
