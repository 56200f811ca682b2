// g16_protocol.inc — textually included right behind g16_quicktest.inc, once EVERY wave of the block has passed the same
// number of barriers: the hot lanes are looked at, survivors queued, appended to the candidate buffers and compacted, in rounds
// separated by block barriers (WIDE: the finish puts the survivors straight into the block's stash; one barrier, no rounds).
// Needs: what g16_quicktest.inc left (last, lane, halfp, hm, thrv, gmv, nvalid) + a, acc, rt, wr, wq, wib, nq_t, k,
// q0, qn, vns, tauk, cnts, cand, flags, wq_keys, wq_qs, qcnt, epoch, VDB_G16_ACC_ELEM(x, element), compact(), METRIC, HIB, BM, CAP, QCAP
// (QCAP <= 64).
#ifndef VDB_PP_STAMP_AT
#define VDB_PP_STAMP_AT(SLOT) do { } while (0)
#define VDB_G16_OWN_STAMP_STUB 1
#endif
#ifndef VDB_PP_STAMP_COUNT
#define VDB_PP_STAMP_COUNT(SLOT) do { } while (0)
#define VDB_PP_STAMP_ADD(SLOT, N) do { } while (0)
#endif
    VDB_PP_STAMP_AT(16);  // (stamped builds: 16 the lazy group masks, 17 scans, 18 finishes, 19 = epilogues in which this wave had a hot lane)
    if (hm[0] | hm[1] | hm[2] | hm[3]) VDB_PP_STAMP_COUNT(19);
    VDB_PP_STAMP_ADD(22, __popcll(hm[0]) + __popcll(hm[1]) + __popcll(hm[2]) + __popcll(hm[3]));  // (stamped builds: hot lanes, all epilogues)
    for (;;) {
      ++epoch;
      VDB_PP_STAMP_COUNT(23);  // (stamped builds: rounds)
      // ---- (1) look at the hot lanes.  SCAN: the hot lanes of a column group test their 32 elements one by one against the
      //      lane's bound (the quick test's, now per element); the lanes whose element passes leave it RAW — accumulator, row
      //      in tile, query column — behind the finished entries of the wave's queue (slot = fill + rank among the passing
      //      lanes: ballot + mbcnt, no LDS atomic — its return would be a round trip per element): ~6 instructions per
      //      element and ~12 per element with a push, whatever the number of hot lanes.  FINISH: the raw entries are finished
      //      densely, one per lane — exact score, key, test against the query's k-th best key — and the survivors compacted
      //      into the queue.  A scan whose pushes do not fit the queue is discarded and repeated over fewer hot lanes (hsz,
      //      sized from what the failed scan pushed; one lane's 32 elements always fit an empty queue); when even that does
      //      not fit, the wave asks for another round.  (Round 2's version gathered each hot lane's 32 elements with 32
      //      v_readlane + select and finished them on the spot: ~150 instructions per hot LANE — 12 of a row tile's 22 us
      //      under the thresholds of a launch's first tiles.) ----
      bool pend = false;
      {
        const uint32_t ln1 = lane_now();
        uint32_t fill = qcnt;  // finished + raw entries
        uint32_t hsz = 64u;    // hot lanes per scan
        bool stop = false;
#define VDB_G16_SCAN(T) \
        while (hm[T] && !stop) { \
          if (hsz == 1u && fill + 32u > (uint32_t)QCAP) { /* no room for a whole lane: finish what is there first */ \
            stop = true; \
            break; \
          } \
          const uint32_t hrank = __builtin_amdgcn_mbcnt_hi((uint32_t)(hm[T] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm[T], 0u)); \
          const bool mine = (((hm[T] >> ln1) & 1ull) != 0) & (hrank < hsz); \
          const uint64_t msk = __ballot(mine); \
          uint32_t nf = fill; \
          const uint32_t hi0 = ((uint32_t)(wr * 128) + 4u * (ln1 >> 4)) | (((uint32_t)(wq * 64 + (T) * 16) + (ln1 & 15u)) << 8); \
_Pragma("unroll") \
          for (int g8 = 0; g8 < 4; g8++) { \
            if (!__ballot(mine & (((gmv[T] >> g8) & 1u) != 0u))) continue; /* nobody's group of 8 can hold a survivor */ \
_Pragma("unroll") \
            for (int j8 = 0; j8 < 8; j8++) { \
              float x; \
              VDB_G16_ACC_ELEM(x, acc[(8 * g8 + j8) >> 2][T][(8 * g8 + j8) & 3]); /* read HERE (not a copy kept since the quick test: 128 live registers) */ \
              /* (Jaccard: the element's own |v| enters its test, as in the quick test; the raw entry keeps d) */ \
              const float xt = METRIC == kJaccard ? __builtin_fmaf(-cpv[T], vns[wr * 128 + 4 * (int)(ln1 >> 4) + ((8 * g8 + j8) >> 2) * 16 + ((8 * g8 + j8) & 3)], x) : x; \
              const bool pass = mine & !(xt < thrv[T]); \
              const uint64_t pm = __ballot(pass); \
              if (pm) { \
                if (pass) { \
                  const uint32_t slot = min(nf + __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u)), (uint32_t)QCAP); \
                  uint32_t hi = hi0; \
                  asm volatile("" : "+v"(hi)); /* (or all 128 sums are formed ahead of the loop and parked in scratch memory) */ \
                  wq_keys[slot] = ((uint64_t)(hi + (uint32_t)(((8 * g8 + j8) >> 2) * 16 + ((8 * g8 + j8) & 3))) << 32) | (uint64_t)__float_as_uint(x); \
                } \
                nf += (uint32_t)__popcll(pm); \
              } \
            } \
          } \
          if (nf > (uint32_t)QCAP) { /* did not fit (what it wrote is ignored: fill stays): fewer lanes */ \
            const uint32_t lanes = (uint32_t)__popcll(msk), room = (uint32_t)QCAP - fill; \
            hsz = lanes > 1u ? max(1u, min(lanes - 1u, lanes * room / (2u * (nf - fill)))) : 1u; \
            if (lanes == 1u) { /* (a single lane past a part-filled queue) */ \
              stop = true; \
              break; \
            } \
            continue; \
          } \
          fill = nf; \
          hm[T] &= ~msk; \
        }
        // FINISH of one raw entry per lane (RAW = query column << 40 | row in tile << 32 | accumulator bits; HAVE = the lane holds one): the
        // score the result carries, its key, the test against the query's k-th best key; the survivors are compacted behind the queue's
        // finished entries when they fit (FITS; nothing is written when they do not).
#define VDB_G16_FINISH(HAVE, RAW, FITS) do { \
          const uint64_t raw_ = (RAW); \
          const uint32_t b = (uint32_t)(raw_ >> 40) & 255u; \
          const float x = __uint_as_float((uint32_t)raw_); \
          const uint32_t rl = (uint32_t)(raw_ >> 32) & 255u; \
          const uint32_t row = rt * BM + rl; \
          float score; \
          if (METRIC == kHamming) {  /* simd_explicit.rs:234-287 on the +-1 re-encoding: q . v = dim - 2 |q ^ v|, qn[b] = dim */ \
            score = 0.5f * (qn[b] - x); \
          } else if (METRIC == kJaccard) {  /* simd_explicit.rs:431-442: intersection / union, 1.0 for an empty union */ \
            const float uni = qn[b] + vns[rl] - x; \
            score = uni == 0.0f ? 1.0f : x / uni; \
          } else { \
            score = halfp ? finish_score_half<METRIC>(x, qn[b], METRIC == kCosine ? vns[rl] : 1.0f) \
                          : finish_score<METRIC>(x, qn[b], METRIC == kCosine ? vns[rl] : 1.0f); \
          } \
          /* (WIDE: nothing behind the kernel vouches for a row it drops — the k <= 10 stage's proof sees a NaN bound and gives the query up. \
             A NaN approximate score — a NaN / inf component; its row is hot by the quick test's `force` rule — must therefore PASS whatever \
             its sign: +qNaN is the best key of a higher-is-better metric, the exact re-scoring then ranks the row where it belongs) */ \
          if constexpr (WIDE) score = canon_nan(score); \
          const uint64_t key = make_key<HIB>(score, row); \
          bool take = (HAVE) & (row < a.n_rows) & (key < tauk[b]); \
          if (take && a.alive) take = a.alive[row] != 0;  /* soft-deleted rows are filtered where it is rare */ \
          if constexpr (WIDE) { \
            /* WIDE: straight into the block's STASH — the query's CAP slots of the candidate buffers, which the instance keeps no list \
               in; cnts[b] counts every survivor, an LDS atomic (no device-scope round trip, nothing drains the LDS-DMA queue).  A full \
               slot row (rare) sends the entry to the query's global list on its own; the stash is flushed behind the last row tile \
               (g16_writeout.inc).  Nothing is queued: FITS always holds, qcnt stays 0 */ \
            if (take) { \
              const uint32_t si = atomicAdd(&cnts[b], 1u); \
              if (si < (uint32_t)CAP) { \
                cand[(size_t)b * CAP + si] = key; \
              } else { \
                const uint32_t qg = q0 + b; \
                const uint32_t gi = atomicAdd(&a.wide_cnt[qg], 1u); \
                if (gi < a.wide_cap) a.wide_keys[(size_t)qg * a.wide_cap + gi] = key; \
              } \
            } \
            FITS = true; \
          } else { \
          const uint64_t mt = __ballot(take); \
          FITS = qcnt + (uint32_t)__popcll(mt) <= (uint32_t)QCAP; \
          if (FITS) { \
            if (take) { \
              const uint32_t slot = qcnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mt >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mt, 0u)); \
              wq_keys[slot] = key; \
              wq_qs[slot] = (uint8_t)b; \
            } \
            qcnt += (uint32_t)__popcll(mt); \
          } \
          } \
        } while (0)
#ifndef VDB_G16_NO_DUMP  // (the lock-step kernel leaves it out: its k-loop pays for every scalar the epilogue keeps alive)
        // (Round 5, measured and rejected: a block-SHARED dump — every hot lane of the block copied into a stage slot no request targets
        // during an epilogue, all eight waves finishing the list together in a second round.  Balanced, and 2-7 % slower: the second round
        // (barrier, flag reads, an append pass) costs more than the wait it removes.  tools/probes/pp_shared_dump_experiment.patch,
        // profiles/r05r_*.)
        // FEW hot lanes (the steady state: a lane is hot in three of four wave tiles, one or two at a time — profiles/r05o_*): no scan.
        // The two lowest hot lanes of a column group leave their 32 accumulators each in the unused tail of the wave's queue (8
        // ds_write_b128 under their exec mask), and the wave finishes the 64 elements at once, one per lane.  The finish is the exact
        // test; the lane bound the scan applies first is only its necessary condition.  Needs qcnt <= 8 (the tail: entries 8 .. 39) and
        // the survivors to fit; otherwise — and beyond kG16DumpMaxLanes hot lanes, where the scan's cost per element wins — the scan
        // below takes what is left in hm[].
        if ((uint32_t)__popcll(hm[0]) + (uint32_t)__popcll(hm[1]) + (uint32_t)__popcll(hm[2]) + (uint32_t)__popcll(hm[3]) <= (uint32_t)kG16DumpMaxLanes) {
          bool dump_ok = true;
          if (hm[0] | hm[1] | hm[2] | hm[3]) VDB_PP_STAMP_COUNT(21);  // (stamped builds: look phases that start in the dump path)
          float* dump = reinterpret_cast<float*>(wq_keys + 8);
#define VDB_G16_DUMP(T) \
          while (hm[T] && dump_ok) { \
            if (qcnt > 8u) { \
              dump_ok = false; \
              break; \
            } \
            VDB_PP_STAMP_COUNT(24); /* (stamped builds: dump passes) */ \
            const uint32_t h0 = (uint32_t)__builtin_ctzll(hm[T]); \
            const uint64_t rest = hm[T] & (hm[T] - 1ull); \
            const uint32_t h1 = rest ? (uint32_t)__builtin_ctzll(rest) : 64u; \
            if (ln1 == h0 || ln1 == h1) { \
              f32x4* d = reinterpret_cast<f32x4*>(dump) + (ln1 == h1 ? 8 : 0); \
_Pragma("unroll") \
              for (int rf = 0; rf < 8; rf++) d[rf] = acc[rf][T]; \
            } \
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
            __builtin_amdgcn_wave_barrier(); \
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
            const uint32_t hs = ln1 < 32u ? h0 : h1;  /* the lane's element: e = ln1 & 31 of hot lane hs: row fragment e >> 2, register e & 3 */ \
            const uint32_t e = ln1 & 31u; \
            const float xd = dump[ln1]; \
            const uint32_t hi = ((((uint32_t)(wq * 64 + (T) * 16) + (hs & 15u)) << 8) | ((uint32_t)(wr * 128) + 4u * (hs >> 4) + (e >> 2) * 16u + (e & 3u))); \
            bool fits; \
            VDB_G16_FINISH(hs < 64u, ((uint64_t)hi << 32) | (uint64_t)__float_as_uint(xd), fits); \
            __builtin_amdgcn_wave_barrier();  /* every lane has read its element before the next pair is written */ \
            if (!fits) { \
              dump_ok = false; \
              break; \
            } \
            hm[T] = rest & (rest - 1ull); \
          }
          VDB_G16_DUMP(0)
          VDB_G16_DUMP(1)
          VDB_G16_DUMP(2)
          VDB_G16_DUMP(3)
#undef VDB_G16_DUMP
          fill = qcnt;
          VDB_PP_STAMP_AT(20);  // (stamped builds: the dump path)
        }
#endif
        // what the dump path left (or everything, when many lanes are hot) goes through the scan: the group masks of those columns,
        // once per row tile (later rounds only revisit lanes that were hot in the first)
        if (gm_lazy && (hm[0] | hm[1] | hm[2] | hm[3])) {  // (wave-uniform)
#define VDB_G16_MASKS(T) do { if (METRIC == kJaccard) VDB_G16_GROUP_MASKS_J(T); else VDB_G16_GROUP_MASKS(T); } while (0)
          if (hm[0]) VDB_G16_MASKS(0);
          if (hm[1]) VDB_G16_MASKS(1);
          if (hm[2]) VDB_G16_MASKS(2);
          if (hm[3]) VDB_G16_MASKS(3);
#undef VDB_G16_MASKS
          gm_lazy = false;
        }
        for (;;) {
          VDB_G16_SCAN(0)
          VDB_G16_SCAN(1)
          VDB_G16_SCAN(2)
          VDB_G16_SCAN(3)
          VDB_PP_STAMP_AT(17);
          if (fill > qcnt) {  // finish (QCAP <= 64: one entry per lane; every lane reads its entry before any survivor is written)
            const bool have = ln1 < fill - qcnt;
            const uint64_t raw = have ? wq_keys[qcnt + ln1] : 0ull;
            bool fits;
            VDB_G16_FINISH(have, raw, fits);  // (always fits: the survivors are among the raw entries, which did)
            (void)fits;
            fill = qcnt;
            VDB_PP_STAMP_AT(18);
          }
          if (!stop) break;
          if (qcnt + 32u > (uint32_t)QCAP) {  // the queue must be emptied first: another round
            pend = true;
            break;
          }
          stop = false;
        }
#undef VDB_G16_SCAN
#undef VDB_G16_FINISH
      }
      VDB_PP_STAMP_AT(12);  // look phase (scan + finish)
      if constexpr (WIDE) {
        // WIDE: every survivor is in the stash already and the bound does not move — no append, no round to repeat, no flags.  The one
        // barrier left is the last k-tile's closing barrier (the next row tile's norms land in vns, which every quick test has read)
        __syncthreads();
        VDB_PP_STAMP_AT(13);
        break;
      }
      // (flags[0] = the LATEST round somebody asked to repeat.  Nothing holds a wave back behind its own read of the word below, so a
      // fast wave may already be in round e + 1 — and mark it — while a slower one, still appending in round e, has not read yet: the
      // reader therefore tests `>= epoch`, not `== epoch` (a wave can only be in round e + 1 because round e WAS marked; epochs only
      // grow).  Round 6: with the WIDE instance's global atomics in the append a wave can be microseconds behind; under `==` it read the
      // next round's mark, left the protocol a round early and ran the rest of its block one barrier out of step — rows of single
      // wave tiles went missing at k >= 64, profiles/r06d_wide_rows_lost_before_the_flag_fix.log)
      if (pend || (last && qcnt)) flags[0] = epoch;
      __syncthreads();  // sync point `epoch` (first round: also the k-tile's closing barrier)
      VDB_PP_STAMP_AT(13);  // the sync point's barrier
      // ---- (2) buffers past k since the last sync point: compact them (everybody, between two barriers) ----
      if constexpr (!WIDE) {
      if (flags[1] == epoch) {
        compact();
        __syncthreads();
        VDB_PP_STAMP_AT(14);  // compaction + its barrier
      }
      }
      // ---- (3) append the queue to the candidate buffers; an entry whose buffer is full stays queued ----
      bool want = false;
      {
        const uint32_t ln3 = lane_now();  // (re-derived, not carried across the look phase: see lane_now)
        const uint64_t key = ln3 < qcnt ? wq_keys[ln3] : kKeyInvalid;
        const uint32_t b = ln3 < qcnt ? wq_qs[ln3] : 0u;
        bool full = false;
        if (key != kKeyInvalid && key < tauk[b]) {
          const uint32_t idx = atomicAdd(&cnts[b], 1u);
          if (idx < (uint32_t)CAP) {
            cand[(size_t)b * CAP + idx] = key;
            want = idx >= k;  // past k: the k-th best can be tightened
          } else {
            full = true;
            want = true;
          }
        }
        const uint64_t mf = __ballot(full);
        qcnt = (uint32_t)__popcll(mf);
        if (full) {
          const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(mf >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mf, 0u));
          wq_keys[slot] = key;  // slot <= lane and every lane has read its entry: no entry is overwritten before it is read
          wq_qs[slot] = (uint8_t)b;
        }
      }
      if (__ballot(want)) flags[1] = epoch + 1;
      VDB_PP_STAMP_AT(15);  // append
      bool again = flags[0] >= epoch;
      if (last) {  // the block's last row tile: everything still queued must get in before the lists are written out
        if (qcnt) flags[2] = epoch;
        __syncthreads();
        again |= flags[2] == epoch;
      }
      if (!again) break;
    }
#ifdef VDB_G16_OWN_STAMP_STUB
#undef VDB_PP_STAMP_AT
#undef VDB_G16_OWN_STAMP_STUB
#endif
