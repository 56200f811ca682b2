// vdb_select_hold.hpp — the selection stage's park-after-failure rule: host arithmetic only, nothing of HIP in it, so that
// tests/select_hold_model.cpp can run the four selectors' state machine on the CPU, in brute_dev's asking order.
//
// A finished selection batch posts its verdict {unproven, queries, sequence, level} to pinned host memory (sweep_split.hip
// select_finish_kernel: the sequence number last, behind a system fence).  Each selector (select_stage.hip select_level_wide,
// select_level, select_level_l2, select_level_sq8) reacts to the verdicts of ITS level only: more than 1/16 of a batch unproven
// means the handle's data defeats that selection, and the selector stands aside for the next `length` search calls it is asked in.
// Every selector keeps the sequence number it has looked at for itself: select_level_wide is asked first on every chunk, and with
// one shared number it consumed every verdict before the selectors behind it saw theirs.
#pragma once
#include <stdint.h>

namespace vdb {

constexpr uint32_t kSelectHoldBatches = 64;

struct SelectHold {
  uint32_t level;                        // the verdict level this selector reacts to: 4 WIDE, 2 bf16, 5 Euclidean, 3 SQ8
  uint32_t length = kSelectHoldBatches;  // batches a hold lasts
  uint32_t seen = 0;                     // sequence number of the last verdict looked at (0: none yet; the first posted is 1)
  uint32_t left = 0;                     // batches of the running hold still to come
  uint64_t asked_in = 0;                 // the search call of the last counted ask (0: none yet; the first call is 1)
  bool held = false;                     // ... and what it answered

  // One chunk the selector is otherwise eligible for: true = it is held (the caller's next tier answers).
  // `stats` may be null (no selection batch ran on this context so far).  `call` numbers the search calls of the context: a hold
  // counts CALLS — a call whose exact tier takes its queries a few at a time asks again for every chunk; the first answer stands
  // for the whole call and is counted once.
  bool ask(const volatile uint32_t* stats, uint64_t call) {
    if (stats) {
      const uint32_t seq = stats[2];  // first: a reader that sees the new sequence number sees the counts
      if (seq != seen) {
        seen = seq;
        if (stats[3] == level && (uint64_t)stats[0] * 16 > stats[1]) left = length;  // > 1/16 unproven
      }
    }
    if (asked_in == call) return held;
    asked_in = call;
    held = left != 0;
    if (held) left--;
    return held;
  }
};

// the four selectors of one search context; a filtered call copies the set and puts it back (its verdicts are not the handle's)
struct SelectHolds {
  SelectHold wide{4u}, sel16{2u}, l2{5u}, sq8{3u};
  uint64_t call = 0;  // search calls of the context so far (search_dev counts)
};

}  // namespace vdb
