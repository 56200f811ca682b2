"""What `last_select_level()` must report over 67 calls of 32 queries on a handle whose data defeats every selection (every verdict
more than 1/16 unproven), each verdict read before the next call — derived by reading the `select_level_*` rules
(velesdb_amd/csrc/select_stage.hip) over `vdb_select_hold.hpp`, default selector level 3.  Shared by the CPU model
(tests/test_select_hold_cpu.py) and the GPU trace test (tests/test_gpu_dev_sequences.py), so the two agree by construction.

Call 0 is WIDE (4).  Its verdict starts WIDE's hold of 64 batches at call 1, which therefore ends with call 64: call 65 is WIDE
again, fails again, and call 66 is back in the hold.  Below WIDE:
  * Cosine k = 10: call 1 is level 2; its verdict parks level 2 at call 2 (level 1 from there).  That hold of 64 has used 63 batches
    by call 64, so call 66 is its last: level 1.
  * Cosine k = 20: no level below WIDE takes k > 10: the exact kernels (0).
  * Euclidean k = 10: call 1 is the Euclidean level 2 (reported as 2, verdict level 5), parked from call 2: the exact tiers (0).
  * SQ8 storage mode, Cosine k = 10: call 1 is level 3, parked from call 2: the exact SQ8 sweep (0).
"""
CALLS = 67
TRACES = {
    "cosine_k10": [4, 2] + [1] * 63 + [4, 1],
    "cosine_k20": [4] + [0] * 64 + [4, 0],
    "euclidean_k10": [4, 2] + [0] * 63 + [4, 0],
    "sq8_cosine_k10": [4, 3] + [0] * 63 + [4, 0],
}
assert all(len(t) == CALLS for t in TRACES.values())
