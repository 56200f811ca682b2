"""Shared inputs of tests/test_hybrid_cpu.py and tests/test_gpu_hybrid.py: the adversarial user queries the issue of the hybrid kernel
names, a generator of random ones, the host model's loader (tests/hybrid_model.cpp over csrc/vdb_hybrid.hpp) and the packing of
queries into the arrays vdb_hip_hybrid_fuse takes.  A case is a dict: V / T = id lists (best first), w = vector_weight (None = the
default), dead = text ids that are unknown to the handle or removed, allowed = the filter's ids (None = the unfiltered form)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import hybrid_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL_SO = os.path.join(tempfile.gettempdir(), "vdb_hybrid_model_%d" % os.getuid(), "libhybrid_model.so")

U64_MAX = 0xFFFFFFFFFFFFFFFF
WEIGHTS = [0.0, 1.0, 0.5, 0.3, -2.0, 7.0, float("inf")]
LIVE, ALLOWED = 1, 2


def hybrid_model():
    """The product's hybrid rule on the host, built on first use (g++, -ffp-contract=off as the library)."""
    src = os.path.join(ROOT, "tests", "hybrid_model.cpp")
    hdrs = [os.path.join(ROOT, "velesdb_amd", "csrc", h) for h in ("vdb_hybrid.hpp", "vdb_fusion.hpp")]
    so = _MODEL_SO
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I",
                               os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.hybrid_model_max_records.restype, L.hybrid_model_max_records.argtypes = u32, []
    L.hybrid_model_default_weight_bits.restype, L.hybrid_model_default_weight_bits.argtypes = u32, []
    L.hybrid_model_clamp.restype, L.hybrid_model_clamp.argtypes = C.c_int, [C.c_float, vp]
    L.hybrid_model_fuse.restype, L.hybrid_model_fuse.argtypes = C.c_int, [vp, u32, vp, vp, u32, C.c_float, C.c_int, u32, vp, vp, vp]
    L.hybrid_model_fuse_batch.restype, L.hybrid_model_fuse_batch.argtypes = C.c_int, [vp, vp, u32, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    return L


def case(V=(), T=(), w=None, dead=(), allowed=None):
    return {"V": [int(i) for i in V], "T": [int(i) for i in T], "w": w, "dead": set(dead), "allowed": None if allowed is None else set(allowed)}


def reference(c, k, all_live=False):
    """the restatement's answer for a case: [(id, score)]"""
    if all_live:
        return hr.hybrid(c["V"], c["T"], k, c["w"])
    if c["allowed"] is not None:
        return hr.hybrid_filtered(c["V"], c["T"], k, c["w"], lambda i: i not in c["dead"] and i in c["allowed"])
    return hr.hybrid(c["V"], c["T"], k, c["w"], lambda i: i not in c["dead"])


def model_fuse(L, c, k, raw_weight=None):
    """a case through the host model -> (rc, ids, score bits, n), padded arrays of max(k, 1)"""
    V = np.array(c["V"], dtype=np.uint64)
    T = np.array(c["T"], dtype=np.uint64)
    filtered = c["allowed"] is not None
    flags = np.array([(0 if t in c["dead"] else LIVE) | (ALLOWED if filtered and t not in c["dead"] and t in c["allowed"] else 0) for t in c["T"]],
                     dtype=np.uint8)
    kk = max(k, 1)
    oi = np.full(kk, hr.PAD_ID, dtype=np.uint64)
    ob = np.full(kk, hr.PAD_SCORE, dtype=np.uint32)
    on = np.zeros(1, dtype=np.uint32)
    w = raw_weight if raw_weight is not None else (0.5 if c["w"] is None else c["w"])
    rc = L.hybrid_model_fuse(V.ctypes.data, V.size, T.ctypes.data, flags.ctypes.data, T.size, w, int(filtered), k, oi.ctypes.data, ob.ctypes.data,
                             on.ctypes.data)
    return rc, oi, ob, int(on[0])


def pack(cases):
    """cases -> (vec_ids [nq][vs] u64, vec_n, text_ids [nq][ts] u64, text_n, weights f32 [nq]); strides >= 1; w None -> 0.5"""
    vs = max([len(c["V"]) for c in cases] + [1])
    ts = max([len(c["T"]) for c in cases] + [1])
    vi = np.zeros((len(cases), vs), dtype=np.uint64)
    ti = np.zeros((len(cases), ts), dtype=np.uint64)
    for j, c in enumerate(cases):
        vi[j, :len(c["V"])] = np.array(c["V"], dtype=np.uint64)
        ti[j, :len(c["T"])] = np.array(c["T"], dtype=np.uint64)
    return (vi, np.array([len(c["V"]) for c in cases], dtype=np.uint32), ti, np.array([len(c["T"]) for c in cases], dtype=np.uint32),
            np.array([0.5 if c["w"] is None else c["w"] for c in cases], dtype=np.float32))


def distinct(c):
    return len(set(c["V"]) | set(c["T"]))


def adversarial_cases():
    """{name: case}: what the kernel's compaction, sort, run fold, tie order and cut can get wrong"""
    hi = 1 << 32
    out = {
        "empty_vector_list": case([], [5, 3, 9]),
        "empty_text_list": case([5, 3, 9], []),
        "both_empty": case([], []),
        "lists_equal": case([7, 3, 9, 1], [7, 3, 9, 1]),
        "reversed_every_id_ties_pairwise": case([9, 3, 7, 1, 8, 2], [2, 8, 1, 7, 3, 9], 0.5),
        "duplicates_inside_the_text_list": case([1, 2, 3], [2, 2, 4, 2, 4], 0.3),
        "duplicates_inside_the_vector_list": case([1, 1, 2, 1], [2, 3], 0.7),
        "ids_zero_and_max": case([0, U64_MAX, 5], [U64_MAX, 0, 6], 0.5),
        "ids_differ_in_one_half": case([5, hi | 5, 2 * hi | 5, 6], [hi | 6, hi | 5, 5, 2 * hi | 6, hi, 1], 0.5),
        # order under the key: 100 101 102 103 104 | 1 2 3 — 101 sits inside a cut at 3, 102 at it, 103 just outside
        "non_live_text_ids_around_the_cut": case([1, 2, 3], [100, 101, 102, 103, 104], 0.3, dead=[101, 102, 103]),
        "filter_rejects_every_text_hit": case([1, 2, 3], [100, 2, 101, 102], 0.5, allowed=[1, 3]),
        "filter_keeps_some_text_hits": case([1, 2, 3], [100, 2, 101, 3, 102, 2], 0.4, dead=[101], allowed=[1, 2, 3, 101, 102]),
        "filter_and_no_vector_list": case([], [4, 5, 6, 7], 0.5, dead=[5], allowed=[4, 5, 7]),
        "filter_rejects_everything": case([], [4, 5, 6], 0.5, allowed=[]),
    }
    base = case([11, 4, 8, 15, 16], [23, 8, 42, 11, 4, 4])
    for w in WEIGHTS:
        out["weight_%s" % w] = dict(base, w=w)
    out["weight_default"] = dict(base, w=None)
    return out


def cut_points(c):
    D = distinct(c)
    return sorted({0, 1, max(D - 1, 0), D, D + 1, 4 * D})


def random_case(rng):
    universe = int(rng.choice([3, 8, 40]))
    base = [0, 1 << 32, U64_MAX - 64][int(rng.integers(0, 3))]
    V = [base + int(i) for i in rng.integers(0, universe, size=int(rng.integers(0, 13)))]
    T = [base + int(i) for i in rng.integers(0, universe, size=int(rng.integers(0, 13)))]
    if rng.random() < 0.5:
        V = list(dict.fromkeys(V))          # (a walk's list holds an id once)
    w = [None, 0.5, 0.0, 1.0, float(rng.random()), float(rng.standard_normal() * 2)][int(rng.integers(0, 6))]
    dead = [t for t in set(T) - set(V) if rng.random() < 0.3]
    allowed = None
    if rng.random() < 0.4:
        allowed = set(V) | {t for t in set(T) if rng.random() < 0.6}
    return case(V, T, w, dead, allowed)


def sized_case(n_records, rng, w=0.5):
    """exactly n_records ids in the two lists together, ids drawn with repetition across (and inside) the lists"""
    nv = int(rng.integers(0, n_records + 1))
    universe = max(2, n_records // 2)
    base = 1 << 33
    V = [base + int(i) for i in rng.permutation(max(universe, nv))[:nv]]
    T = [base + int(i) for i in rng.integers(0, universe, size=n_records - nv)]
    return case(V, T, w)
