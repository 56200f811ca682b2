"""Shared inputs of tests/test_fusion_cpu.py and tests/test_gpu_fusion.py: the strategies, the adversarial groups the issue of the
fusion kernel names, a generator of random groups, the host model's loader (tests/fusion_model.cpp over csrc/vdb_fusion.hpp) and the
packing of groups into the arrays vdb_hip_fuse_results takes.  A group is a list of lists of (id, score)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL_SO = os.path.join(tempfile.gettempdir(), "vdb_fusion_model_%d" % os.getuid(), "libfusion_model.so")

U64_MAX = 0xFFFFFFFFFFFFFFFF
STRATEGIES = [("average",), ("maximum",), ("rrf", 60), ("rrf", 1), ("weighted", 0.6, 0.3, 0.1), ("weighted", 0.7, 0.3, 0.0)]
CODE = {"average": 0, "maximum": 1, "rrf": 2, "weighted": 3}


def abi(strategy):
    """(code, rrf_k, weights f32[3]) of a fusion_ref strategy tuple"""
    kind = strategy[0]
    w = np.array(strategy[1:4] if kind == "weighted" else (0, 0, 0), dtype=np.float32)
    return CODE[kind], (strategy[1] if kind == "rrf" else 0), w


def fusion_model():
    """The product's fusion rule on the host, built on first use (g++, -ffp-contract=off as the library)."""
    src = os.path.join(ROOT, "tests", "fusion_model.cpp")
    hdr = os.path.join(ROOT, "velesdb_amd", "csrc", "vdb_fusion.hpp")
    if not os.path.exists(_MODEL_SO) or os.path.getmtime(_MODEL_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(_MODEL_SO), exist_ok=True)
        tmp = _MODEL_SO + ".%d" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I",
                               os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", tmp, src])
        os.replace(tmp, _MODEL_SO)
    L = C.CDLL(_MODEL_SO)
    vp, u32 = C.c_void_p, C.c_uint32
    L.fusion_model_max_vectors.restype, L.fusion_model_max_vectors.argtypes = u32, []
    L.fusion_model_max_records.restype, L.fusion_model_max_records.argtypes = u32, []
    L.fusion_model_overfetch.restype, L.fusion_model_overfetch.argtypes = C.c_uint64, [u32]
    L.fusion_model_weights_error.restype, L.fusion_model_weights_error.argtypes = C.c_int, [C.c_float, C.c_float, C.c_float]
    L.fusion_model_fuse.restype, L.fusion_model_fuse.argtypes = C.c_int, [C.c_int, u32, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.fusion_model_fuse_groups.restype, L.fusion_model_fuse_groups.argtypes = C.c_int, [C.c_int, u32, vp, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    return L


def pack(groups):
    """groups -> (ids [n_lists][stride] u64, scores f32, list_n u32, group_sizes u32); stride >= 1"""
    lists = [l for g in groups for l in g]
    stride = max([len(l) for l in lists] + [1])
    ids = np.zeros((len(lists), stride), dtype=np.uint64)
    sc = np.zeros((len(lists), stride), dtype=np.float32)
    for j, l in enumerate(lists):
        for p, (i, s) in enumerate(l):
            ids[j, p], sc[j, p] = i, s
    return ids, sc, np.array([len(l) for l in lists], dtype=np.uint32), np.array([len(g) for g in groups], dtype=np.uint32)


def model_fuse(L, strategy, group, top_k):
    """one group through the host model -> (ids, score bits, n), padded arrays of max(top_k, 1)"""
    ids, sc, ln, _ = pack([group])
    code, k, w = abi(strategy)
    kk = max(top_k, 1)
    oi = np.full(kk, U64_MAX, dtype=np.uint64)
    ob = np.full(kk, 0x7FC00000, dtype=np.uint32)
    on = np.zeros(1, dtype=np.uint32)
    rc = L.fusion_model_fuse(code, k, w.ctypes.data, ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, len(group), ids.shape[1], top_k,
                             oi.ctypes.data, ob.ctypes.data, on.ctypes.data)
    assert rc == 0, rc
    return oi, ob, int(on[0])


def adversarial_groups():
    """{name: group}: what the kernel's sort, run detection and tie order can get wrong"""
    hi = 1 << 32
    rng = np.random.default_rng(41)
    big_ids = rng.integers(0, 300, size=(10, 200))
    big_sc = -np.sort(-rng.standard_normal((10, 200)).astype(np.float32), axis=1)
    return {
        "duplicates_inside_a_list": [[(1, 0.9), (1, 0.8), (2, 0.7), (1, 0.95)], [(2, 0.6), (2, 0.65), (3, 0.5)]],
        "empty_lists_among_others": [[], [(1, 0.9), (2, 0.8)], [], [(2, 0.85), (3, 0.75)], []],
        "all_lists_empty": [[], [], []],
        "no_lists": [],
        "one_list": [[(7, 0.5), (3, 0.4), (9, 0.3)]],
        "ten_lists": [[(int(i), float(np.float32(1.0 - 0.01 * p - 0.001 * q))) for p, i in enumerate(range(q, q + 12))] for q in range(10)],
        "ids_zero_and_max": [[(0, 0.9), (U64_MAX, 0.8), (5, 0.7)], [(U64_MAX, 0.95), (0, 0.1)], [(U64_MAX, 0.2)]],
        "ids_differ_in_one_half": [[(5, 0.9), (hi | 5, 0.8), (2 * hi | 5, 0.7), (6, 0.6)], [(hi | 6, 0.9), (hi | 5, 0.85), (5, 0.8), (2 * hi | 6, 0.1)],
                                   [(2 * hi | 5, 0.3), (hi, 0.2), (1, 0.1)]],
        "negative_and_minus_zero": [[(1, -0.5), (2, -0.0), (3, -1.5), (4, 0.0)], [(2, -0.0), (1, -0.25), (4, 0.0), (3, -3.0)], [(3, -0.0), (5, -1e-38)]],
        "mixed_zeros_for_one_id": [[(1, 0.0), (1, -0.0), (2, -0.0), (2, 0.0)], [(1, -0.0), (2, 0.0)]],
        "reversed_pair_all_tie": [[(11, 0.9), (4, 0.8)], [(4, 0.7), (11, 0.6)]],
        "reversed_lists_pairwise_ties": [[(i, 1.0 - 0.1 * p) for p, i in enumerate([9, 3, 7, 1, 8, 2])],
                                         [(i, 1.0 - 0.1 * p) for p, i in enumerate([2, 8, 1, 7, 3, 9])]],
        "equal_scores_everywhere": [[(i, 0.5) for i in (40, hi | 1, 3, U64_MAX, 0)], [(i, 0.5) for i in (0, 3, 40)]],
        "ten_by_two_hundred": [[(int(i), float(s)) for i, s in zip(big_ids[q], big_sc[q])] for q in range(10)],
    }


def random_group(rng):
    V = int(rng.integers(0, 11))
    universe = int(rng.choice([3, 8, 40]))
    base = [0, 1 << 32, U64_MAX - 64][int(rng.integers(0, 3))]
    group = []
    for _ in range(V):
        n = int(rng.integers(0, 13))
        sc = rng.standard_normal(n).astype(np.float32)
        if rng.random() < 0.3:
            sc = np.round(sc * 2) / 2          # many equal scores
        sc = -np.sort(-sc)
        ids = rng.integers(0, universe, size=n)
        group.append([(base + int(i), float(s)) for i, s in zip(ids, sc)])
    return group


def sized_group(n_records, rng, universe=None):
    """a group of exactly n_records records in up to ten lists, ids drawn with repetition"""
    V = min(10, n_records)
    cuts = sorted(rng.choice(np.arange(1, n_records), size=V - 1, replace=False).tolist()) if V > 1 else []
    lens = np.diff([0] + cuts + [n_records])
    universe = universe or max(2, n_records // 3)
    return [[(int(i), float(s)) for i, s in zip(rng.integers(0, universe, size=n), -np.sort(-rng.standard_normal(n).astype(np.float32)))]
            for n in lens]
