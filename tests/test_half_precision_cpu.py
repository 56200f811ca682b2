"""CPU tier of the half-precision rows (VectorPrecision::{F16, BF16}, half_precision.rs): the numpy reference the GPU tests compare
with (tests/half_ref.py) against the reference's own F16 literals (tests/golden/half_precision_f16_literals.json, values with
file:line) and against the oracle's bf16 functions where the two overlap; the new surface of the C ABI and of its Python mirror; and
what the compiler made of the new kernels (an f16 matrix-core instruction is in the library, the half-row Euclidean sweep uses no
scratch)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import half_ref as hr  # noqa: E402

HEADER = os.path.join(ROOT, "include", "velesdb_hip.h")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "half_precision_f16_literals.json")))
F = np.float32


def gen(dim, seed):   # generate_test_vector, half_precision_tests.rs:7-10
    return np.sin(F(seed) + np.arange(dim, dtype=F) * F(0.1), dtype=F)


# ---- the helper against the reference's literals -------------------------------------------------------------------------------
def test_reference_f16_literals():
    g = GOLDEN["dot_product_f16"]
    s = hr.scores(hr.DOT, hr.F16, np.array([g["b"]], F), np.array([g["a"]], F))[0, 0]
    assert abs(s - g["expected"]) < g["tolerance"] and s == F(32.0)          # small integers: exact
    g = GOLDEN["cosine_identical_f16"]
    v = gen(g["dim"], g["seed"])[None, :]
    assert abs(hr.scores(hr.COSINE, hr.F16, v, v)[0, 0] - g["expected"]) < g["tolerance"]
    g = GOLDEN["euclidean_f16"]
    s = hr.scores(hr.EUCLIDEAN, hr.F16, np.array([g["b"]], F), np.array([g["a"]], F))[0, 0]
    assert abs(s - g["expected"]) < g["tolerance"] and s == F(5.0)
    g = GOLDEN["ranking_f16"]
    q, rows = gen(g["dim"], g["query_seed"])[None, :], np.stack([gen(g["dim"], g["close_seed"]), gen(g["dim"], g["far_seed"])])
    for prec in (hr.F32, hr.F16):
        close, far = hr.scores(hr.COSINE, prec, rows, q)[0]
        assert close > far, prec
    g = GOLDEN["roundtrip_f16"]
    orig = np.array(g["values"], F)
    assert np.max(np.abs(hr.round_half(orig, hr.F16) - orig)) < g["max_abs_error"]


def test_f16_rounding_is_ieee_round_to_nearest_even():
    two = lambda e: F(2.0) ** F(e)  # noqa: E731
    x = np.array([65504.0, 65519.99, 65520.0, -65520.0, 1e30,                  # largest finite, just below the halfway point, halfway -> inf
                  2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26, 3 * 2.0 ** -25,   # subnormals, underflow ties
                  1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 0.0, -0.0], F)
    exp = np.array([65504.0, 65504.0, np.inf, -np.inf, np.inf,
                    2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 0.0, 2.0 ** -24, 0.0, 2.0 ** -23,               # 1.5 ulp -> 2 ulp (even)
                    1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, 0.0, -0.0], F)
    got = hr.round_half(x, hr.F16)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (got, exp)
    assert two(-24) == got[5]


def test_sequential_chain_is_a_plain_loop():
    rng = np.random.default_rng(3)
    q, r = hr.round_half(rng.standard_normal((2, 37)), hr.F16), hr.round_half(rng.standard_normal((3, 37)), hr.F16)
    dot, l2 = hr.seq_dot(q, r), hr.seq_l2(q, r)
    for i in range(2):
        for j in range(3):
            a, b = F(0.0), F(0.0)
            for t in range(37):
                a = F(a + F(q[i, t] * r[j, t]))
                d = F(q[i, t] - r[j, t])
                b = F(b + F(d * d))
            assert a == dot[i, j] and np.sqrt(b) == l2[i, j]


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_helper_equals_the_oracle_where_they_overlap(metric):
    po = pytest.importorskip("oracle.pyoracle")
    rng = np.random.default_rng(11)
    x = rng.standard_normal(5000).astype(F) * F(100.0)
    assert np.array_equal(hr.round_half(x, hr.BF16).view(np.uint32), po.round_bf16(x).view(np.uint32))
    rows, qs = rng.standard_normal((700, 100)).astype(F), rng.standard_normal((9, 100)).astype(F)
    pm, m = (po.COSINE, hr.COSINE) if metric == "cosine" else (po.DOT, hr.DOT)
    eid, esc = po.scan_topk_bf16(pm, rows, qs, 10)
    gid, gsc, kk = hr.scan_topk(m, hr.BF16, rows, qs, 10)
    assert kk == 10 and np.array_equal(gid, eid) and np.array_equal(gsc.view(np.uint32), esc.view(np.uint32))


def test_exact_f16_grid_is_exact_and_not_representable_in_bf16():
    # the data of the GPU file's case (b): odd multiples of 1/256 in +-[257/256, 511/256], dim 64 — every product, every partial sum of the
    # dot product and of (q - v)^2 is exact in f32 whatever the order; bf16 rounding changes every element and the top-10
    rng = np.random.default_rng(8)
    def grid(shape):
        return ((2 * rng.integers(128, 256, shape) + 1) / 256.0 * rng.choice([-1.0, 1.0], shape)).astype(F)
    rows, qs = grid((400, 64)), grid((6, 64))
    assert np.array_equal(hr.round_half(rows, hr.F16), rows) and np.all(hr.round_half(rows, hr.BF16) != rows)
    r64, q64 = rows.astype(np.float64), qs.astype(np.float64)
    assert np.array_equal(hr.seq_dot(qs, rows).astype(np.float64), q64 @ r64.T)
    d2 = ((q64[:, None, :] - r64[None, :, :]) ** 2).sum(2)
    assert np.array_equal(hr.seq_l2(qs, rows), np.sqrt(d2).astype(F))
    a, _, _ = hr.scan_topk(hr.DOT, hr.F16, rows, qs, 10)
    b, _, _ = hr.scan_topk(hr.DOT, hr.BF16, rows, qs, 10)
    assert not np.array_equal(a, b)


# ---- the new surface: header, library, Python mirror (all of these fail without the feature) ------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_half_precision_surface():
    src = header_text()
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", src))
    assert re.search(r"int32_t\s+vdb_hip_index_enable_half_precision\s*\(\s*vdb_hip_index\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert enums["VDB_SEARCH_BRUTE_F16"] == 7
    assert (enums["VDB_PRECISION_F32"], enums["VDB_PRECISION_F16"], enums["VDB_PRECISION_BF16"]) == (0, 1, 2)
    assert "enum vdb_vector_precision" in src
    new_bits = [enums["VDB_KERNEL_F16"], enums["VDB_KERNEL_SWEEP_HALF_L2"]]
    assert all(b >= 8192 and b & (b - 1) == 0 for b in new_bits) and new_bits[0] != new_bits[1]
    older = [v for k, v in enums.items() if k.startswith("VDB_KERNEL_") and k not in ("VDB_KERNEL_F16", "VDB_KERNEL_SWEEP_HALF_L2")]
    assert not set(new_bits) & set(older)


def test_library_and_python_mirror_expose_it():
    import velesdb_amd as va
    from velesdb_amd import _ffi
    assert hasattr(C.CDLL(_ffi.LIB_PATH), "vdb_hip_index_enable_half_precision")
    assert "vdb_hip_index_enable_half_precision" in _ffi.SIGNATURES
    src = header_text()
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(VDB_[A-Z0-9_]+)\s*=\s*(-?\d+)", src))
    assert va.MODE_BRUTE_F16 == enums["VDB_SEARCH_BRUTE_F16"]
    assert va.KERNEL_F16 == enums["VDB_KERNEL_F16"] and va.KERNEL_SWEEP_HALF_L2 == enums["VDB_KERNEL_SWEEP_HALF_L2"]
    assert [int(p) for p in (va.VectorPrecision.F32, va.VectorPrecision.F16, va.VectorPrecision.BF16)] == [0, 1, 2]
    assert callable(va.HnswIndex.enable_half_precision) and callable(va.HnswIndex.search_batch_brute_force_half)
    rs = open(os.path.join(ROOT, "velesdb-hip", "src", "lib.rs")).read()
    for item in ("pub enum VectorPrecision", "pub fn enable_half_precision", "pub fn search_batch_brute_force_half"):
        assert item in rs, item


# ---- what the compiler made of the new kernels -----------------------------------------------------------------------------------
def test_f16_matrix_instruction_and_spill_free_half_row_sweep():
    pytest.importorskip("msgpack")
    import kernel_resources as kr
    if not os.path.exists(kr.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    ks = kr.kernels()
    l2 = [k for k in ks if kr.family(k["name"]) == "sweep_topk_half_l2"]
    assert len(l2) == 6, [k["name"] for k in l2]                         # {f16, bf16} x query tiles of 16 / 4 / 1
    for k in l2:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"] and k["waves_per_simd"] >= 3, k
    f16 = [k for k in ks if kr.family(k["name"]) == "sweep_topk_gemm_f16_pp"
           or (kr.family(k["name"]) in ("sweep_topk_mfma_bf16", "sweep_topk_gemm_f32") and k["name"].rstrip(">").endswith(", true"))]
    assert len(f16) >= 2 + 8 + 8, [k["name"] for k in f16]
    with_f16 = 0
    for oi in sorted({k["obj"] for k in f16}):
        funcs = kr.disassemble(kr.code_objects()[oi])
        for k in f16:
            if k["obj"] != oi:
                continue
            body = [x for _, b in funcs[k["symbol"]] for x in b]
            n16, nbf = kr.count(body, "v_mfma_f32_16x16x32_f16"), kr.count(body, "v_mfma_f32_16x16x32_bf16")
            assert n16 > 0 and nbf == 0, (k["name"], n16, nbf)             # an f16 instance multiplies f16, only
            with_f16 += 1
        for k in l2:
            if k["obj"] == oi:
                body = [x for _, b in funcs[k["symbol"]] for x in b]
                assert kr.count(body, "scratch_") == 0 and kr.count(body, "flat_") == 0 and kr.count(body, "v_mfma") == 0, k["name"]
    assert with_f16 == len(f16)
    for oi in sorted({k["obj"] for k in l2}):
        funcs = kr.disassemble(kr.code_objects()[oi])
        for k in l2:
            body = [x for _, b in funcs[k["symbol"]] for x in b]
            assert kr.count(body, "scratch_") == 0 and kr.count(body, "flat_") == 0, k["name"]
            conv = kr.count(body, "v_cvt_f32_f16")
            assert (conv > 0) == ("<true" in k["name"]), (k["name"], conv)  # the f16 instance converts with v_cvt_f32_f16, bf16 by shifts
    # the f16 ping-pong instances obey the selection kernel's register rules (tests/test_kernel_resources_cpu.py pins the bf16 ones)
    for k in ks:
        if kr.family(k["name"]) == "sweep_topk_gemm_f16_pp":
            assert k["agpr"] == 0 and 224 <= k["vgpr"] <= 256 and k["block"] == 512 and k["waves_per_simd"] == 2 and k["scratch"] == 0, k
