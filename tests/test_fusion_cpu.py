"""CPU tier of the multi-query search with result fusion: no GPU needed.

  * tests/fusion_ref.py — the numpy-float32 restatement of FusionStrategy::fuse — satisfies every case of the reference's own
    fusion/strategy_tests.rs (tests/golden/fusion_kats.json: inputs, assertions and tolerances as data);
  * the PRODUCT's rule — csrc/vdb_fusion.hpp, the text fuse_lists_kernel is written over, compiled for the host by
    tests/fusion_model.cpp — equals the restatement bit for bit on the adversarial groups and on a few thousand random ones;
  * the over-fetch table and the weight validation (sums evaluated in f32);
  * the header, the built library and the ctypes binding carry the two entry points, the enum and VDB_KERNEL_FUSE, and the argument
    checks that need no device answer as documented.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import fusion_cases as fc
import fusion_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "fusion_kats.json")))
INVALID, UNSUPPORTED = -1, -7


@pytest.fixture(scope="module")
def model():
    return fc.fusion_model()


def _check(check, fused, fixture):
    kind = check["kind"]
    score = {i: s for i, s in fused}
    if kind == "nonempty":
        assert fused
    elif kind == "empty":
        assert fused == []
    elif kind == "len":
        assert len(fused) == check["n"]
    elif kind == "sorted_desc":
        assert all(fused[i - 1][1] >= fused[i][1] for i in range(1, len(fused)))
    elif kind == "score_near":
        assert np.abs(F(score[check["id"]] - F(check["value"]))) < F(check["tol"]), (check, score[check["id"]])
    elif kind == "first_score_near":
        assert np.abs(F(fused[0][1] - F(check["value"]))) < F(check["tol"])
    elif kind == "score_gt":
        assert score[check["id"]] > F(check["value"])
    elif kind == "score_gt_under":
        other = dict(fr.fuse(tuple(check["other_strategy"]), fixture))
        assert score[check["id"]] > other[check["id"]]
    elif kind == "first_gt_second":
        assert fused[0][1] > fused[1][1]
    elif kind == "id_scores_above":
        assert score[check["id"]] > score[check["other_id"]]
    elif kind == "ids_present":
        assert set(check["ids"]) <= set(score)
    elif kind == "id_count":
        assert sum(1 for i, _ in fused if i == check["id"]) == check["n"]
    elif kind == "all_scores_between":
        assert all(F(check["lo"]) <= s <= F(check["hi"]) for _, s in fused)
    elif kind == "all_scores_gt":
        assert all(s > F(check["value"]) for _, s in fused)
    else:
        raise AssertionError("unknown check " + kind)


@pytest.mark.parametrize("case", KATS["cases"], ids=lambda c: c["name"])
def test_restatement_satisfies_the_reference_kats(case):
    fixture = [[(i, s) for i, s in q] for q in KATS["fixtures"][case["fixture"]]]
    fused = fr.fuse(tuple(case["strategy"]), fixture)
    assert len({i for i, _ in fused}) == len(fused)
    for check in case["checks"]:
        _check(check, fused, fixture)


def test_model_satisfies_the_reference_kats(model):
    for case in KATS["cases"]:
        fixture = [[(i, s) for i, s in q] for q in KATS["fixtures"][case["fixture"]]]
        ids, sb, n = fc.model_fuse(model, tuple(case["strategy"]), fixture, 64)
        fused = [(int(ids[j]), sb[j:j + 1].view(np.float32)[0]) for j in range(n)]
        for check in case["checks"]:
            _check(check, fused, fixture)


def test_reference_weight_validation_cases(model):
    assert KATS["rrf_default_k"] == 60
    for v in KATS["weighted_validation"]:
        assert (fr.weighted_error(*v["weights"]) is None) == v["valid"], v
        assert (model.fusion_model_weights_error(*v["weights"]) == 0) == v["valid"], v


def _same(model, strategy, group, top_k):
    want = fr.fuse_top(strategy, group, top_k)
    got = fc.model_fuse(model, strategy, group, top_k)
    assert got[2] == want[2], (strategy, top_k, got[2], want[2])
    assert np.array_equal(got[0], want[0]), (strategy, top_k, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (strategy, top_k, got[1], want[1])
    return want


@pytest.mark.parametrize("name", sorted(fc.adversarial_groups()))
def test_model_equals_restatement_on_adversarial_groups(model, name):
    group = fc.adversarial_groups()[name]
    strategies = fc.STRATEGIES if name != "ten_by_two_hundred" else fc.STRATEGIES[:3] + fc.STRATEGIES[4:5]
    for strategy in strategies:
        full = fr.fuse(strategy, group)
        for top_k in sorted({0, 1, max(len(full) - 1, 0), len(full), len(full) + 1, len(full) + 7}):
            if name == "ten_by_two_hundred" and top_k not in (len(full), 10):
                continue
            _same(model, strategy, group, top_k)
    if name in ("all_lists_empty", "no_lists"):
        assert fr.fuse(("rrf", 60), group) == []


def test_ties_are_decided_by_id(model):
    g = fc.adversarial_groups()
    ids, sb, n = _same(model, ("rrf", 60), g["reversed_pair_all_tie"], 5)
    assert n == 2 and list(ids[:2]) == [4, 11] and sb[0] == sb[1]
    ids, sb, n = _same(model, ("rrf", 60), g["reversed_lists_pairwise_ties"], 6)
    assert list(ids[:6]) == [2, 9, 3, 8, 1, 7] and sb[0] == sb[1] and sb[2] == sb[3] and sb[4] == sb[5]
    ids, sb, n = _same(model, ("maximum",), g["equal_scores_everywhere"], 9)
    assert list(ids[:n]) == [0, 3, 40, (1 << 32) | 1, fc.U64_MAX]


def test_model_equals_restatement_on_random_groups(model):
    rng = np.random.default_rng(20260)
    for t in range(3000):
        group = fc.random_group(rng)
        strategy = fc.STRATEGIES[t % len(fc.STRATEGIES)]
        if t % 7 == 0:
            strategy = ("rrf", int(rng.choice([0, 7, 1000, 4294967295])))
        _same(model, strategy, group, int(rng.choice([1, 3, 10, 200])))


def test_overfetch_table(model):
    want = {0: 0, 1: 20, 10: 200, 11: 110, 50: 500, 51: 255, 100: 500, 101: 202}
    for top_k, k in want.items():
        assert fr.overfetch(top_k) == k and model.fusion_model_overfetch(top_k) == k, top_k
    assert model.fusion_model_overfetch(0xFFFFFFFF) == 2 * 0xFFFFFFFF   # (no wrap: the caller sees the product)
    assert model.fusion_model_max_vectors() == 10 == fr.MAX_VECTORS and model.fusion_model_max_records() == 8192


def test_weight_validation_in_f32(model):
    import velesdb_amd as va
    # sums the issue names, evaluated in f32: (a + m) + h, |sum - 1| > 0.001 is invalid
    cases = [((0.5, 0.3, 0.1989), False), ((0.5, 0.3, 0.1991), True), ((0.5, 0.3, 0.2009), True), ((0.5, 0.3, 0.2011), False),
             ((0.6, 0.3, 0.1), True), ((1.0, 0.0, 0.0), True), ((0.0, 0.0, 0.0), False), ((-0.1, 0.6, 0.5), False), ((0.6, -0.0, 0.4), True),
             ((float("nan"), 0.5, 0.5), False), ((0.5, float("nan"), 0.5), False), ((0.5, 0.5, float("nan")), False),
             ((float("inf"), 0.0, 0.0), False)]
    for w, valid in cases:
        a, m, h = (F(x) for x in w)
        if not any(np.isnan(x) for x in (a, m, h)) and min(a, m, h) >= 0 and np.isfinite(a + m + h):
            assert valid == (not (np.abs(F(F(F(a + m) + h) - F(1.0))) > F(0.001))), w    # the table above IS the f32 rule
        assert (fr.weighted_error(*w) is None) == valid, w
        assert (model.fusion_model_weights_error(*w) == 0) == valid, w
        if valid:
            assert va.FusionStrategy.Weighted(*w).code == 3
        else:
            with pytest.raises(va.FusionError) as e:
                va.FusionStrategy.Weighted(*w)
            assert ("non-negative" in str(e.value)) == (fr.weighted_error(*w) == "negative")
    assert model.fusion_model_weights_error(-0.1, 0.6, 0.5) == 1 and model.fusion_model_weights_error(0.5, 0.3, 0.1) == 2
    assert va.FusionStrategy.rrf_default() == va.FusionStrategy.RRF(60) and va.FusionStrategy.RRF().rrf_k == 60


def test_header_library_and_binding_carry_the_feature():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "velesdb_hip.h")).read(), flags=re.S)
    for name in ("vdb_hip_fuse_results", "vdb_hip_index_multi_query_search"):
        assert re.search(r"int32_t\s+" + name + r"\s*\(", hdr), name
        assert name in _ffi.SIGNATURES
    enum = re.search(r"enum vdb_fusion_strategy\s*\{([^}]*)\}", hdr).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"(VDB_FUSION_[A-Z]+)\s*=\s*(\d+)", enum)) == {
        "VDB_FUSION_AVERAGE": 0, "VDB_FUSION_MAXIMUM": 1, "VDB_FUSION_RRF": 2, "VDB_FUSION_WEIGHTED": 3}
    assert re.search(r"#define\s+VDB_KERNEL_FUSE\s+524288\b", hdr)   # (a macro beside enum vdb_kernel_bit: the header says why)
    assert _ffi.VDB_KERNEL_FUSE == va.KERNEL_FUSE == 524288
    assert (_ffi.VDB_FUSION_AVERAGE, _ffi.VDB_FUSION_MAXIMUM, _ffi.VDB_FUSION_RRF, _ffi.VDB_FUSION_WEIGHTED) == (0, 1, 2, 3)
    assert [va.FusionStrategy.Average().code, va.FusionStrategy.Maximum().code, va.FusionStrategy.RRF(5).code,
            va.FusionStrategy.Weighted(0.6, 0.3, 0.1).code] == [0, 1, 2, 3]
    assert os.path.exists(_ffi.LIB_PATH), "run `python -m velesdb_amd.build` first"
    L = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(L, "vdb_hip_fuse_results") and hasattr(L, "vdb_hip_index_multi_query_search")
    lib = _ffi.lib()
    assert lib.vdb_hip_fuse_results.argtypes is not None and len(lib.vdb_hip_fuse_results.argtypes) == 15
    assert len(lib.vdb_hip_index_multi_query_search.argtypes) == 12
    assert "fuse_lists_kernel" in open(os.path.join(ROOT, "velesdb_amd", "csrc", "fusion.hip")).read()
    assert b"fuse_lists_kernel" in open(_ffi.LIB_PATH, "rb").read()


def test_fuse_results_refusals_are_decided_on_the_host():
    """Argument errors and the LDS limit are answered before a device is looked for: the same codes with and without a GPU, the
    outputs untouched."""
    import velesdb_amd as va
    rng = np.random.default_rng(3)

    def call(fusion, groups, top_k=5, sizes=None, null=None):
        ids, sc, ln, gs = fc.pack(groups)
        if sizes is not None:
            gs = np.array(sizes, dtype=np.uint32)
        oi = np.full((len(gs), top_k), 77, dtype=np.uint64)
        os_ = np.full((len(gs), top_k), 77, dtype=np.float32)
        on = np.full(len(gs), 77, dtype=np.uint32)
        code, k, w = fusion
        p = {"w": w.ctypes.data if w is not None else None, "ids": ids.ctypes.data, "sc": sc.ctypes.data, "ln": ln.ctypes.data, "gs": gs.ctypes.data,
             "oi": oi.ctypes.data, "os": os_.ctypes.data, "on": on.ctypes.data}
        if null:
            p[null] = None
        rc = va.lib().vdb_hip_fuse_results(0, code, k, p["w"], p["ids"], p["sc"], p["ln"], ids.shape[0], ids.shape[1], p["gs"], len(gs), top_k,
                                           p["oi"], p["os"], p["on"])
        assert (oi == 77).all() and (os_ == 77).all() and (on == 77).all()
        return rc

    g = fc.adversarial_groups()["one_list"]
    rrf = (2, 60, None)
    assert call(rrf, [g, g], sizes=[1, 2]) == INVALID and "group_sizes" in va._ffi.last_error()
    assert call(rrf, [g, g], sizes=[1]) == INVALID
    for null in ("ids", "sc", "ln", "gs", "oi", "os", "on"):
        assert call(rrf, [g], null=null) == INVALID, null
    assert call((4, 60, None), [g]) == INVALID and call((-1, 60, None), [g]) == INVALID
    assert call((3, 0, None), [g]) == INVALID                                           # WEIGHTED without weights
    for w in ((0.5, 0.3, 0.1), (-0.1, 0.6, 0.5), (float("nan"), 0.5, 0.5), (0.5, 0.3, 0.2011)):
        assert call((3, 0, np.array(w, dtype=np.float32)), [g]) == INVALID, w
    assert call(rrf, [fc.sized_group(8193, rng)]) == UNSUPPORTED and "8192" in va._ffi.last_error()
    assert call(rrf, [g, fc.sized_group(8193, rng), g]) == UNSUPPORTED and "group 1" in va._ffi.last_error()


def test_python_front_raises_with_the_reference_messages():
    import velesdb_amd as va

    class Probe(va.HnswIndex):
        def __init__(self):  # no handle: the argument checks come before the library is called
            self._dimension, self._h = 4, None

        def __del__(self):
            pass

    ix, rrf = Probe(), va.FusionStrategy.rrf_default()
    with pytest.raises(ValueError, match="multi_query_search requires at least one vector"):
        ix.multi_query_search_ids([], 5, rrf)
    with pytest.raises(ValueError, match="multi_query_search supports at most 10 vectors, got 11"):
        ix.multi_query_search_ids(np.zeros((11, 4), np.float32), 5, rrf)
    with pytest.raises(ValueError, match="Vector dimension mismatch: expected 4, got 3"):
        ix.multi_query_search_ids([np.zeros(4, np.float32), np.zeros(3, np.float32)], 5, rrf)
