"""CPU tier of the hybrid search: no GPU needed.

  * tests/hybrid_ref.py — the numpy-float32 restatement of Collection::hybrid_search / hybrid_search_with_filter — puts the leader
    the reference's own three tests assert first (tests/golden/hybrid_kats.json: id lists and leaders as data);
  * the PRODUCT's rule — csrc/vdb_hybrid.hpp, the text hybrid_fuse_kernel is written over, compiled for the host by
    tests/hybrid_model.cpp — equals the restatement bit for bit on the adversarial queries and on 3 000 random ones;
  * the weight clamp in f32, the NaN refusal and the record limit, decided by the host before a launch;
  * the header, the built library and the ctypes binding carry the two entry points and VDB_KERNEL_HYBRID_FUSE.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import hybrid_cases as hc
import hybrid_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "hybrid_kats.json")))
INVALID, UNSUPPORTED = -1, -7


@pytest.fixture(scope="module")
def model():
    return hc.hybrid_model()


def _same(model, c, k):
    want = hr.top(hc.reference(c, k), k)
    rc, ids, sb, n = hc.model_fuse(model, c, k)
    assert rc == 0
    assert n == want[2], (c, k, n, want[2])
    assert np.array_equal(ids, want[0]), (c, k, ids, want[0])
    assert np.array_equal(sb, want[1]), (c, k, sb, want[1])
    return want


@pytest.mark.parametrize("kat", KATS["cases"], ids=lambda c: c["name"])
def test_restatement_and_model_satisfy_the_reference_kats(model, kat):
    for text in kat["text_orders"]:
        c = hc.case(kat["vector"], text, kat["vector_weight"])
        got = hr.hybrid(c["V"], c["T"], kat["k"], c["w"])
        assert got and got[0][0] == kat["leader"], (kat["name"], text, got)
        assert len({i for i, _ in got}) == len(got)
        ids, _, n = _same(model, c, kat["k"])
        assert n and int(ids[0]) == kat["leader"]


@pytest.mark.parametrize("name", sorted(hc.adversarial_cases()))
def test_model_equals_restatement_on_adversarial_queries(model, name):
    c = hc.adversarial_cases()[name]
    for k in hc.cut_points(c):
        _same(model, c, k)
    _same(model, dict(c, dead=set(), allowed=None), 4 * hc.distinct(c) + 1)     # the same lists as vdb_hip_hybrid_fuse sees them


def test_the_stated_tie_order_and_cut(model):
    adv = hc.adversarial_cases()
    # every id of the reversed pair ties with its mirror image: the larger id first, and the larger id survives a cut between them
    ids, sb, n = _same(model, adv["reversed_every_id_ties_pairwise"], 6)
    assert list(ids[:6]) == [9, 2, 8, 3, 7, 1] and sb[0] == sb[1] and sb[2] == sb[3] and sb[4] == sb[5] and sb[1] > sb[2]
    ids, sb, n = _same(model, adv["reversed_every_id_ties_pairwise"], 3)
    assert list(ids[:3]) == [9, 2, 8] and n == 3
    # w = 1: the text weight is 0, every text-only id ties at +0.0 behind the vector list; w = 0 the other way round
    ids, sb, n = _same(model, adv["weight_1.0"], 10)
    assert list(ids[:n]) == [11, 4, 8, 15, 16, 42, 23] and sb[5] == sb[6] == 0
    ids, sb, n = _same(model, adv["weight_0.0"], 10)
    # every occurrence adds: 4 sits at text ranks 4 and 5, and 1/64 + 1/65 beats the text leader's 1/60
    assert list(ids[:n]) == [4, 23, 8, 42, 11, 16, 15] and sb[5] == sb[6] == 0
    want = F(F(0.0) + F(F(1.0) / F(64.0))) + F(F(1.0) / F(65.0))
    assert sb[0] == hr.bits(F(want))
    # ids that differ in one 32-bit half only are different ids
    ids, sb, n = _same(model, adv["ids_differ_in_one_half"], 20)
    assert n == 8
    # non-live text ids take their place in the cut and are then dropped: fewer than min(k, distinct ids) come back
    c = adv["non_live_text_ids_around_the_cut"]
    for k, expect in ((3, [100]), (4, [100]), (5, [100, 104]), (6, [100, 104, 1]), (8, [100, 104, 1, 2, 3])):
        ids, sb, n = _same(model, c, k)
        assert list(ids[:n]) == expect, (k, ids)
    # the filtered form drops before ranks exist: 2 and 3 move up to text ranks 0 and 1, 102 to rank 2
    c = adv["filter_keeps_some_text_hits"]
    assert [i for i, _ in hc.reference(c, 10)] == [i for i, _ in hr.hybrid([1, 2, 3], [2, 3, 102, 2], 10, 0.4)]
    ids, sb, n = _same(model, adv["filter_rejects_every_text_hit"], 10)
    assert list(ids[:n]) == [1, 2, 3]
    assert _same(model, adv["filter_rejects_everything"], 5)[2] == 0


def test_model_equals_restatement_on_random_queries(model):
    rng = np.random.default_rng(20261)
    for t in range(3000):
        c = hc.random_case(rng)
        _same(model, c, int(rng.choice([0, 1, 3, 10, 40])))


def test_weights_are_clamped_in_f32_and_nan_is_refused(model):
    out = np.zeros(1, dtype=np.uint32)
    assert model.hybrid_model_default_weight_bits() == hr.bits(F(0.5)) == hr.bits(hr.clamp_weight(None))
    for w, want in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.3, F(0.3)), (-2.0, 0.0), (7.0, 1.0), (float("inf"), 1.0), (float("-inf"), 0.0),
                    (np.nextafter(F(1.0), F(0.0)), np.nextafter(F(1.0), F(0.0))), (np.nextafter(F(1.0), F(2.0)), 1.0), (1e-45, F(1e-45)), (-1e-45, 0.0)):
        assert model.hybrid_model_clamp(w, out.ctypes.data) == 1
        assert int(out[0]) == hr.bits(F(want)) == hr.bits(hr.clamp_weight(w)), w
    # tw = 1.0f - w is an f32 subtraction of the clamped f32 weight
    c = hc.adversarial_cases()["weight_0.3"]
    assert hr.bits(hr.hybrid([], [5], 1, 0.3)[0][1]) == hr.bits(F(F(0.0) + F(F(F(1.0) - F(0.3)) / F(60.0))))
    assert model.hybrid_model_clamp(float("nan"), out.ctypes.data) == 0
    assert hc.model_fuse(model, c, 3, raw_weight=float("nan"))[0] == INVALID
    with pytest.raises(ValueError):
        hr.clamp_weight(float("nan"))


def test_header_library_and_binding_carry_the_feature():
    from velesdb_amd import _ffi
    import velesdb_amd as va
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "velesdb_hip.h")).read(), flags=re.S)
    for name in ("vdb_hip_hybrid_fuse", "vdb_hip_index_hybrid_search"):
        assert re.search(r"int32_t\s+" + name + r"\s*\(", hdr), name
        assert name in _ffi.SIGNATURES
    assert re.search(r"#define\s+VDB_KERNEL_HYBRID_FUSE\s+4194304\b", hdr)   # (a macro beside enum vdb_kernel_bit, as VDB_KERNEL_FUSE)
    assert _ffi.VDB_KERNEL_HYBRID_FUSE == va.KERNEL_HYBRID_FUSE == 4194304
    assert va.HYBRID_MAX_RECORDS == hr.MAX_RECORDS == 8192
    assert os.path.exists(_ffi.LIB_PATH), "run `python -m velesdb_amd.build` first"
    L = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(L, "vdb_hip_hybrid_fuse") and hasattr(L, "vdb_hip_index_hybrid_search")
    lib = _ffi.lib()
    assert len(lib.vdb_hip_hybrid_fuse.argtypes) == 13 and len(lib.vdb_hip_index_hybrid_search.argtypes) == 12
    assert "hybrid_fuse_kernel" in open(os.path.join(ROOT, "velesdb_amd", "csrc", "hybrid.hip")).read()
    assert b"hybrid_fuse_kernel" in open(_ffi.LIB_PATH, "rb").read()
    for name in ("hybrid_fuse_arrays", "KERNEL_HYBRID_FUSE", "HYBRID_MAX_RECORDS"):
        assert hasattr(va, name), name
    for name in ("hybrid_search_batch", "hybrid_search", "hybrid_search_with_filter"):
        assert callable(getattr(va.HnswIndex, name)), name


def test_hybrid_fuse_refusals_are_decided_on_the_host(model):
    """Argument errors, a NaN weight and the LDS limit are answered by the host plan before a device is looked for: the same codes
    with and without a GPU, the outputs untouched."""
    import velesdb_amd as va
    rng = np.random.default_rng(5)
    assert model.hybrid_model_max_records() == 8192

    def call(cases, k=5, null=None, weights="own", text_n=None):
        vi, vn, ti, tn, w = hc.pack(cases)
        if text_n is not None:
            tn = np.array(text_n, dtype=np.uint32)
        if isinstance(weights, np.ndarray):
            w = weights
        oi = np.full((len(cases), k), 77, dtype=np.uint64)
        os_ = np.full((len(cases), k), 77, dtype=np.float32)
        on = np.full(len(cases), 77, dtype=np.uint32)
        p = {"vi": vi.ctypes.data, "vn": vn.ctypes.data, "ti": ti.ctypes.data, "tn": tn.ctypes.data, "w": None if weights is None else w.ctypes.data,
             "oi": oi.ctypes.data, "os": os_.ctypes.data, "on": on.ctypes.data}
        if null:
            p[null] = None
        rc = va.lib().vdb_hip_hybrid_fuse(0, p["vi"], p["vn"], vi.shape[1], p["ti"], p["tn"], ti.shape[1], p["w"], len(cases), k, p["oi"], p["os"],
                                          p["on"])
        assert (oi == 77).all() and (os_ == 77).all() and (on == 77).all()
        return rc

    c = hc.adversarial_cases()["lists_equal"]
    for null in ("vi", "vn", "ti", "tn", "oi", "os", "on"):
        assert call([c], null=null) == INVALID, null
    assert call([c, c], weights=np.array([0.5, float("nan")], np.float32)) == INVALID and "query 1" in va._ffi.last_error()
    assert call([c, c], text_n=[4, 5]) == INVALID and "query 1" in va._ffi.last_error()
    big = hc.sized_case(8193, rng)
    assert call([big]) == UNSUPPORTED and "8192" in va._ffi.last_error()
    assert call([c, big, c], weights=None) == UNSUPPORTED and "query 1" in va._ffi.last_error()
    with pytest.raises(va.VelesHipError) as e:
        va.hybrid_fuse_arrays(*hc.pack([c, big])[:4], 5)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(va.VelesHipError) as e:
        va.hybrid_fuse_arrays(*hc.pack([c])[:4], 5, vector_weights=float("nan"))
    assert e.value.code == INVALID
    # the index entry point refuses its arguments before it looks at the handle's state: no handle at all is INVALID
    assert va.lib().vdb_hip_index_hybrid_search(None, None, None, 0, 5, None, None, 0, None, None, None, None) == INVALID
    # the host model refuses the same record count
    assert hc.model_fuse(model, big, 5)[0] == UNSUPPORTED


def test_python_front_checks_its_arguments():
    import velesdb_amd as va

    class Probe(va.HnswIndex):
        def __init__(self):  # no handle: the argument checks come before the library is called
            self._dimension, self._h = 4, None

        def __del__(self):
            pass

    ix = Probe()
    with pytest.raises(ValueError, match=r"Queries count \(2\) does not match id lists count \(1\)"):
        ix.hybrid_search_batch(np.zeros((2, 4), np.float32), [[1, 2]], 5)
    with pytest.raises(ValueError, match=r"Queries count \(2\) does not match vector_weight count \(3\)"):
        ix.hybrid_search_batch(np.zeros((2, 4), np.float32), [[1], [2]], 5, vector_weight=[0.5, 0.5, 0.5])
    with pytest.raises(AssertionError, match="dimension mismatch"):
        ix.hybrid_search(np.zeros(3, np.float32), [1], 5)
