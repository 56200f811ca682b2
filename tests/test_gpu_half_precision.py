"""GPU parity tests of the half-precision rows: VectorPrecision::{F16, BF16} x {Cosine, DotProduct, Euclidean}
(half_precision.rs:94-101, 199-308) through VDB_SEARCH_BRUTE_F16 / VDB_SEARCH_BRUTE_BF16.

Reference: tests/half_ref.py (the reference's sequential f32 chains in numpy, exact by construction; pinned on the CPU by
tests/test_half_precision_cpu.py).  The bar is the one tests/test_gpu_bf16.py sets for half precision — the matrix instruction's internal
summation order is undocumented — 1e-5: absolute on a cosine, relative to |q||v| on a dot product, RELATIVE TO THE DISTANCE ITSELF for
Euclidean (a near-duplicate row must come out as accurately as a far one: the expanded form |q|^2 + |v|^2 - 2 q.v misses that by two
orders of magnitude); tie-aware ids; and BIT EQUALITY wherever every product and partial sum is exact.  Every case asserts the kernel
bits of the path it claims to drive."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
VP = va.VectorPrecision
METRIC = {hr.COSINE: DM.Cosine, hr.DOT: DM.DotProduct, hr.EUCLIDEAN: DM.Euclidean}
TOL = 1e-5


def served_by(ix, must, must_not=0):
    m = ix.last_kernels()
    assert (m & must) == must and not (m & must_not), "kernel mask %#x, expected %#x without %#x" % (m, must, must_not)


def tier_bits(metric, prec, nq, n, dim, k):
    """The kernel bits brute_bf16_dev's rules give a whole batch of nq queries (one tier per call in every case below)."""
    if metric == hr.EUCLIDEAN:
        return va.KERNEL_SWEEP_HALF_L2
    f16 = va.KERNEL_F16 if prec == hr.F16 else 0
    if nq >= 224 and k <= 10 and dim % 64 == 0 and dim >= 128 and n >= 65536:
        return f16 | va.KERNEL_GEMM_BF16_GLDS
    if nq >= 64 and dim % 64 == 0 and k <= 48:
        return f16 | va.KERNEL_GEMM_BF16
    return f16 | va.KERNEL_SWEEP_MFMA_BF16


def check(metric, prec, rows, qs, k, gids, gsc, gcnt, sample=None, alive=None):
    """The rule of tests/test_gpu_bf16.py::check (for `sample` queries of the batch, or all of them)."""
    sample = np.arange(qs.shape[0]) if sample is None else np.asarray(sample)
    qsel = qs[sample]
    eid, esc, kk = hr.scan_topk(metric, prec, rows, qsel, k, alive)
    full, scale = hr.truth64(metric, prec, rows, qsel)
    if alive is not None:
        full = np.where(alive[None, :], full, np.inf if metric == hr.EUCLIDEAN else -np.inf)
    sign = 1.0 if metric == hr.EUCLIDEAN else -1.0           # ascending in sign * score = best first
    for j, qi in enumerate(sample):
        assert gcnt[qi] == kk
        g_i, g_s = gids[qi, :kk].astype(np.int64), gsc[qi, :kk].astype(np.float64)
        assert len(set(g_i.tolist())) == kk
        err = np.abs(g_s - full[j, g_i])
        print("q%d %s prec %d: max err / scale = %.3e" % (qi, metric, prec, float(np.max(err / np.maximum(scale[j, g_i], 1e-300)))))
        assert np.all(err <= TOL * scale[j, g_i]), (qi, err.max())
        assert np.all(np.diff(sign * g_s) >= -1e-12)           # best first
        kth_true = np.sort(sign * full[j])[kk - 1]
        bound = TOL * (abs(kth_true) if metric == hr.EUCLIDEAN else scale[j][np.isfinite(scale[j])].max())
        assert sign * g_s[-1] <= kth_true + bound, (qi,)      # nothing better was missed
        e_i, e_s = eid[j, :kk].astype(np.int64), esc[j, :kk].astype(np.float64)
        for r in range(kk):                                    # tie-aware rank agreement with the sequential reference
            if g_i[r] != e_i[r]:
                assert abs(e_s[r] - full[j, g_i[r]]) <= 2 * TOL * scale[j, g_i[r]], (qi, r)


def search(ix, qs, k, prec):
    return ix.search_batch_brute_force_half(qs, k, VP.F16 if prec == hr.F16 else VP.BF16)


# ---- conversion, observed through the search -------------------------------------------------------------------------------------
PROBES = np.array([2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14,            # smallest / odd / largest subnormal, smallest normal
                   1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24,                                     # halfway between subnormals: to even (2, 2)
                   1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20,  # ties to even (down, up), just above a tie
                   65504.0, 65519.99, 65520.0, -65520.0, 1e6,                              # largest finite, just below halfway, -> inf
                   0.0, -0.0, 2.0 ** -25, 2.0 ** -26, -(2.0 ** -26), 2.0 ** -25 * 1.0001,  # zeros, underflow to 0 (tie to even), just above -> 2^-24
                   0.1, -0.3333, 1000.7], dtype=np.float32)


@pytest.fixture(scope="module")
def probe_small():
    dim, n = 128, 48            # k = n = 48: the largest k every tier's small-corpus kernel takes
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = np.resize(PROBES, n)
    ix = va.HnswIndex(dim, DM.DotProduct)
    ix.upload(np.arange(n), rows)
    ix.enable_half_precision(VP.F16)
    yield ix, rows
    ix.close()


@pytest.mark.parametrize("nq", [1, 20, 300])
def test_f16_conversion_observed_through_the_search(probe_small, nq):
    """Rows that are zero except for a probe in column 0, query e0, k = n: every score must be np.float16(probe), bit for bit — IEEE
    rounding of the rows (ties to even, overflow to inf, gradual underflow) AND a matrix instruction that keeps f16 subnormal INPUTS —
    on the streaming kernel (1, 20 queries) and the register-staged GEMM kernel (300)."""
    ix, rows = probe_small
    n, dim = rows.shape
    qs = np.zeros((nq, dim), np.float32)
    qs[:, 0] = 1.0
    gi, gs, gc = search(ix, qs, n, hr.F16)
    served_by(ix, va.KERNEL_F16 | (va.KERNEL_SWEEP_MFMA_BF16 if nq < 64 else va.KERNEL_GEMM_BF16))
    with np.errstate(over="ignore"):
        want = rows[:, 0].astype(np.float16).astype(np.float32)
    want[want == 0] = 0.0                                        # (+0 + -0 = +0 in every summation order)
    assert np.array_equal(hr.scores(hr.DOT, hr.F16, rows, qs[:1])[0].view(np.uint32), want.view(np.uint32))
    assert np.all(gc == n)
    for qi in (0, nq // 2, nq - 1):
        got = np.empty(n, np.float32)
        got[gi[qi].astype(np.int64)] = gs[qi]
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, [(float(rows[b, 0]), float(got[b]), float(want[b])) for b in bad[:8]]
        assert np.array_equal(gi[qi], hr.topk(want[None, :], n, True)[0][0])     # best first, equal scores by row


def test_f16_conversion_on_the_big_tier():
    """>= 65 536 rows x >= 224 queries: sweep_topk_gemm_f16_pp.  The probes up to the smallest normal (subnormals, subnormal ties,
    values that underflow to zero) are the only rows with a score >= 0 — every other row scores -1 through column 1 — so the top-10
    of every query IS the probe set, scaled by the query's power of two (exact)."""
    dim, n, nq, k = 128, 70_000, 256, 10
    rng = np.random.default_rng(4)
    tiny = PROBES[(np.abs(PROBES) <= 2.0 ** -14) & ~np.signbit(PROBES)]
    assert tiny.size == 10
    rows = np.zeros((n, dim), np.float32)
    rows[:, 1] = -1.0
    where = np.sort(rng.choice(n, tiny.size, replace=False))
    rows[where, 0] = tiny
    rows[where, 1] = 0.0
    qs = np.zeros((nq, dim), np.float32)
    qs[:, 0] = 2.0 ** (np.arange(nq) % 8)
    qs[:, 1] = 1.0
    ix = va.HnswIndex(dim, DM.DotProduct, va.HnswParams(16, 100, n))
    ix.upload(np.arange(n), rows)
    ix.enable_half_precision(VP.F16)
    gi, gs, gc = search(ix, qs, k, hr.F16)
    served_by(ix, va.KERNEL_F16 | va.KERNEL_GEMM_BF16_GLDS)
    eid, esc, _ = hr.scan_topk(hr.DOT, hr.F16, rows, qs[:8], k)
    assert np.all(esc >= 0) and np.count_nonzero(esc[0]) == 7 and esc[0].max() == np.float32(2.0 ** -14)
    for qi in range(nq):
        assert np.array_equal(gi[qi], eid[qi % 8]) and np.array_equal(gs[qi].view(np.uint32), esc[qi % 8].view(np.uint32)), (qi, gs[qi], esc[qi % 8])
    ix.close()


# ---- tolerance parity on N(0,1) data ----------------------------------------------------------------------------------------------
PARITY = [(hr.F16, hr.COSINE), (hr.F16, hr.DOT), (hr.F16, hr.EUCLIDEAN), (hr.BF16, hr.EUCLIDEAN)]


@pytest.mark.parametrize("prec,metric", PARITY)
@pytest.mark.parametrize("n,dim", [(6000, 768), (3000, 256), (2000, 100), (500, 40), (40, 8)])
def test_half_precision_parity(prec, metric, n, dim):
    rng = np.random.default_rng(n + dim + 17 * prec + metric)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    batches = [(1, 10), (20, 10), (70, 5), (100, 10), (129, 5), (300, 10), (3, 64), (64, 1)]
    qsets = [rng.standard_normal((nq, dim)).astype(np.float32) for nq, _ in batches]
    if metric == hr.EUCLIDEAN:      # near duplicates of four queries (1e-2 noise) and one row EQUAL to a query (distance exactly 0)
        q = qsets[5]
        spots = rng.choice(n, 5, replace=False)
        rows[spots[:4]] = q[[0, 7, 150, 299]] + 1e-2 * rng.standard_normal((4, dim)).astype(np.float32)
        rows[spots[4]] = q[33]
    ix = va.HnswIndex(dim, METRIC[metric])
    ix.upload(np.arange(n // 2), rows[: n // 2])
    ix.enable_half_precision(VP.F16 if prec == hr.F16 else VP.BF16)        # converts what is there ...
    ix.upload(np.arange(n // 2, n), rows[n // 2:])                          # ... and what arrives later
    for (nq, k), qs in zip(batches, qsets):
        gi, gs, gc = search(ix, qs, k, prec)
        served_by(ix, tier_bits(metric, prec, nq, n, dim, k))
        check(metric, prec, rows, qs, k, gi, gs, gc)
        if metric == hr.EUCLIDEAN and nq == 300:
            assert gs[33, 0] == 0.0 and gi[33, 0] == spots[4]
            for j, qi in enumerate([0, 7, 150, 299]):
                assert gi[qi, 0] == spots[j]
    ix.close()


# ---- exact data: bit equality with the sequential reference, ties by row ----------------------------------------------------------
def grid_f16(rng, shape):
    """Exact in f16 and NOT in bf16: odd multiples of 1/256 in +-[257/256, 511/256] (tests/test_half_precision_cpu.py checks the claim)."""
    return ((2 * rng.integers(128, 256, shape) + 1) / 256.0 * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def assert_bits(ix, metric, prec, rows, qs, k, alive=None):
    gi, gs, gc = search(ix, qs, k, prec)
    eid, esc, kk = hr.scan_topk(metric, prec, rows, qs, k, alive)
    assert np.all(gc == kk)
    assert np.array_equal(gi[:, :kk], eid[:, :kk])
    assert np.array_equal(gs[:, :kk].view(np.uint32), esc[:, :kk].view(np.uint32))
    return gi


# (bf16 rows through the new entry point on integers only: the 1/256 grid is not representable in bf16)
@pytest.mark.parametrize("prec,metric,data", [(p, m, d) for d in ("ints", "grid") for p, m in PARITY if not (d == "grid" and p == hr.BF16)] + [(hr.BF16, hr.COSINE, "ints")])
def test_exact_data_bit_equal_small_tiers(prec, metric, data):
    dim, n = (64, 3000) if data == "grid" else (128, 5000)
    rng = np.random.default_rng(100 * prec + 10 * metric + len(data))
    make = grid_f16 if data == "grid" else ints
    rows = make(rng, (n, dim))
    rows[[5, 2999]] = 0.0
    if metric != hr.EUCLIDEAN:                      # (a difference against 2^-24 is no longer an exact square)
        rows[[9, 1003], :] = 0.0
        rows[[9, 1003], 3] = 2.0 ** -24             # norm 6e-8 < f32::EPSILON: cosine 0.0 by the reference's rule; an f16 subnormal
    rows[[256, 257, 2000]] = rows[[1, 1, 1]]        # duplicates: exact ties, by row
    ix = va.HnswIndex(dim, METRIC[metric])
    ix.upload(np.arange(n), rows)
    ix.enable_half_precision(VP.F16 if prec == hr.F16 else VP.BF16)
    for nq in (3, 70, 300):
        qs = make(rng, (nq, dim))
        qs[nq // 2] = 0.0                           # a zero query: every cosine 0, ties by row
        qs[0] = rows[1]
        gi = assert_bits(ix, metric, prec, rows, qs, 10)
        served_by(ix, tier_bits(metric, prec, nq, n, dim, 10))
    dead = sorted({int(gi[0, 0]), int(gi[1, 0]), 256})
    for d in dead:
        assert ix.remove(d)
    alive = np.ones(n, bool)
    alive[dead] = False
    for nq in (3, 70, 300):
        assert_bits(ix, metric, prec, rows, make(rng, (nq, dim)), 10, alive)
    ix.close()


@pytest.mark.parametrize("metric", [hr.DOT, hr.COSINE])
def test_f16_big_tier_exact_products_bit_equal(metric):
    # as test_bf16_glds_exact_products_bit_equal, on values bf16 cannot hold: a kernel that read the bf16 image, or fragments in the
    # wrong lanes (the data is asymmetric), cannot pass
    # The big tier needs dim >= 128, and 128 grid values are too many to stay exact (squares of odd m / 256, m <= 511, sum to 2^25
    # units of 2^-16): the grid fills 64 columns — an irregular set, the same for rows and queries — and the other 64 are zero, so
    # every norm and dot product is the 64-term sum whose exactness tests/test_half_precision_cpu.py checks (asserted again below).
    dim, n, nq, k = 128, 70_077, 300, 10
    rng = np.random.default_rng(n + metric)
    cols = np.sort(rng.choice(dim, 64, replace=False))
    rows, qs = np.zeros((n, dim), np.float32), np.zeros((nq, dim), np.float32)
    rows[:, cols] = grid_f16(rng, (n, 64))
    qs[:, cols] = grid_f16(rng, (nq, 64))
    units = np.rint(rows.astype(np.float64) * 256.0)                     # integers m: a row's squares sum to sum(m^2) / 65536
    assert np.array_equal(units / 256.0, rows) and (units ** 2).sum(1).max() <= 2.0 ** 24
    assert (np.abs(units) @ np.abs(np.rint(qs.astype(np.float64) * 256.0)).T[:, :8]).max() <= 2.0 ** 24   # (sampled: every |partial sum| <= this)
    best = np.argsort(-(qs[:8] @ rows.T), axis=1)[:, :2].ravel()
    spots = np.array([255, 256, 257, 16383, 16384, 16385, 65535, 65536, 70_000, n - 2, n - 1, n // 2, n // 2 + 255, 300, 4000, 9999])
    rows[spots] = rows[best]                                            # good rows duplicated across tile / launch boundaries
    rows[[5, 20_000, n - 3]] = 0.0
    rows[[9, 40_003]] = 0.0
    rows[[9, 40_003], 7] = 2.0 ** -24                                   # norm below f32::EPSILON
    qs[3] = 0.0
    ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(16, 100, n))
    ix.upload(np.arange(n), rows)
    ix.enable_half_precision(VP.F16)
    ix.enable_half_precision(VP.BF16)                                   # both images on one handle: each its own answers
    gi = assert_bits(ix, metric, hr.F16, rows, qs, k)
    served_by(ix, va.KERNEL_F16 | va.KERNEL_GEMM_BF16_GLDS)
    bi, bs, _ = search(ix, qs, k, hr.BF16)
    served_by(ix, va.KERNEL_GEMM_BF16_GLDS, va.KERNEL_F16)
    eid, esc, _ = hr.scan_topk(metric, hr.BF16, rows, qs[:4], k)
    full, scale = hr.truth64(metric, hr.BF16, rows, qs[:4])
    for qi in range(4):
        assert np.all(np.abs(bs[qi].astype(np.float64) - full[qi, bi[qi].astype(np.int64)]) <= TOL * scale[qi, bi[qi].astype(np.int64)])
    assert not np.array_equal(bi, gi)                                   # the bf16 image gives another top-10
    dead = sorted({int(gi[0, 0]), int(gi[17, 0]), int(spots[1]), int(gi[299, 9])})
    for d in dead:
        assert ix.remove(d)
    alive = np.ones(n, bool)
    alive[dead] = False
    assert_bits(ix, metric, hr.F16, rows, qs, k, alive)
    served_by(ix, va.KERNEL_F16 | va.KERNEL_GEMM_BF16_GLDS)
    ix.close()


# ---- the big tier on N(0,1) data ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,dim,cases", [
    (hr.COSINE, 70_000, 768, [(230, 10), (1024, 1)]),
    (hr.DOT, 70_000, 768, [(600, 1), (1024, 10)]),
    (hr.COSINE, 300_001, 128, [(600, 10), (1024, 1)]),
    (hr.DOT, 300_001, 128, [(230, 1), (1024, 10)]),
])
def test_f16_big_tier(metric, n, dim, cases):
    rng = np.random.default_rng(n * 13 + dim + metric)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(16, 100, n))
    ix.upload(np.arange(n), rows)
    ix.enable_half_precision(VP.F16)
    for nq, k in cases:
        qs = rng.standard_normal((nq, dim), dtype=np.float32)
        gi, gs, gc = search(ix, qs, k, hr.F16)
        served_by(ix, va.KERNEL_F16 | va.KERNEL_GEMM_BF16_GLDS)
        sample = np.unique(np.concatenate([[0, nq - 1, 255 % nq, 256 % nq], rng.integers(0, nq, 20)]))
        check(metric, hr.F16, rows, qs, k, gi, gs, gc, sample)
    ix.close()


# ---- state and errors -----------------------------------------------------------------------------------------------------------------
def test_half_precision_state_and_errors(tmp_path):
    dim, n = 64, 900
    rng = np.random.default_rng(9)
    rows = grid_f16(rng, (n, dim))
    qs = grid_f16(rng, (5, dim))
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(16, 100, 64))     # small capacity: the uploads below grow the images
    ix.upload(np.arange(300), rows[:300])
    with pytest.raises(va.VelesHipError) as e:
        search(ix, qs, 3, hr.F16)                                        # mode 7 before enable
    assert e.value.code == -8
    with pytest.raises(va.VelesHipError) as e:
        search(ix, qs, 3, hr.BF16)
    assert e.value.code == -8
    with pytest.raises(va.VelesHipError) as e:
        ix.enable_half_precision(VP.F32)
    assert e.value.code == -7
    with pytest.raises(va.VelesHipError):
        ix.enable_bf16()                                                 # still refuses a Euclidean handle
    ix.enable_half_precision(VP.F16)
    ix.enable_half_precision(VP.BF16)
    ix.enable_half_precision(VP.F16)                                     # idempotent
    ix.upload(np.arange(300, n), rows[300:])                             # grow
    assert_bits(ix, hr.EUCLIDEAN, hr.F16, rows, qs, 10)
    served_by(ix, va.KERNEL_SWEEP_HALF_L2, va.KERNEL_F16)
    gb, sb, cb = search(ix, qs, 10, hr.BF16)                             # its own image: another answer, right by ITS reference
    served_by(ix, va.KERNEL_SWEEP_HALF_L2, va.KERNEL_F16)
    check(hr.EUCLIDEAN, hr.BF16, rows, qs, 10, gb, sb, cb)
    gi = assert_bits(ix, hr.EUCLIDEAN, hr.F16, rows, qs, 10)
    assert not np.array_equal(sb, hr.scan_topk(hr.EUCLIDEAN, hr.F16, rows, qs, 10)[1])
    assert ix.remove(int(gi[0, 0]))
    alive = np.ones(n, bool)
    alive[int(gi[0, 0])] = False
    assert_bits(ix, hr.EUCLIDEAN, hr.F16, rows, qs, 10, alive)
    # save / load of the index directory, then enable: the half copies are derived images, rebuilt from the loaded rows
    ix2 = va.HnswIndex(dim, DM.Cosine)
    ix2.insert_batch_parallel([(i, rows[i]) for i in range(200)])
    ix2.enable_half_precision(VP.F16)
    before = search(ix2, qs, 10, hr.F16)
    d = str(tmp_path / "idx")
    ix2.save(d)
    ix3 = va.HnswIndex.load(d)
    with pytest.raises(va.VelesHipError):
        search(ix3, qs, 10, hr.F16)
    ix3.enable_half_precision(VP.F16)
    after = search(ix3, qs, 10, hr.F16)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    for h in (ix, ix2, ix3):
        h.close()
    for m in (DM.Hamming, DM.Jaccard):
        hx = va.HnswIndex(32, m)
        with pytest.raises(va.VelesHipError) as e:
            hx.enable_half_precision(VP.F16)
        assert e.value.code == -7
        hx.close()


def test_device_resident_entry_point_and_single_query_front():
    # vdb_hip_index_search (the combining front), the _dev variant and rows that arrive through upload_dev serve mode 7 like mode 3
    import ctypes as C
    torch = pytest.importorskip("torch")
    dim, n = 64, 2000
    rng = np.random.default_rng(12)
    rows, qs = grid_f16(rng, (n, dim)), grid_f16(rng, (7, dim))
    for metric in (hr.DOT, hr.EUCLIDEAN):
        ix = va.HnswIndex(dim, METRIC[metric])
        ix.upload(np.arange(n // 2), rows[: n // 2])
        ix.enable_half_precision(VP.F16)
        drows = torch.from_numpy(rows[n // 2:]).cuda()
        torch.cuda.synchronize()
        ix.upload_dev(n // 2, drows.data_ptr(), n - n // 2)
        eid, esc, _ = hr.scan_topk(metric, hr.F16, rows, qs, 10)
        ids, sc, cnt = np.zeros(10, np.uint64), np.zeros(10, np.float32), C.c_uint32(0)
        va._ffi.check(va.lib().vdb_hip_index_search(ix._h, qs[0].ctypes.data_as(C.c_void_p), dim, 10, 0, va.MODE_BRUTE_F16,
                                                    ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(cnt)))
        assert cnt.value == 10 and np.array_equal(ids, eid[0]) and np.array_equal(sc.view(np.uint32), esc[0].view(np.uint32))
        dq = torch.from_numpy(qs).cuda()
        d_ids = torch.zeros((7, 10), dtype=torch.int64, device="cuda")
        d_sc = torch.zeros((7, 10), dtype=torch.float32, device="cuda")
        d_n = torch.zeros(7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ix.search_batch_dev(dq.data_ptr(), 7, 10, 0, va.MODE_BRUTE_F16, d_ids.data_ptr(), d_sc.data_ptr(), d_n.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_ids.cpu().numpy().astype(np.uint64), eid)
        assert np.array_equal(d_sc.cpu().numpy().view(np.uint32), esc.view(np.uint32))
        assert np.all(d_n.cpu().numpy() == 10)
        ix.close()
