"""Euclidean batches over the f16 / bf16 image on the matrix cores (VDB_KERNEL_SELECT_HALF_L2): the answer must be the
streaming kernel's — ids, score bits, counts — which the same handle gives with the selector level at 0; on exact data it must be
tests/half_ref.py's sequential reference bit for bit; on N(0,1) data within 1e-5 of the float64 truth, relative to the distance itself
(the rule of tests/test_gpu_half_precision.py::check).  65 613 rows are not a multiple of the 128-row tile, 192 columns are three k-steps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP = va.DistanceMetric, va.VectorPrecision
N = 65536 + 77
PRECS = [hr.F16, hr.BF16]
BOTH = va.KERNEL_SWEEP_HALF_L2 | va.KERNEL_SELECT_HALF_L2


def make_index(rows, prec):
    ix = va.HnswIndex(rows.shape[1], DM.Euclidean, va.HnswParams(16, 100, rows.shape[0]))
    ix.upload(np.arange(rows.shape[0]), rows)
    ix.enable_half_precision(VP.F16 if prec == hr.F16 else VP.BF16)
    return ix


def both_levels(ix, prec, qs, k, search=None, selected=True):
    """The call on the new path and at selector level 0: equal bits, and the kernel mask says which ran."""
    search = search or (lambda: ix.search_batch_brute_force_half(qs, k, VP.F16 if prec == hr.F16 else VP.BF16))
    got, mask = search(), ix.last_kernels()
    ix.set_option(va.OPT_SELECTOR_LEVEL, 0)
    want, mask0 = search(), ix.last_kernels()
    ix.set_option(va.OPT_SELECTOR_LEVEL, -1)
    assert (mask & BOTH) == (BOTH if selected else va.KERNEL_SWEEP_HALF_L2), hex(mask)
    assert bool(mask & va.KERNEL_F16) == (selected and prec == hr.F16) and (mask0 & (BOTH | va.KERNEL_F16)) == va.KERNEL_SWEEP_HALF_L2, (hex(mask), hex(mask0))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    return got


def normal_data(dim, nq, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((N, dim), dtype=np.float32)
    qs = rng.standard_normal((nq, dim), dtype=np.float32)
    spots = rng.choice(N, 9, replace=False)                      # near duplicates of some queries, and one row EQUAL to a query
    rows[spots[:4]] = qs[[0, 5, 11, 15]] + 1e-2 * rng.standard_normal((4, dim), dtype=np.float32)
    rows[spots[4:8]] = qs[[1, 5, 12, 15]] + 1e-3 * rng.standard_normal((4, dim), dtype=np.float32)
    rows[spots[8]] = qs[7]
    return rows, qs


@pytest.fixture(scope="module", params=[(p, d) for p in PRECS for d in (128, 192)], ids=lambda v: "prec%d-dim%d" % v)
def normal(request):
    prec, dim = request.param
    rows, qs = normal_data(dim, 1040, 100 * prec + dim)
    ix = make_index(rows, prec)
    yield prec, rows, qs, ix
    ix.close()


def truth_check(prec, rows, qs, k, got, sample, alive=None):
    """tests/test_gpu_half_precision.py::check for the Euclidean case: 1e-5 relative to the distance itself, tie-aware."""
    eid, esc, kk = hr.scan_topk(hr.EUCLIDEAN, prec, rows, qs[sample], k, alive)
    full = hr.truth64(hr.EUCLIDEAN, prec, rows, qs[sample])[0]
    if alive is not None:
        full = np.where(alive[None, :], full, np.inf)
    for j, qi in enumerate(sample):
        g_i, g_s = got[0][qi, :kk].astype(np.int64), got[1][qi, :kk].astype(np.float64)
        assert got[2][qi] == kk and len(set(g_i.tolist())) == kk
        err = np.abs(g_s - full[j, g_i])
        print("q%d k%d prec %d: max err / distance = %.3e" % (qi, k, prec, float(np.max(err / np.maximum(full[j, g_i], 1e-300)))))
        assert np.all(err <= 1e-5 * full[j, g_i]) and np.all(np.diff(g_s) >= 0)
        assert g_s[-1] <= np.sort(full[j])[kk - 1] * (1 + 1e-5)                                   # nothing nearer was missed
        for r in np.flatnonzero(g_i != eid[j, :kk].astype(np.int64)):                              # tie-aware rank agreement
            assert abs(float(esc[j, r]) - full[j, g_i[r]]) <= 2e-5 * full[j, g_i[r]], (qi, r)


@pytest.mark.parametrize("nq", [16, 17, 130])
def test_bits_of_the_streaming_kernel(normal, nq):
    prec, rows, qs, ix = normal
    for k in (1, 10, 37, 128):
        got = both_levels(ix, prec, qs[:nq], k, selected=nq >= 64 or k <= 10)    # (the measured floor: 64 queries when k > 10)
        truth_check(prec, rows, qs[:nq], k, got, [0, 5, 7, nq - 1])
    assert got[1][7, 0] == 0.0


def test_eligibility_edges_and_two_chunks(normal):
    prec, rows, qs, ix = normal
    both_levels(ix, prec, qs[:15], 10, selected=False)            # below the batch floor
    both_levels(ix, prec, qs, 10)                                  # 1 024 + 16 queries: two chunks
    dim = rows.shape[1]
    for r, q in ((rows[:65535], qs[:16]), (rows[:, :dim - 32], qs[:16, :dim - 32])):   # one row short; dim 96 / 160: no whole 64-column steps
        small = make_index(np.ascontiguousarray(r), prec)
        both_levels(small, prec, np.ascontiguousarray(q), 10, selected=False)
        small.close()


def test_masks(normal):
    prec, rows, qs, ix = normal
    vp = VP.F16 if prec == hr.F16 else VP.BF16
    rng = np.random.default_rng(3)
    for denom in (2, 8, 32):                                       # forced mask substitution; 1/32 leaves the seed too few rows: streaming
        flt = ix.create_filter(np.flatnonzero(rng.integers(0, denom, N) == 0))
        ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_MASK)
        both_levels(ix, prec, qs[:20], 10, lambda: ix.search_batch_filtered_half(qs[:20], 10, flt, vp), selected=denom < 32)
        ix.set_option(va.OPT_FILTER_ROUTE, -1)
        flt.close()
    first = ix.search_batch_brute_force_half(qs[:20], 10, vp)[0]
    dead = sorted(set(first[:, 0].tolist()) | set(first[3].tolist()))
    for d in dead:                                                 # (last: the fixture's handle keeps its dead rows)
        assert ix.remove(int(d))
    alive = np.ones(N, bool)
    alive[dead] = False
    got = both_levels(ix, prec, qs[:20], 10)
    truth_check(prec, rows, qs[:20], 10, got, [0, 3, 7], alive)


@pytest.mark.parametrize("prec", PRECS)
def test_exact_data_ties_by_id(prec):
    """Integer rows drawn from 40 patterns: ~1 640 rows at every distance, ~102 of them inside the 4 096-row seed prefix — rank k falls
    inside a group of equal distances whose rows lie on both sides of the prefix (k = 128 needs ids past it); every sum is exact."""
    rng = np.random.default_rng(40 + prec)
    pool = rng.integers(-3, 4, (40, 128)).astype(np.float32)
    rows = pool[rng.integers(0, 40, N)]
    qs = np.concatenate([pool[:12], rng.integers(-3, 4, (58, 128)).astype(np.float32)])
    ix = make_index(rows, prec)
    for k in (10, 128):
        got = both_levels(ix, prec, qs, k)
        eid, esc, kk = hr.scan_topk(hr.EUCLIDEAN, prec, rows, qs, k)
        assert np.all(got[2] == kk) and np.array_equal(got[0], eid) and np.array_equal(got[1].view(np.uint32), esc.view(np.uint32))
    ix.close()


@pytest.mark.parametrize("prec", PRECS)
def test_fallback_and_special_values(prec):
    rows, qs = normal_data(128, 48, 7 + prec)
    rows[5, 3] = 65520.0                                            # f16: inf
    rows[60000, 0] = np.nan
    qs[4, 9], qs[13, 0] = np.nan, np.inf                            # two marked queries inside an ordinary batch (2 / 48: no hold)
    ix = make_index(rows, prec)
    both_levels(ix, prec, qs, 10)
    for d in range(6, 4096):                                        # six live rows in the seed prefix: every query is marked at k = 10
        assert ix.remove(d)
    both_levels(ix, prec, qs, 10)
    ix.close()


@pytest.mark.parametrize("prec", PRECS)
def test_overflowing_lists_enter_and_leave_the_hold(prec):
    """All rows identical: every list overflows, the whole batch falls back (right bits), and the verdict parks the path for the next
    64 calls (vdb_select_hold.hpp; the counts of tests/test_select_hold_cpu.py's model): call 1 selected, 2 .. 65 streaming, 66 again."""
    rng = np.random.default_rng(prec)
    rows = np.repeat(rng.standard_normal((1, 128), dtype=np.float32), N, axis=0)
    qs = rng.standard_normal((16, 128), dtype=np.float32)
    ix = make_index(rows, prec)
    vp = VP.F16 if prec == hr.F16 else VP.BF16
    ix.set_option(va.OPT_SELECTOR_LEVEL, 0)
    want = ix.search_batch_brute_force_half(qs, 10, vp)
    ix.set_option(va.OPT_SELECTOR_LEVEL, -1)
    assert np.array_equal(want[0], np.tile(np.arange(10, dtype=np.uint64), (16, 1)))
    trace = []
    for _ in range(67):
        got = ix.search_batch_brute_force_half(qs, 10, vp)
        trace.append(bool(ix.last_kernels() & va.KERNEL_SELECT_HALF_L2))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[2], want[2])
    assert trace == [True] + [False] * 64 + [True, False]
    ix.close()
