"""GPU parity tests, above dim 1 024, of the features merged after tests/test_gpu_large_dim_features.py: per-query filters on the
f32 exact sweep, the listed sweeps over the SQ8 codes and the half images (one filter and one filter per query), mask substitution
in Binary and half Cosine / DotProduct, and the half walk with the exact f32 re-score.  These are the dims where every LDS budget
that depends on dim changes the plan:

  A  per-query filters on the f32 exact sweep: mode C with the query in LDS at the class the 60 KiB window forces (B 8 -> 4 -> 1),
     mode M with the pass the 160 KiB budget halves (16 -> 8);
  B  SQ8, one filter and per query: the > 64 KiB dynamic-LDS opt-in of every listed instance, the class fall-back 8 -> 4 -> 1 of
     mode_listed_plan, query addresses past 64 KiB, 64 staging chunks and a partial last one;
  C  half images: Euclidean over f16 / bf16 (16 -> 4 -> 1, the 163 712-byte exact fit), Cosine / DotProduct and Binary under a mask;
  D  the half walk with the f32 re-score on generic dims (the LDS query scratch rewritten with the unrounded query).

Nothing here is a new reference or a new tolerance: the oracle (oracle.pyoracle) and the helpers of each feature's own tests,
imported.  Everything is bit equality of ids, counts, score bits and padding, except half Cosine / DotProduct on N(0,1) rows (TOL of
tests/test_gpu_half_precision.py, unchanged).  Every test asserts which kernel or route served it, and the pass class the plan took
against the tables of literals below: each carries the byte counts that force it, so a change of a footprint formula fails a test
instead of silently moving the edge.  Where each class is bound to the product:

  * SQ8 and half Euclidean: tests/test_large_dim_filters_modes_shapes_cpu.py holds the tables to mode_listed_plan of
    velesdb_amd/csrc/vdb_filter_route.hpp itself, compiled stand-alone.  On the device the per-query calls show the class through the
    launch count of last_filters_exact_plan (3 / 2 / 1 launches); for the ONE-FILTER calls nothing on the device shows the class —
    it is asserted in the CPU tier (and against the restated fms.passes_of), the device shows the kernel bit and the answer.
  * f32 mode C: sweep_listed_plan cannot be compiled on the host; the tables are held to the restatement below, and the launch count of
    the forced listed route (3 / 2 / 1 by class) binds that to the product on the device.
  * f32 mode M is the exception: a mode-M call is always one launch and no diagnostic exposes its pass width, so the widths (16, 8,
    17 = 8 + 9) are asserted against the restatement m_lds / m_passes ONLY.  A change of listed_m_lds_bytes or of the halving loop in
    csrc/sweep_listed.hip fails no test here unless it also changes an answer or makes a launch fail.

Left out: the f16 grid data (hp.grid_f16) for Euclidean.  Its squared differences reach 1022^2 units of 2^-16; the argument of
tests/test_gpu_filtered_modes.py keeps their sum below 2^24 at dim 17 only — at dim 1 536 the typical sum is above 2^28."""
import numpy as np
import pytest

import filtered_half_rescore_ref as fr
import filtered_walk_ref as fw
import half_ref as hr
import half_walk_ref as hw
import hybrid_cases as hc
import hybrid_ref as hyr
import test_gpu_filtered as tf
import test_gpu_filtered_modes as fm
import test_gpu_filters_exact as fx
import test_gpu_filters_graph_half_rescore as gr
import test_gpu_filters_modes as fms
import test_gpu_half_precision as hp
import test_gpu_large_dim_features as ldf
from oracle import pyoracle as po
from test_gpu_storage_modes import special_rows

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, SM = va.DistanceMetric, va.StorageMode
LISTED, MASK, AUTO = va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK, va.FILTER_ROUTE_AUTO
ROUTES = {"auto": AUTO, "listed": LISTED, "mask": MASK}
UNSUPPORTED = va._ffi.VDB_ERR_UNSUPPORTED
FLOATS = [DM.Cosine, DM.DotProduct, DM.Euclidean]

# ================================================================================================ the tables of literals
# f32 grouped sweep, mode C, the query in LDS (CPL 0), window 61 440 B: (dim, k) -> (bytes at B 8, at B 4, at B 1, class taken).
# Footprint: B * ceil(dim / 4) * 16 for the queries + B * k * 8 + B * 8 for the lists, each rounded to 16.
C_WINDOW = 61440
C_TABLE = {
    (1536, 10): (49856, 24928, 6240, 8),      # the one (dim, k) of this file where eight queries fit
    (1536, 200): (62016, 31008, 7760, 4),     # 62 016 > 61 440: the k-lists alone push B 8 out
    (2047, 10): (66240, 33120, 8288, 4),      # eight queries are 65 536 B before any list
    (2047, 200): (78400, 39200, 9808, 4),
    (2048, 10): (66240, 33120, 8288, 4),      # (2 048 = 8 x 256: above the register-chunk instances, CPL 0 again)
    (2048, 200): (78400, 39200, 9808, 4),
    (2432, 10): (78528, 39264, 9824, 4),
    (2432, 200): (90688, 45344, 11344, 4),
    (4096, 10): (131776, 65888, 16480, 1),    # four queries are 65 536 B before any list
    (4096, 200): (143936, 71968, 18000, 1),
    (4095, 10): (131776, 65888, 16480, 1),    # (ceil(4 095 / 4) = 1 024: the footprint of 4 096, the predicated tail in the body)
    (4095, 200): (143936, 71968, 18000, 1),
}
# f32 grouped sweep, mode M, budget 163 840 B: (dim, k) -> (bytes at 16 queries, at 9, at 8, the widest pass).  Footprint: nq *
# dim_pad * 4 (dim_pad = dim rounded up to 128) + 34 816 for the row stage + nq * k * 8 + 448.  sweep_listed_plan halves the pass
# of a group of 16 or more (16 -> 8) where 16 queries do not fit; what is LEFT of a group is held to the budget on its own, so a
# group of 17 runs as 8 + 9 there (nine queries fit), not 8 + 8 + 1 — launch_groups_m sizes the launch's LDS by its widest pass.
M_BUDGET = 160 * 1024
M_TABLE = {
    (1536, 10): (134848, 91280, 85056, 16),
    (1536, 200): (159168, 104960, 97216, 16),
    (2047, 10): (167616, 109712, 101440, 8),  # 167 616 > 163 840 (dim_pad 2 048)
    (2047, 200): (191936, 123392, 113600, 8),
    (2048, 10): (167616, 109712, 101440, 8),
    (2048, 200): (191936, 123392, 113600, 8),
    (2432, 10): (192192, 123536, 113728, 8),  # (k = 200 at dim 2 432 answers in mode C: ldf.expected_mode)
}
# SQ8 listed sweeps, budget 163 840 B: (dim, k) -> (bytes at B 8, at B 4, at B 1, class taken).  Footprint 4 * B * dpad + 20 480 +
# 8 * B * k + 16 * B, dpad = dim rounded up to 4.
FM_BUDGET = 160 * 1024
OPT_IN = 64 * 1024                            # above it a launch needs the per-instance hipFuncSetAttribute
SQ8_TABLE = {
    (1536, 10): (70400, 45440, 26720, 8),     # the first B 8 instance past the 64 KiB opt-in, two blocks per CU
    (1536, 200): (82560, 51520, 28240, 8),
    (4096, 10): (152320, 86400, 36960, 8),    # one block per CU, query addresses past 64 KiB, 64 staging chunks
    (4096, 200): (164480, 92480, 38480, 4),   # 164 480 > 163 840: nine queries run 4 + 4 + 1; B 4 past the opt-in
    (4099, 10): (152448, 86464, 36976, 8),    # dpad 4 100, a partial last chunk
    (4099, 200): (164608, 92544, 38496, 4),
    (9000, 10): (309248, 164864, 56576, 1),   # 164 864 > 163 840
    (9000, 200): (321408, 170944, 58096, 1),
}
# half-row Euclidean listed sweeps, budget 163 840 B: (dim, k) -> (bytes at B 16, at B 4, at B 1, class taken).  Footprint 4 * B *
# stride + 8 * B * k + 8 * B, stride = dim rounded up to 8.
HALF_TABLE = {
    (1536, 10): (99712, 24928, 6240, 16),
    (1536, 200): (124032, 31008, 7760, 16),
    (2536, 10): (163712, 40928, 10240, 16),   # 128 B under the limit: the exact-fit launch
    (2544, 10): (164224, 41056, 10272, 4),    # 384 B over it
    (4096, 10): (263552, 65888, 16480, 4),    # the first B 4 instance past the opt-in
    (4095, 10): (263552, 65888, 16480, 4),    # (stride 4 096)
    (10240, 10): (656768, 164192, 41056, 1),  # 164 192 > 163 840
}


# ---- the plans, restated -------------------------------------------------------------------------------------------------------------
def c_lds(B, k, dim):
    """sweep_lds_bytes(B, k, dim, cpl = 0) of csrc/sweep.hip"""
    s = ((B * k * 8 + B * 8) + 15) & ~15
    return (s + B * ((dim + 3) // 4) * 16 + 15) & ~15


def c_passes(nq, k, dim):
    """[(B, queries)] of a group of nq queries in mode C: sweep_listed_plan's rule (csrc/sweep_listed.hip; the GPU tests bind it to
    the product through the launch count of last_filters_exact_plan — it cannot be compiled on the host from a header)"""
    out, left = [], nq
    while left:
        B = 8 if left >= 5 else (4 if left >= 2 else 1)
        while B > 1 and c_lds(B, k, dim) > C_WINDOW:
            B = 4 if B == 8 else 1
        assert c_lds(B, k, dim) <= C_WINDOW
        out.append((B, min(B, left)))
        left -= min(B, left)
    return out


def m_lds(nq, k, dim):
    """listed_m_lds_bytes of csrc/sweep_listed.hip"""
    return nq * ((dim + 127) // 128 * 128) * 4 + 2 * 64 * 68 * 4 + nq * k * 8 + 3 * 16 * 4 + 64 * 4


def m_passes(nq, k, dim):
    """[queries per pass] of a group of nq queries in mode M: sweep_listed_plan's rule"""
    out, left = [], nq
    while left:
        p = min(left, 16)
        while p > 1 and m_lds(p, k, dim) > M_BUDGET:
            p = (p + 1) // 2
        out.append(p)
        left -= p
    return out


def table_passes(half, nq, cap):
    """[(B, queries)] of a group in SQ8 / half Euclidean when `cap` is the widest class the table says fits"""
    out, left = [], nq
    while left:
        B = (16 if left > 4 else (4 if left > 1 else 1)) if half else (8 if left >= 8 else (4 if left >= 4 else 1))
        B = min(B, cap)
        out.append((B, min(B, left)))
        left -= min(B, left)
    return out


def mode_class(half, dim, k, nq):
    """the class the table gives the FIRST pass of nq queries — held to the restated mode_listed_plan of tests/test_gpu_filters_modes.py"""
    cap = (HALF_TABLE if half else SQ8_TABLE)[(dim, k)][3]
    want = table_passes(half, nq, cap)
    assert fms.passes_of(half, nq, k, dim) == want, (half, dim, k, nq, fms.passes_of(half, nq, k, dim), want)
    return want[0][0]


def launches(passes):
    """grouped launches of a call: one per class present"""
    return len({B for B, _ in passes})


# ---- shared state, dropped with the module -------------------------------------------------------------------------------------------
_CASES, _HANDLES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases_and_handles_with_the_module():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _CASES.clear()
    for key in [key for key in fms._SQ8 if (key[1], key[2]) in B_SHAPES]:
        del fms._SQ8[key]


# ================================================================================================ A. per-query filters, f32 exact sweep
A_SHAPES = [(2000, 1536), (2000, 2047), (2000, 2048), (1500, 2432), (1200, 4096), (1200, 4095)]
A_KS = (10, 200)
A_GROUPS = (1, 4, 5, 9, 17, 2)     # queries of the filters below, in their order; + A_UNFILTERED without a filter
A_UNFILTERED = 2


def a_case(metric, n, dim):
    """a shortened fx.mixed_table: six filters — empty, k - 1 rows (k = 10), 65 rows, 1 %, half, a negated 10 % — with 1, 4, 5, 9, 17
    and 2 queries, two unfiltered queries, shuffled"""
    key = ("A", int(metric), n, dim)
    if key not in _CASES:
        rng = np.random.default_rng(5200 * n + dim + int(metric))
        rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
        sets = []
        for c in (0, fx.K0 - 1, 65, max(1, n // 100), n // 2):
            sel = np.sort(rng.choice(n, size=c, replace=False)).astype(np.int64)
            sets.append((sel, False, sel))
        excl = np.sort(rng.choice(n, size=n // 10, replace=False)).astype(np.int64)
        sets.append((excl, True, np.setdiff1d(np.arange(n, dtype=np.int64), excl)))
        fq = [g for g, c in enumerate(A_GROUPS) for _ in range(c)] + [None] * A_UNFILTERED
        fq = [fq[i] for i in rng.permutation(len(fq))]
        _CASES[key] = dict(rows=rows, ids=ids, sets=sets, fq=fq, Q=tf.rand_rows(rng, len(fq), dim, metric))
    return _CASES[key]


class AWorld(fx.World):
    """fx.World over a_case, on a handle sized to its corpus"""

    def __init__(self, metric, n, dim):
        self.c = a_case(metric, n, dim)
        self.ix = ldf.handle(dim, metric, n)
        assert self.ix.upload(self.c["ids"], self.c["rows"]) == n
        self.filters = [self.ix.create_filter(self.c["ids"][given], negate=neg) for given, neg, _ in self.c["sets"]]
        for f, (_, _, sel) in zip(self.filters, self.c["sets"]):
            assert f.matched == len(sel)


def a_expected_launches(mode, k, dim):
    """grouped launches of the forced listed route (every group but the empty one is listed) and the passes of the group of 9 / 17"""
    if mode == "M":
        f16, f9, f8, widest = M_TABLE[(dim, k)]
        assert (m_lds(16, k, dim), m_lds(9, k, dim), m_lds(8, k, dim)) == (f16, f9, f8), (dim, k)
        assert (f16 <= M_BUDGET) == (widest == 16) and f8 <= M_BUDGET and f9 <= M_BUDGET
        assert m_passes(17, k, dim) == ([16, 1] if widest == 16 else [8, 9]) and m_passes(9, k, dim) == [9], (dim, k, m_passes(17, k, dim))
        return 1
    f8, f4, f1, cls = C_TABLE[(dim, k)]
    assert (c_lds(8, k, dim), c_lds(4, k, dim), c_lds(1, k, dim)) == (f8, f4, f1), (dim, k)
    assert cls == (8 if f8 <= C_WINDOW else (4 if f4 <= C_WINDOW else 1)) and f1 <= C_WINDOW
    assert c_passes(9, k, dim) == {8: [(8, 8), (1, 1)], 4: [(4, 4), (4, 4), (1, 1)], 1: [(1, 1)] * 9}[cls], (dim, k, c_passes(9, k, dim))
    assert c_passes(17, k, dim)[0] == (cls, cls) and all(B <= cls for B, _ in c_passes(17, k, dim))
    return launches([p for g in A_GROUPS[1:] for p in c_passes(g, k, dim)])   # (8, 4, 1 present at class 8; 4, 1 at class 4; 1 at class 1)


def run_a(metric, n, dim, engine=1):
    w = AWorld(metric, n, dim)
    try:
        ix, c = w.ix, w.c
        n_sets = len(c["sets"])
        for k in A_KS:
            mode = ldf.mode_name_of(ix, metric, dim, k, engine)
            want_launches = a_expected_launches(mode, k, dim)
            exp = w.alone(c["Q"], c["fq"], k)
            res = {}
            for rname, route in ROUTES.items():
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                got = ix.search_batch_brute_force_with_filters(c["Q"], k, w.table())
                plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
                assert plan[0] == n_sets and plan[3] == A_UNFILTERED and plan[1] + plan[2] == n_sets, (rname, plan)
                assert bool(m & va.KERNEL_SWEEP_LISTED_GROUPS) == (plan[4] > 0) and not m & va.KERNEL_SWEEP_LISTED, (rname, hex(m))
                if rname == "listed":   # every group but the empty one: one launch per class present (mode M: one)
                    assert plan[1] == n_sets - 1 and plan[4] == want_launches and plan[5] == 1, (mode, k, plan, want_launches)
                elif rname == "mask":
                    assert plan[1] == 0 and plan[4] == 0 and plan[5] == 0, plan
                else:                   # auto: whatever it lists stays within the forced listed route's launches
                    assert plan[4] <= want_launches and plan[5] == (1 if plan[1] else 0), (plan, want_launches)
                fx.same(got, exp, (str(metric), n, dim, k, rname, mode))
                res[rname] = got
            for rname in ("listed", "mask"):
                fx.same(res[rname], res["auto"], (str(metric), n, dim, k, "routes agree"))
            empty = [i for i, g in enumerate(c["fq"]) if g == 0]
            assert len(empty) == 1 and res["listed"][2][empty[0]] == 0
            if k == 10:                 # the oracle over each query's subset: independent of the product
                omode = po.MODE_M if mode == "M" else po.MODE_C
                for g, sel in [(g, s[2]) for g, s in enumerate(c["sets"])] + [(None, np.arange(n, dtype=np.int64))]:
                    qi = [i for i, f in enumerate(c["fq"]) if f == g]
                    exp_o = tf.oracle_subset(metric, c["rows"], c["ids"], c["Q"][qi], k, sel, omode)
                    tf.assert_equal(tuple(a[qi] for a in res["listed"]), exp_o, (str(metric), n, dim, "oracle", g))
    finally:
        w.close()


@pytest.mark.parametrize("n,dim", A_SHAPES)
@pytest.mark.parametrize("metric", FLOATS)
def test_per_query_filters_at_large_dims(gpu_required, metric, n, dim):
    """engine 1: Euclidean in mode C everywhere (class 8 only at dim 1 536 with k = 10, class 4 to dim 2 432, class 1 at 4 096 /
    4 095); Cosine / DotProduct in mode M up to 2 048 (2 432 at k = 10), passes of 16 at 1 536 and of 8 from 2 047, mode C behind"""
    run_a(metric, n, dim)


@pytest.mark.parametrize("n,dim", [(2000, 2047), (1200, 4096)])
def test_per_query_filters_cosine_mode_c_body_at_large_dims(gpu_required, n, dim):
    """engine 0: the grouped mode-C Cosine body with the query in LDS at class 4 (2 047, a predicated tail) and class 1 (4 096)"""
    va.set_sweep_engine(0)
    try:
        run_a(DM.Cosine, n, dim, engine=0)
    finally:
        va.set_sweep_engine(1)


@pytest.mark.parametrize("metric", [DM.Euclidean, DM.Cosine])
def test_per_query_filters_beyond_every_lds_plan(gpu_required, metric):
    """ldf.test_filtered_beyond_every_lds_plan's shape as a per-query call — two filters and one unfiltered query.  One query is
    65 632 B, above the 60 KiB window.  That takes the listed plan away, so no group may take the grouped route — and it is the very
    condition under which the exact vector-ALU tier refuses (64 rows and 8 queries in mode C reach no other tier), so at this shape
    the plain call, the one-filter calls and the per-query call all answer VDB_ERR_UNSUPPORTED: there are no answers to compare.
    What is checked is that refusal — the same status from every call of the loop and from the per-query call on every route,
    never a launch failure — and the plan the refused call leaves in its diagnostic, which is filled before anything launches:
    both groups on mask substitution, no grouped launch, no merge, no listed kernel bit"""
    n, dim, k = 64, 16384, 10
    assert c_lds(1, k, dim) == 65632 > C_WINDOW
    rng = np.random.default_rng(16384 + int(metric))
    rows, ids = tf.rand_rows(rng, n, dim, metric), tf.ext_ids(n)
    fq = [0, 1, None, 1, 0, 0, 1, 0]
    Q = tf.rand_rows(rng, len(fq), dim, metric)
    sels = [np.sort(rng.choice(n, n // 2, replace=False)), np.sort(rng.choice(n, k - 1, replace=False))]
    ix = ldf.handle(dim, metric, n)
    flts = []
    try:
        ix.upload(ids, rows)
        assert ix.sweep_arith_mode(k) == "C"

        def refused(fn, what):
            with pytest.raises(va.VelesHipError) as e:
                fn()
            assert e.value.code == UNSUPPORTED, (what, e.value.code, str(e.value))
            return str(e.value)

        assert "too large for the fused top-k path" in refused(lambda: ix.search_batch_brute_force(Q, k), "plain")
        flts = [ix.create_filter(ids[s]) for s in sels]
        table = [None if g is None else flts[g] for g in fq]
        for rname, route in ROUTES.items():
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            for i, g in enumerate(fq):     # the loop of one-query calls the per-query call is held to: each refuses the same way
                if g is None:
                    refused(lambda: ix.search_batch_brute_force(Q[i:i + 1], k), (rname, i))
                else:
                    refused(lambda: ix.search_batch_brute_force_filtered(Q[i:i + 1], k, flts[g]), (rname, i))
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED, (rname, i, hex(ix.last_kernels()))
            refused(lambda: ix.search_batch_brute_force_with_filters(Q, k, table), rname)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            assert plan == (2, 0, 2, 1, 0, 0), (rname, plan)
            assert not m & (va.KERNEL_SWEEP_LISTED_GROUPS | va.KERNEL_SWEEP_LISTED), (rname, hex(m))
    finally:
        for f in flts:
            f.close()
        ix.close()


# ================================================================================================ B. SQ8, one filter and per query
B_SHAPES = [(1500, 1536), (1200, 4096), (1000, 4099), (300, 9000)]
B_KS = (10, 200)
B_METRICS = [DM.Cosine, DM.Euclidean, DM.DotProduct]
B_SIZES = [(0, 9), (1, 7), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (None, 2)]   # fms.test_sq8_mixed_table_bit_exact's 23 queries


def sq8_handle(metric, n, dim):
    """the rows of fms.sq8_case (special_rows with copies: constant-vector rows, duplicates) on a handle sized to them"""
    key = ("sq8", int(metric), n, dim)
    if key not in _HANDLES:
        c = fms.sq8_case(metric, n, dim)
        ix = ldf.handle(dim, metric, n)
        ix.set_storage_mode(SM.SQ8)
        assert ix.upload(c["ids"], c["rows"]) == n
        _HANDLES[key] = ix
    return _HANDLES[key]


def sq8_expected(metric, n, dim, k, name, sel):
    """the oracle's SQ8 search over the set's rows for all 23 queries of the case: once, any prefix or subset of it serves a call"""
    key = ("sq8exp", int(metric), n, dim, k, name)
    if key not in _CASES:
        c = fms.sq8_case(metric, n, dim)
        _CASES[key] = fm.sq8_subset(metric, c["rows"], c["ids"], c["Q"], k, sel)
    return _CASES[key]


@pytest.mark.parametrize("k", B_KS)
@pytest.mark.parametrize("metric", B_METRICS)
@pytest.mark.parametrize("n,dim", B_SHAPES)
def test_sq8_one_filter_at_large_dims(gpu_required, metric, n, dim, k):
    c, ix = fms.sq8_case(metric, n, dim), sq8_handle(metric, n, dim)
    cap = SQ8_TABLE[(dim, k)][3]
    assert [mode_class(False, dim, k, nq) for nq in (1, 4, 9)] == [1, min(4, cap), cap]
    excl, _, long_sel = c["long_set"]
    for name, given, negate, sel in (("not10pct", excl, True, long_sel), ("65", c["picks"][65], False, c["picks"][65])):
        exp = sq8_expected(metric, n, dim, k, name, sel)
        with ix.create_filter(c["ids"][given], negate=negate) as flt:
            assert flt.matched == len(sel)
            for nq in (1, 4, 9):
                res = []
                for route in (LISTED, MASK):
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    got = ix.search_batch_filtered_sq8(c["Q"][:nq], k, flt)
                    m = ix.last_kernels()
                    assert bool(m & va.KERNEL_SWEEP_LISTED) == (route == LISTED) and m & va.KERNEL_SQ8, (name, nq, route, hex(m))
                    assert not m & va.KERNEL_SWEEP_LISTED_GROUPS, hex(m)
                    tf.assert_equal(got, exp[:nq], (str(metric), n, dim, k, name, nq, route))
                    res.append(got)
                assert np.array_equal(res[0][2], res[1][2])
                for qi, cnt in enumerate(res[0][2]):
                    assert np.array_equal(res[0][0][qi, :cnt], res[1][0][qi, :cnt]) and np.array_equal(tf.bits(res[0][1][qi, :cnt]), tf.bits(res[1][1][qi, :cnt]))


@pytest.mark.parametrize("k", B_KS)
@pytest.mark.parametrize("metric", B_METRICS)
@pytest.mark.parametrize("n,dim", B_SHAPES)
def test_sq8_per_query_filters_at_large_dims(gpu_required, metric, n, dim, k):
    """fms.test_sq8_mixed_table_bit_exact's table: groups of 9 and 7 queries, five of one (lists of 63, 1, 64 and k - 1 rows, one
    empty), two unfiltered.  Class 8: launches at 8, 4 and 1 (9 = 8 + 1, 7 = 4 + 1 + 1 + 1); class 4: two launches (9 = 4 + 4 + 1);
    class 1: one launch of one-query items"""
    c, ix = fms.sq8_case(metric, n, dim), sq8_handle(metric, n, dim)
    cap = SQ8_TABLE[(dim, k)][3]
    assert mode_class(False, dim, k, 9) == cap
    assert table_passes(False, 9, cap) == {8: [(8, 8), (1, 1)], 4: [(4, 4), (4, 4), (1, 1)], 1: [(1, 1)] * 9}[cap]
    want_launches = launches(table_passes(False, 9, cap) + table_passes(False, 7, cap) + [(1, 1)])
    assert want_launches == {8: 3, 4: 2, 1: 1}[cap]
    rows, ids, Q = c["rows"], c["ids"], c["Q"]
    excl, _, long_sel = c["long_set"]
    km1 = np.sort(np.random.default_rng(n + dim + k).choice(n, size=k - 1, replace=False)).astype(np.int64)
    sels = [long_sel, c["picks"][65], c["picks"][63], c["picks"][1], c["picks"][64], km1, np.empty(0, np.int64)]
    fq = fms.interleave(B_SIZES, 5)
    assert len(fq) == Q.shape[0]
    filters = [ix.create_filter(ids[excl], negate=True)] + [ix.create_filter(ids[s]) for s in sels[1:]]
    try:
        assert [f.matched for f in filters] == [len(s) for s in sels]
        table = [None if g is None else filters[g] for g in fq]
        counts = {f: len(s) for f, s in zip(filters, sels)}
        by_set = {**dict(enumerate(sels)), None: np.arange(n, dtype=np.int64)}
        subset = lambda qi, sel: fm.sq8_subset(metric, rows, ids, Q[qi], k, sel)  # noqa: E731
        res = {}
        for rname, route in ROUTES.items():
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = ix.search_batch_with_filters_sq8(Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            want, _ = fms.predict(route, va.MODE_BRUTE_SQ8, metric, table, counts, n, k, dim)
            assert plan == want, (rname, plan, want)
            if rname == "listed":
                assert plan == (7, 6, 1, 2, want_launches, 1), (cap, plan)
            elif rname == "auto":      # an SQ8 group goes listed only with at most three queries: the five one-query groups but the empty one
                assert plan == (7, 4, 3, 2, 1, 1), plan
            else:
                assert plan == (7, 0, 7, 2, 0, 0), plan
            assert bool(m & va.KERNEL_SWEEP_LISTED_GROUPS) == (plan[4] > 0) and m & va.KERNEL_SQ8 and not m & va.KERNEL_SWEEP_LISTED, (rname, hex(m))
            fms.oracle_check(got, fq, by_set, subset)
            res[rname] = got
        for rname in ("auto", "mask"):
            fx.same(res["listed"], res[rname], (str(metric), n, dim, k, "listed against", rname))
            fx.same(res[rname], res["listed"], (str(metric), n, dim, k, rname, "against listed"))
    finally:
        for f in filters:
            f.close()


# ================================================================================================ C. half images and sign bits
C_EUCLID = [(1200, 1536), (800, 2536), (800, 2544), (800, 4096), (800, 4095), (300, 10240)]
HALF_MODES = {"f16": fms.F16, "bf16": fms.BF16}


def half_handle(metric, prec, ids, rows):
    """fm.half_index on a handle sized to its corpus: half the rows converted by enable_half_precision, half on arrival"""
    n = len(ids)
    ix = ldf.handle(rows.shape[1], fm.HMETRIC[metric], n)
    ix.upload(ids[: n // 2], rows[: n // 2])
    ix.enable_half_precision(fm.vp(prec))
    ix.upload(ids[n // 2:], rows[n // 2:])
    return ix


@pytest.mark.parametrize("M", [fms.F16, fms.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n,dim", C_EUCLID)
def test_half_euclidean_listed_sweeps_at_large_dims(gpu_required, M, n, dim):
    """hp.ints rows (integers in [-4, 4]: squared differences <= 64, 10 240 of them stay below 2^24, so every order of summation
    gives the oracle's bits), one filter with 1 / 4 / 17 queries and fms.HALF_SIZES' table (groups of 17, 5, 3, 1, 1, 1 and two
    unfiltered), both routes.  Class 16: launches at 16, 4 and 1; class 4: 17 = 4 + 4 + 4 + 4 + 1, two launches; class 1: one"""
    assert dim * 64 < 2 ** 24
    rng = np.random.default_rng(41 * n + dim + M.prec)
    rows, ids = hp.ints(rng, (n, dim)), tf.ext_ids(n)
    rows[[5, n - 2]] = 0.0
    rows[[256, 257]] = rows[[1, 1]]
    sets = fms.half_sets(rng, n)
    fq = fms.interleave(fms.HALF_SIZES, 9)
    Q = hp.ints(rng, (len(fq), dim))
    Q[0] = rows[n - 1]
    sels = {name: s[2] for name, s in sets.items()}
    sels[None] = np.arange(n, dtype=np.int64)
    ix = half_handle(hr.EUCLIDEAN, M.prec, ids, rows)
    filters = {}
    try:
        filters = {name: ix.create_filter(ids[given], negate=neg) for name, (given, neg, _) in sets.items()}
        table = [None if g is None else filters[g] for g in fq]
        counts = {filters[name]: len(sels[name]) for name in filters}
        for k in [kk for d, kk in HALF_TABLE if d == dim]:
            cap = HALF_TABLE[(dim, k)][3]
            assert [mode_class(True, dim, k, nq) for nq in (1, 4, 17)] == [1, min(4, cap), cap]
            assert table_passes(True, 17, cap) == {16: [(16, 16), (1, 1)], 4: [(4, 4)] * 4 + [(1, 1)], 1: [(1, 1)] * 17}[cap]
            # ---- one filter
            for name in ("not10pct", "1pct"):
                exp = fm.half_subset(hr.EUCLIDEAN, M.prec, rows, ids, Q[:17], k, sels[name])
                for nq in (1, 4, 17):
                    for route in (LISTED, MASK):
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        got = ix.search_batch_filtered_half(Q[:nq], k, filters[name], fm.vp(M.prec))
                        m = ix.last_kernels()
                        assert m & va.KERNEL_SWEEP_HALF_L2 and bool(m & va.KERNEL_SWEEP_LISTED) == (route == LISTED), (name, nq, route, hex(m))
                        assert not m & va.KERNEL_SWEEP_LISTED_GROUPS, hex(m)
                        tf.assert_equal(got, exp[:nq], (M.prec, n, dim, k, name, nq, route))
            # ---- one filter per query
            want_launches = launches([p for _, c in fms.HALF_SIZES[:5] for p in table_passes(True, c, cap)])
            assert want_launches == {16: 3, 4: 2, 1: 1}[cap]
            subset = lambda qi, sel: fm.half_subset(hr.EUCLIDEAN, M.prec, rows, ids, Q[qi], k, sel)  # noqa: E731
            res = []
            for route in (LISTED, MASK):
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                got = M.table_call(ix, Q, k, table)
                plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
                want, _ = fms.predict(route, M.mode, DM.Euclidean, table, counts, n, k, dim)
                assert plan == want == ((6, 5, 1, 2, want_launches, 1) if route == LISTED else (6, 0, 6, 2, 0, 0)), (route, plan, want)
                assert m & va.KERNEL_SWEEP_HALF_L2 and bool(m & va.KERNEL_SWEEP_LISTED_GROUPS) == (route == LISTED) and not m & va.KERNEL_SWEEP_LISTED, hex(m)
                fms.oracle_check(got, fq, sels, subset)
                res.append(got)
            fx.same(res[0], res[1], (M.prec, n, dim, k, "listed against mask"))
            fx.same(res[1], res[0], (M.prec, n, dim, k, "mask against listed"))
    finally:
        for f in filters.values():
            f.close()
        ix.close()


C_DOT_SIZES = [("half", 9), ("1pct", 5), ("not10pct", 3), (None, 2)]


@pytest.mark.parametrize("M,metric", [(fms.F16, hr.COSINE), (fms.F16, hr.DOT), (fms.BF16, hr.COSINE), (fms.BF16, hr.DOT)], ids=["f16-cos", "f16-dot", "bf16-cos", "bf16-dot"])
@pytest.mark.parametrize("data", ["ints", "gauss"])
@pytest.mark.parametrize("n,dim", [(1200, 1536), (800, 4096)])
def test_half_cosine_dot_under_a_mask_at_large_dims(gpu_required, M, metric, data, n, dim):
    """mask substitution on every tier (no listed kernel): hp.ints rows (products <= 16, 4 096 of them far below 2^24) bit for bit
    the subset oracle, N(0, 1) rows within hp.TOL (hp.check, tie-aware); one filter with 1 / 16 / 70 queries and one per-query call
    of three groups, bit for bit the one-filter call over each group"""
    k = 10
    rng = np.random.default_rng(83 + 5 * M.prec + metric + len(data) + dim)
    make = (lambda shape: hp.ints(rng, shape)) if data == "ints" else (lambda shape: rng.standard_normal(shape).astype(np.float32))
    rows = make((n, dim))
    ids = tf.ext_ids(n) if data == "ints" else np.arange(n, dtype=np.uint64)
    sets = fms.half_sets(rng, n)
    sels = {name: s[2] for name, s in sets.items()}
    sels[None] = np.arange(n, dtype=np.int64)
    ix = half_handle(metric, M.prec, ids, rows)
    filters = {}
    try:
        filters = {name: ix.create_filter(ids[given], negate=neg) for name, (given, neg, _) in sets.items()}

        def held(got, Q, sel, sample=None):
            if data == "ints":
                tf.assert_equal(got, fm.half_subset(metric, M.prec, rows, ids, Q, k, sel), (M.prec, metric, n, dim, len(sel), Q.shape[0]))
            else:
                gi, gs, gc = got
                hp.check(metric, M.prec, rows[sel], Q, k, fm.positions(sel, gi, gc), gs, gc, sample)

        for nq in (1, 16, 70):
            Q = make((nq, dim))
            for name in ("half", "1pct"):
                for route in (AUTO, LISTED):
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    got = ix.search_batch_filtered_half(Q, k, filters[name], fm.vp(M.prec))
                    hp.served_by(ix, hp.tier_bits(metric, M.prec, nq, n, dim, k), va.KERNEL_SWEEP_LISTED | va.KERNEL_SWEEP_LISTED_GROUPS)
                    if route == AUTO:
                        held(got, Q, sels[name], None if nq <= 16 else [0, 1, nq // 2, nq - 1])
                        first = got
                    else:
                        fx.same(got, first, (M.prec, metric, data, name, nq, "the forced listed route is mask substitution too"))
        fq = fms.interleave(C_DOT_SIZES, 9)
        Q = make((len(fq), dim))
        table = [None if g is None else filters[g] for g in fq]
        ix.set_option(va.OPT_FILTER_ROUTE, AUTO)
        exp = fms.by_group(M, ix, Q, k, table)
        for route in (AUTO, LISTED):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = M.table_call(ix, Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            assert plan == (3, 0, 3, 2, 0, 0), (route, plan)
            assert not m & (va.KERNEL_SWEEP_LISTED_GROUPS | va.KERNEL_SWEEP_LISTED), hex(m)
            assert bool(m & va.KERNEL_F16) == (M.prec == hr.F16), hex(m)
            fx.same(got, exp, (M.prec, metric, data, route))
            for name, _ in C_DOT_SIZES:
                qi = [i for i, g in enumerate(fq) if g == name]
                held(tuple(a[qi] for a in got), Q[qi], sels[name])
    finally:
        for f in filters.values():
            f.close()
        ix.close()


@pytest.mark.parametrize("n,dim", [(1000, 4096), (1000, 4099)])
def test_binary_under_a_mask_at_large_dims(gpu_required, n, dim):
    """sign bits of 4 096 and 4 099 dimensions (128 words; 128 words and three bits), thirty equal codes: exact integers, ties by row"""
    k = 12
    rng = np.random.default_rng(n + 3 * dim)
    rows, ids = fm.with_copies(special_rows(rng, n, dim)), tf.ext_ids(n)
    rows[50:80] = rows[49]
    sets = fms.half_sets(rng, n)
    sels = {name: s[2] for name, s in sets.items()}
    sels[None] = np.arange(n, dtype=np.int64)
    fq = fms.interleave([("not10pct", 6), ("half", 2), ("k-1", 1), ("empty", 1), (None, 2)], 3)
    Q = rng.standard_normal((len(fq), dim)).astype(np.float32)
    Q[0] = rows[49]
    ix = ldf.handle(dim, DM.Euclidean, n)
    filters = {}
    try:
        ix.upload(ids, rows)
        ix.set_storage_mode(SM.Binary)
        filters = {name: ix.create_filter(ids[given], negate=neg) for name, (given, neg, _) in sets.items()}
        for name in ("not10pct", "half", "k-1"):
            for nq in (1, 6):
                for route in (AUTO, LISTED):
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    got = ix.search_batch_filtered_binary(Q[:nq], k, filters[name])
                    m = ix.last_kernels()
                    assert m & va.KERNEL_BITS and not m & (va.KERNEL_SWEEP_LISTED | va.KERNEL_SWEEP_LISTED_GROUPS), hex(m)
                    tf.assert_equal(got, fm.binary_subset(rows, ids, Q[:nq], k, sels[name]), (n, dim, name, nq, route))
        table = [None if g is None else filters[g] for g in fq]
        exp = fms.alone(fms.BINARY, ix, Q, k, table)
        for route in (AUTO, LISTED, MASK):
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            got = ix.search_batch_with_filters_binary(Q, k, table)
            plan, m = ix.last_filters_exact_plan(), ix.last_kernels()
            assert plan == (4, 0, 4, 2, 0, 0), (route, plan)
            assert m & va.KERNEL_BITS and not m & (va.KERNEL_SWEEP_LISTED_GROUPS | va.KERNEL_SWEEP_LISTED), hex(m)
            fx.same(got, exp, (n, dim, route))
            fms.oracle_check(got, fq, sels, lambda qi, sel: fm.binary_subset(rows, ids, Q[qi], k, sel))
    finally:
        for f in filters.values():
            f.close()
        ix.close()


# ================================================================================================ D. half walk with the f32 re-score
D_SHAPES = hw.LARGE_SHAPES[3:]
D_KEF = (10, 64, 4)     # k, ef, ratio: cand_k 40, ef_w 64


@pytest.fixture(scope="module")
def rescore_worlds(tmp_path_factory):
    """fr.World (the oracle-built graph over Gaussian rows, dumped) and gr.Handle (the handle that loaded it, both images)"""
    root, cache = str(tmp_path_factory.mktemp("large_half_rescore")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            w = fr.World(root, metric, shape)
            cache[(metric, shape)] = (w, gr.Handle(w))
        return cache[(metric, shape)]
    yield get
    for _, h in cache.values():
        h.close()


def assert_exact_f32_scores(w, v, ids, sc, cnt):
    """every returned score is the f32 engine distance of the UNROUNDED query to the f32 row, as a score: bit for bit"""
    for qi in range(len(cnt)):
        c = int(cnt[qi])
        ds = po.batch_distance(v.metric, w.qs[qi], w.rows[ids[qi, :c].astype(np.int64)], po.MODE_C)
        assert np.array_equal(sc[qi, :c].view(np.uint32), fw.score_bits(v.metric, list(ds))), qi


@pytest.mark.parametrize("prec", fr.PRECISIONS)
@pytest.mark.parametrize("shape", D_SHAPES, ids=gr.SHAPE_IDS)
@pytest.mark.parametrize("metric", [hr.COSINE, hr.EUCLIDEAN])
def test_half_rescore_walk_at_large_generic_dims(gpu_required, rescore_worlds, metric, shape, prec):
    (w, h), (k, ef, ratio) = rescore_worlds(metric, shape), D_KEF
    v = w.view(prec)
    cap_max = h.largest(k, ratio)
    # ---- no filter: the plain call and the per-query call with no table entry
    want = fr.expect_call(v, w.filters["all"], k, ef, ratio, va.ROUTE_AUTO, max_list=cap_max)
    assert want[2] == [1] * gr.NQ
    ids, sc, cnt = h.ix.search_batch_half_rescore(w.qs, k, gr.MODE[prec], ef=ef, oversampling=ratio)
    kern, stats = h.ix.last_kernels(), h.ix.last_search_stats()
    assert kern & va.KERNEL_HALF_RESCORE and kern & va.KERNEL_HNSW_HALF and bool(kern & va.KERNEL_F16) == (prec == hr.F16), hex(kern)
    assert not kern & va.KERNEL_FILTER_RANK, hex(kern)
    fr.assert_call(((ids, sc, cnt), np.ones(gr.NQ, np.uint32), stats), want, (metric, shape, prec, "plain"))
    assert_exact_f32_scores(w, v, ids, sc, cnt)
    none = gr.batch(h.ix, w.qs, k, [None] * gr.NQ, prec, ef, ratio)
    assert none[3] == gr.walk_bits(prec), hex(none[3])
    fr.assert_call(none[:3], want, (metric, shape, prec, "no table entry"))
    # ---- one filter, the walk and the exact pass
    for name in ("half", "tenth"):
        allowed = w.filters[name]
        for route in (va.ROUTE_WALK, va.ROUTE_EXACT):
            want = fr.expect_call(v, allowed, k, ef, ratio, route, max_list=cap_max)
            assert want[2] == [1 if route == va.ROUTE_WALK else 2] * gr.NQ, "the reference itself overflows the largest list at this shape"
            got = gr.one(h.ix, w.qs, k, h.flt(name), prec, ef, ratio, route=route)
            kern = h.ix.last_kernels()
            assert kern == (gr.walk_bits(prec) if route == va.ROUTE_WALK else va.KERNEL_FILTER_RANK), (name, route, hex(kern))
            fr.assert_call(got, want, (metric, shape, prec, name, route))
            assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])
            assert_exact_f32_scores(w, v, *got[0])
    # ---- both filters and None in one call: every query what the reference gives it alone
    names = [("half", "tenth", None)[i % 3] for i in range(gr.NQ)]
    got = gr.batch(h.ix, w.qs, k, [h.flt(nm) for nm in names], prec, ef, ratio)
    (ids, sc, cnt), routes, stats, kern = got
    assert kern == gr.walk_bits(prec), hex(kern)
    nd = ne = 0
    for qi, nm in enumerate(names):
        wi, wb, wr, ws = fr.expect_call(v, w.filters[nm or "all"], k, ef, ratio, va.ROUTE_AUTO, max_list=cap_max, qs=w.qs[qi:qi + 1])
        c = int(cnt[qi])
        assert wr == [1] and int(routes[qi]) == 1 and ids[qi, :c].tolist() == wi[0], (qi, nm)
        assert np.array_equal(sc[qi, :c].view(np.uint32), wb[0]), (qi, nm)
        assert np.all(ids[qi, c:] == fr.PAD_ID) and np.all(sc[qi, c:].view(np.uint32) == 0x7FC00000), (qi, nm)
        nd, ne = nd + ws[0], ne + ws[1]
    assert tuple(stats) == (nd, ne), (stats, nd, ne)
    assert_exact_f32_scores(w, v, ids, sc, cnt)


@pytest.mark.parametrize("metric", [hr.COSINE, hr.EUCLIDEAN])
def test_hybrid_over_the_rescore_walk_at_dim_1536(gpu_required, rescore_worlds, metric):
    """the two-phase lease of the hybrid call (unfiltered queries at 2k, filtered ones at max(4k, k + 10)) over WALK_ROWS_F16_RESCORE:
    tests/hybrid_ref.py's fusion of the lists the re-score call returns for each query alone"""
    (w, h), k = rescore_worlds(metric, D_SHAPES[0]), 10
    assert w.dim == 1536
    rng = np.random.default_rng(1536 + metric)
    names = [None, "half", "tenth", "half", None, "tenth", "half", None]
    filters = [h.flt(nm) for nm in names]
    weights = np.array([0.5, 0.0, 1.0, 0.3, 0.8, 0.5, 0.7, 0.2], np.float32)
    live = set(range(w.n))
    lists, texts = [], []
    for qi, flt in enumerate(filters):
        kf = max(4 * k, k + 10) if flt is not None else 2 * k
        (ids, _, cnt), _ = h.ix.search_batch_with_filters_half_rescore(w.qs[qi:qi + 1], kf, [flt], va.MODE_HNSW_F16)
        # ("tenth" has fewer rows than the list of 40 walks at ef 160: the auto rule answers those queries with the exact pass)
        assert h.ix.last_kernels() in (gr.walk_bits(hr.F16), va.KERNEL_FILTER_RANK), hex(h.ix.last_kernels())
        assert (h.ix.last_kernels() == va.KERNEL_FILTER_RANK) == (names[qi] == "tenth"), (qi, hex(h.ix.last_kernels()))
        lists.append([int(ids[0, j]) for j in range(int(cnt[0]))])
        near = rng.choice(lists[-1], size=len(lists[-1]) // 2, replace=False).tolist()
        other = rng.choice(w.n, size=kf, replace=False).tolist()
        mix = [int(i) for i in near + other + [w.n + 5, 0xFFFFFFFFFFFFFFFF]]
        texts.append([mix[j] for j in rng.permutation(len(mix))[:kf]])
    got = h.ix.hybrid_search_batch_filters(w.qs, texts, k, weights, filters, va.WALK_ROWS_F16_RESCORE)
    kern = h.ix.last_kernels()
    assert kern & va.KERNEL_HYBRID_FUSE and kern & va.KERNEL_HALF_RESCORE and kern & va.KERNEL_F16, hex(kern)
    for qi, nm in enumerate(names):
        allowed = None if nm is None else set(np.flatnonzero(w.filters[nm]).tolist())
        c = hc.case(lists[qi], texts[qi], float(weights[qi]), dead=set(texts[qi]) - live, allowed=allowed)
        eid, ebits, en = hyr.top(hc.reference(c, k, all_live=False), k)
        assert got[2][qi] == en and np.array_equal(got[0][qi], eid) and np.array_equal(got[1][qi].view(np.uint32), ebits), (qi, nm)
