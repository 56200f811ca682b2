"""The gathered matrix-core tiers (FILTER_ROUTE_GATHERED; DESIGN 4.1s half rows, 4.1t packed bits) at the edges their own test files
leave out: a second chunk of a call past 1 024 queries, the TN = 128 -> 16 fallback at 64 or more queries, dims below a slice / no
multiple of 8 or 32 / above 1 024, f16 subnormals, inf and NaN, the Cosine rule for norms below f32::EPSILON, rows appended after the
filter was made, whole tiles of dead rows.  The cases, their data and references: tests/gathered_edge_cases.py (held to the tiers'
launch plan by tests/test_gathered_edges_cpu.py).  Every gathered call asserts the tier's kernel bits and is repeated under mask
substitution (route 2) on the same handle: ids, counts and score bits must agree, next to the numpy reference.  Integer data and bits:
bit for bit; Gaussian data: tests/test_gpu_half_precision.py::check with its TOL."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gathered_edge_cases as ge  # noqa: E402
import half_ref as hr  # noqa: E402
import test_gpu_bits_gathered as bg  # noqa: E402
import test_gpu_filtered as tf  # noqa: E402
import test_gpu_filtered_modes as fm  # noqa: E402
import test_gpu_half_gathered as hg  # noqa: E402
import test_gpu_half_precision as hp  # noqa: E402

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
TIERS = ge.HALF + ge.BITS
GATHER_BITS = va.KERNEL_GEMM_HALF_GATHERED | va.KERNEL_BITS_GATHERED


def index(tier, ids, rows):
    return fm.half_index(tier[2], tier[1], ids, rows) if tier[0] == "half" else bg.index(tier[1], ids, rows)


def gathered(tier, ix, Q, k, flt=None, table=None):
    """the call under route 3, held to the tier's kernel bits"""
    ix.set_option(va.OPT_FILTER_ROUTE, 3)
    if tier[0] == "bits":
        return bg.gathered(tier[1], ix, Q, k, flt, table)
    if table is None:
        return hg.gathered(ix, Q, k, flt, tier[1])
    got = ix.search_batch_brute_force_with_filters_half(Q, k, table, fm.vp(tier[1]))
    hp.served_by(ix, hg.bits_of(tier[1]))
    return got


def masked(tier, ix, Q, k, flt=None, table=None):
    """the same call under mask substitution: no gathered kernel"""
    ix.set_option(va.OPT_FILTER_ROUTE, 2)
    try:
        if tier[0] == "bits":
            got = bg.call(tier[1], ix, Q, k, flt, table)
        elif table is None:
            got = ix.search_batch_filtered_half(Q, k, flt, fm.vp(tier[1]))
        else:
            got = ix.search_batch_brute_force_with_filters_half(Q, k, table, fm.vp(tier[1]))
        assert not ix.last_kernels() & GATHER_BITS, hex(ix.last_kernels())
    finally:
        ix.set_option(va.OPT_FILTER_ROUTE, 3)
    return got


def same(a, b, what, nan_payload_free=False):
    """ids, counts and score bits of two answers (nan_payload_free: a NaN must sit where a NaN sits, its payload is not compared)"""
    assert np.array_equal(a[2], b[2]), (what, "counts")
    for qi in range(len(a[2])):
        c = a[2][qi]
        assert np.array_equal(a[0][qi, :c], b[0][qi, :c]), (what, qi, "ids")
        x, y = a[1][qi, :c], b[1][qi, :c]
        if nan_payload_free:
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, qi, "NaN positions")
            x, y = x[~np.isnan(x)], y[~np.isnan(y)]
        assert np.array_equal(tf.bits(x), tf.bits(y)), (what, qi, "score bits")


def both(tier, ix, Q, k, flt, what):
    got = gathered(tier, ix, Q, k, flt)
    same(got, masked(tier, ix, Q, k, flt), what)
    return got


def run_plain_case(case, d=None, sc=None):
    """every (set, shape) of a case against the reference and against route 2; 1 024 queries: the 130, repeated"""
    d = d or ge.data(case)
    ix = index(case.tier, d.ids, d.rows)
    try:
        for name in case.sets:
            given, negate, sel = d.sets[name]
            with ix.create_filter(d.ids[given], negate=negate) as flt:
                for nq, k in case.shapes:
                    pick = np.arange(nq) % len(d.Q)
                    exp = ge.expected(case.tier, d.sc[: min(nq, len(d.Q))], d.ids, k, sel)
                    tf.assert_equal(both(case.tier, ix, d.Q[pick], k, flt, (case, name, nq, k)), [exp[i] for i in pick], (case, name, nq, k))
    finally:
        ix.close()


# ---- a. two chunks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_a_call_past_1024_queries_answers_every_chunk(gpu_required, tier):
    """1 030 queries (second chunk: 6, the 16-query instance) and 1 088 (64, the 128-query instance), pairwise distinct, all of them
    against the reference; then 1 100 queries with one filter each, 1 030 of them on one filter."""
    c16, c128 = ge.cases("chunks", [tier])
    d = ge.data(c16)
    ix = index(tier, d.ids, d.rows)
    try:
        flts = {}
        for name in c16.sets:
            given, negate, sel = d.sets[name]
            flts[name] = ix.create_filter(d.ids[given], negate=negate)
            exp = ge.expected(tier, d.sc, d.ids, 10, sel)
            for case in (c16, c128):
                ((nq, k),) = case.shapes
                tf.assert_equal(both(tier, ix, d.Q[:nq], k, flts[name], (tier, name, nq)), exp[:nq], (tier, name, nq))
        own = ge.table_owners()
        by = [flts["65"], flts["half"], None]
        table = [by[o] for o in own]
        got = gathered(tier, ix, d.Q, 10, table=table)
        same(got, masked(tier, ix, d.Q, 10, table=table), (tier, "table"))
        exp = [ge.expected(tier, d.sc, d.ids, 10, d.sets[name][2]) for name in ("65", "half")]
        none = np.flatnonzero(own == 2)
        pi, ps, pc = hp.search(ix, d.Q[none], 10, tier[1]) if tier[0] == "half" else bg.call(tier[1], ix, d.Q[none], 10)
        one = [gathered(tier, ix, d.Q[own == o], 10, by[o]) for o in (0, 1)]       # each query's one-filter call (A's: itself chunked, held above)
        at = [np.flatnonzero(own == o) for o in (0, 1)]
        for i in range(len(own)):
            o = own[i]
            if o == 2:
                j = int(np.searchsorted(none, i))
                oi, os_, oc = pi[j], ps[j], pc[j]
            else:
                j = int(np.searchsorted(at[o], i))
                oi, os_, oc = one[o][0][j], one[o][1][j], one[o][2][j]
                assert oc == len(exp[o][i][0]) and np.array_equal(oi[:oc], exp[o][i][0]) and np.array_equal(tf.bits(os_[:oc]), tf.bits(exp[o][i][1])), i
            assert oc == got[2][i] and np.array_equal(oi, got[0][i]) and np.array_equal(tf.bits(os_), tf.bits(got[1][i])), i
        for f in flts.values():
            f.close()
    finally:
        ix.close()


# ---- b. the TN fallback at 64 or more queries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_k_lists_that_do_not_fit_128_queries_fall_back_to_sixteen_query_tiles(gpu_required, tier):
    """n = 9 000 at the largest k with 128-query tiles and at k + 1: nine 16-query tiles at 130 queries, sixty-four at 1 024 (a block then
    walks nine row tiles: the three-slot rotation wraps three times).  One handle for the three cases."""
    cs = ge.cases("fallback", [tier])
    d = ge.data(cs[0])
    ix = index(tier, d.ids, d.rows)
    try:
        for name in ("all", "65", "not10pct"):
            given, negate, sel = d.sets[name]
            with ix.create_filter(d.ids[given], negate=negate) as flt:
                for case in cs:
                    if name not in case.sets:
                        continue
                    ((nq, k),) = case.shapes
                    exp = ge.expected(tier, d.sc, d.ids, k, sel)
                    pick = np.arange(nq) % 130
                    tf.assert_equal(both(tier, ix, d.Q[pick], k, flt, (tier, name, nq, k)), [exp[i] for i in pick], (tier, name, nq, k))
    finally:
        ix.close()


# ---- c. dims --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ge.cases("dims"), ids=lambda c: "-".join(map(str, c.tier + (c.dim,))))
def test_dims_bit_for_bit(gpu_required, case):
    run_plain_case(case)


@pytest.mark.parametrize("dim", [d for d in ge.HALF_DIMS if d > 1024])
@pytest.mark.parametrize("prec,metric", hg.CASES)
def test_dims_above_1024_gaussian_within_the_modes_tolerance(gpu_required, prec, metric, dim):
    n = 1500
    rng = np.random.default_rng([dim, prec, metric])
    rows, Q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((40, dim)).astype(np.float32)
    sets, ids = ge.edge_sets(rng, n), np.arange(n, dtype=np.uint64)
    ix = fm.half_index(metric, prec, ids, rows)
    try:
        for name in ("65", "half", "not10pct"):
            given, negate, sel = sets[name]
            with ix.create_filter(ids[given], negate=negate) as flt:
                for nq in (17, 40):
                    gi, gs, gc = hg.gathered(ix, Q[:nq], 10, flt, prec)
                    hp.check(metric, prec, rows[sel], Q[:nq], 10, fm.positions(sel, gi, gc), gs, gc, [0, 15, 16, nq - 1])
    finally:
        ix.close()


# ---- d. special values (half tier) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 20, 130])
def test_f16_conversion_observed_through_the_gathered_tier(gpu_required, nq):
    """tests/test_gpu_half_precision.py::test_f16_conversion_observed_through_the_search on this tier's load path (registers -> LDS ->
    fragment): every score is np.float16(probe) bit for bit — subnormal INPUTS kept, overflow to inf — under every row and every second row."""
    (case,) = ge.cases("probes")
    d = ge.data(case)
    want = d.extra["want"]
    ix = index(case.tier, d.ids, d.rows)
    try:
        for name in case.sets:
            sel = d.sets[name][2]
            k = len(sel)
            with ix.create_filter(d.ids[sel]) as flt:
                gi, gs, gc = both(case.tier, ix, d.Q[:nq], k, flt, (name, nq))
            assert np.all(gc == k)
            for qi in (0, nq // 2, nq - 1):
                got = np.full(case.n, np.nan, np.float32)
                got[gi[qi].astype(np.int64)] = gs[qi]
                bad = np.flatnonzero(got[sel].view(np.uint32) != want[sel].view(np.uint32))
                assert bad.size == 0, [(float(d.rows[sel[b], 0]), float(got[sel[b]]), float(want[sel[b]])) for b in bad[:8]]
                assert np.array_equal(gi[qi], sel[hr.topk(want[None, sel], k, True)[0][0].astype(np.int64)].astype(np.uint64))
    finally:
        ix.close()


@pytest.mark.parametrize("tier", [t for t in ge.HALF if t[2] == hr.COSINE])
def test_cosine_of_a_non_zero_norm_below_epsilon_is_zero(gpu_required, tier):
    (case,) = ge.cases("tiny", [tier])
    d = ge.data(case)
    ix = index(tier, d.ids, d.rows)
    try:
        for name in case.sets:
            given, negate, sel = d.sets[name]
            with ix.create_filter(d.ids[given], negate=negate) as flt:
                for nq, k in case.shapes:
                    got = both(tier, ix, d.Q[:nq], k, flt, (tier, name, nq, k))
                    tf.assert_equal(got, ge.expected(tier, d.sc[:nq], d.ids, k, sel), (tier, name, nq, k))
                    if k >= len(sel):                     # the whole list comes back: the planted rows are IN it, at 0.0
                        for qi in (0, ge.TINY_Q[0], nq - 1):
                            for r in ge.TINY_ROWS:
                                (at,) = np.flatnonzero(got[0][qi] == d.ids[r])
                                assert tf.bits(got[1][qi, at:at + 1])[0] == 0, (qi, r)
                    if nq > ge.TINY_Q[1]:                 # the query of that kind: 0.0 against every row, ties by row
                        c = got[2][ge.TINY_Q[1]]
                        assert np.all(tf.bits(got[1][ge.TINY_Q[1], :c]) == 0) and np.array_equal(got[0][ge.TINY_Q[1], :c], d.ids[sel[:c]])
    finally:
        ix.close()


@pytest.mark.parametrize("tier", ge.HALF)
def test_nan_and_inf_rows_and_a_nan_query(gpu_required, tier):
    """Two rows that hold a NaN, one that holds 65 520 (inf in f16), one query that holds a NaN.  What touches no NaN is the reference bit
    for bit: a query's answer without the NaN rows is the reference's top of the list without them.  Where a NaN ranks is the key
    order's business (make_key: f32 total order): ids, counts and NaN positions must be those of mask substitution."""
    (case,) = ge.cases("nan", [tier])
    d = ge.data(case)
    out = d.ids[list(ge.nan_rows_of(tier))]
    ix = index(tier, d.ids, d.rows)
    try:
        for name in case.sets:
            given, negate, sel = d.sets[name]
            clean = np.setdiff1d(sel, ge.nan_rows_of(tier))
            with ix.create_filter(d.ids[given], negate=negate) as flt:
                for nq, k in case.shapes:
                    got = gathered(tier, ix, d.Q[:nq], k, flt)
                    same(got, masked(tier, ix, d.Q[:nq], k, flt), (tier, name, nq, k), nan_payload_free=True)
                    exp = ge.expected(tier, d.sc[:nq], d.ids, k, clean)
                    assert np.all(got[2] == min(k, len(sel)))
                    for qi in range(nq):
                        if qi == ge.NAN_Q:
                            assert np.all(np.isnan(got[1][qi, :got[2][qi]]))
                            continue
                        keep = ~np.isin(got[0][qi, :got[2][qi]], out)
                        gi, gs = got[0][qi, :got[2][qi]][keep], got[1][qi, :got[2][qi]][keep]
                        assert len(gi) >= got[2][qi] - len(out) and not np.isnan(gs).any(), (name, qi)
                        assert np.array_equal(gi, exp[qi][0][:len(gi)]) and np.array_equal(tf.bits(gs), tf.bits(exp[qi][1][:len(gi)])), (name, nq, k, qi)
    finally:
        ix.close()


# ---- e. rows inserted after the filter was made ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_rows_appended_after_the_filter_was_made_are_absent(gpu_required, tier):
    """A plain and a negated filter over 600 rows, then 70 more rows (three of them copies of queries: the best row there is): both
    tiers still answer over the ORIGINAL selection, as mask substitution does — and the images of the old rows survive the append."""
    (case,) = ge.cases("appended", [tier])
    d = ge.data(case)
    n0 = d.extra["n0"]
    ix = index(tier, d.ids[:n0], d.rows[:n0])
    try:
        flts = {name: ix.create_filter(d.ids[d.sets[name][0]], negate=d.sets[name][1]) for name in case.sets}
        before = {name: gathered(tier, ix, d.Q, 10, flts[name]) for name in case.sets}
        assert ix.upload(d.ids[n0:], d.rows[n0:]) == 70
        for name in case.sets:
            sel = d.sets[name][2]
            for nq, k in case.shapes:
                got = both(tier, ix, d.Q[:nq], k, flts[name], (tier, name, nq, k))
                tf.assert_equal(got, ge.expected(tier, d.sc[:nq], d.ids, k, sel), (tier, name, nq, k))
                assert not np.isin(got[0], d.ids[n0:]).any()
            same(gathered(tier, ix, d.Q, 10, flts[name]), before[name], (tier, name, "before / after"))
        with ix.create_filter(d.ids[n0:]) as late:          # ... and a filter made NOW holds them
            got = both(tier, ix, d.Q, 10, late, (tier, "late"))
            tf.assert_equal(got, ge.expected(tier, d.sc, d.ids, 10, np.arange(n0, n0 + 70, dtype=np.int64)), (tier, "late"))
        for f in flts.values():
            f.close()
    finally:
        ix.close()


# ---- f. dead tiles ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_whole_tiles_of_dead_rows_and_a_list_without_a_live_row(gpu_required, tier):
    (case,) = ge.cases("dead", [tier])
    d = ge.data(case)
    sel = d.sets["200"][2]
    ix = index(tier, d.ids, d.rows)
    try:
        with ix.create_filter(d.ids[sel]) as flt:
            dead = np.concatenate([sel[64:128], sel[192:]])           # a whole tile and the whole tail tile
            assert all(ix.remove(int(d.ids[r])) for r in dead)
            left = np.setdiff1d(sel, dead)
            assert len(left) == 128
            for nq, k in case.shapes + [(130, 150)]:                  # (k above the live rows: counts of 128)
                got = both(tier, ix, d.Q[:nq], k, flt, (tier, nq, k))
                tf.assert_equal(got, ge.expected(tier, d.sc[:nq], d.ids, k, left), (tier, nq, k))
            assert all(ix.remove(int(d.ids[r])) for r in left)
            for nq, k in case.shapes:
                got = both(tier, ix, d.Q[:nq], k, flt, (tier, nq, k, "empty"))
                assert np.all(got[2] == 0) and got[2].shape == (nq,)
    finally:
        ix.close()
