"""GPU parity tests of the features merged after tests/test_gpu_large_dim.py — filtered exact search, half-precision rows, the
half-precision and filtered graph walks, per-query filters — at the dims that file covers for the plain exact path: 256 / 512 /
1 024 (the register-chunk instances CPL 1 / 2 / 4, which no test of those features reaches: theirs stop at CPL 3 = 768) and
1 536 ... 4 096 (+ 4 095 / 4 099), where every LDS budget that depends on dim changes the plan:

  A  filtered exact search: the listed sweep's query tile forced down by dim (mode C: B 8 -> 4 -> 1 by the 60 KiB window; mode M:
     16 -> 8 queries per pass by 160 KiB, so 17 queries make passes of 8 + 8 + 1), the mode-M body's `e0 + 4 > dim` tail at dim
     2 047 (dim % 4 != 0 and still mode M: dim_pad 2 048; 4 095 is mode C, where the mode-C body's predicated tail runs), and
     mask substitution over the exact kernels' shrinking tile;
  B  mask substitution through the selection stage's large-dim routes (WIDE + gathered pass at dim 2 048, the vector-ALU tile at 4 096);
  C  half-precision exact search: the f16 / bf16 Euclidean sweep above the 64 KiB LDS window (B 16 -> 4 -> 1, refused past 160 KiB),
     the f16 matrix-core tiers above dim 768;
  D  graph walks with the query in LDS scratch (half walk, filtered walk, rank kernel, per-query ladder, f32 walk).

Nothing here is a new reference: the oracle (oracle.pyoracle), tests/half_ref.py, tests/half_walk_ref.py, tests/filtered_walk_ref.py
and the helpers of the tests of each feature, imported.  The bars are those files' bars: bit equality everywhere except the
half-precision exact search on N(0,1) data (TOL = 1e-5 of tests/test_gpu_half_precision.py, justified there).  Every section asserts
WHICH kernel, level or route served a call, and the arithmetic mode against a table written out below."""
import numpy as np
import pytest

import filtered_walk_ref as fw
import half_ref as hr
import half_walk_ref as hw
import test_gpu_filtered as gf
import test_gpu_filtered_graph as fg
import test_gpu_filters_graph as fgs
import test_gpu_half_precision as hp
import test_gpu_hnsw_half as gh
import test_gpu_large_dim as ld
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP = va.DistanceMetric, va.VectorPrecision
FLOATS = [DM.Cosine, DM.DotProduct, DM.Euclidean]
NQ = hw.NQ
UNSUPPORTED, HIP_ERROR = va._ffi.VDB_ERR_UNSUPPORTED, va._ffi.VDB_ERR_HIP


# ================================================================================================ A. filtered exact search
# (2 047: the one shape with dim % 4 != 0 that Cosine / DotProduct answer in mode M — sweep_topk_listed_m's zero-padded last chunk)
A_SHAPES = [(3000, 256), (3000, 512), (2500, 1024), (2000, 1536), (2000, 2048), (2000, 2047), (1500, 2432), (1500, 3072), (1200, 4096),
            (1200, 4095)]
A_NQ_K = [(1, 10), (8, 10), (17, 5), (5, 200), (70, 10)]   # 17: passes of 8 + 8 + 1 where 8 queries fit a pass; 70: several passes of 16
A_SETS = ("one", "k", "1pct", "half", "not10pct")
ROUTES = {"listed": va.FILTER_ROUTE_LISTED, "mask": va.FILTER_ROUTE_MASK, "auto": va.FILTER_ROUTE_AUTO}


def expected_mode(metric, dim, k, engine=1):
    """The oracle mode of VDB_SEARCH_BRUTE, written out (tests/test_gpu_large_dim.py's docstring): M for Cosine / DotProduct with the
    engine on while the matrix-core exact kernel's 16-query tile (8 KiB per 128 elements + 128 B per k + 192 B) fits 160 KiB — every
    k of this file up to dim 2 048, k <= 62 at dim 2 432, never from dim 2 560 (4 095 pads to 4 096) — and C otherwise."""
    if metric == DM.Euclidean or not engine:
        return "C"
    return "M" if dim <= 2048 or (dim == 2432 and k <= 62) else "C"


def handle(dim, metric, n):
    """a handle sized to its corpus (the default capacity of 100 000 rows is gigabytes of row storage at these dims)"""
    return va.HnswIndex(dim, metric, va.HnswParams(16, 100, n))


_A_CASES = {}


def a_case(metric, n, dim):
    """rows, ids, sets, queries of one (metric, shape), and the oracle's answers as they are asked for: built once, never changed"""
    key = (int(metric), n, dim)
    if key not in _A_CASES:
        rng = np.random.default_rng(1000 * n + dim + int(metric))
        rows, ids = gf.rand_rows(rng, n, dim, metric), gf.ext_ids(n)
        sets = {name: s for name, s in gf.allowed_sets(rng, n).items() if name in A_SETS}
        qs = {(nq, k): gf.rand_rows(rng, nq, dim, metric) for nq, k in A_NQ_K}
        _A_CASES[key] = dict(metric=metric, rows=rows, ids=ids, sets=sets, qs=qs, exp={})
    return _A_CASES[key]


def a_expected(c, name, nq, k, mode_name, sel=None):
    key = (name, nq, k, mode_name, None if sel is None else sel.tobytes())
    if key not in c["exp"]:
        mode = po.MODE_M if mode_name == "M" else po.MODE_C
        c["exp"][key] = gf.oracle_subset(c["metric"], c["rows"], c["ids"], c["qs"][(nq, k)], k, c["sets"][name][2] if sel is None else sel, mode)
    return c["exp"][key]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_case_cache_with_the_module():
    """the four test functions of section A share one case per (metric, shape) — about 0.4 GB of rows in all — until the file is done"""
    yield
    _A_CASES.clear()


def mode_name_of(ix, metric, dim, k, engine=1):
    got = ix.sweep_arith_mode(k)
    assert got == expected_mode(metric, dim, k, engine), (str(metric), dim, k, got)
    return got


def run_a(metric, n, dim, route, want_listed, engine=1):
    ix = handle(dim, metric, n)
    try:
        c = a_case(metric, n, dim)
        assert ix.upload(c["ids"], c["rows"]) == n
        ix.set_option(va.OPT_FILTER_ROUTE, route)
        for name, (given, negate, sel) in c["sets"].items():
            with ix.create_filter(c["ids"][given], negate=negate) as flt:
                assert flt.matched == len(sel), name
                for nq, k in A_NQ_K:
                    mode_name = mode_name_of(ix, metric, dim, k, engine)
                    got = ix.search_batch_brute_force_filtered(c["qs"][(nq, k)], k, flt)
                    listed = bool(ix.last_kernels() & va.KERNEL_SWEEP_LISTED)
                    assert listed == want_listed, (name, nq, k, hex(ix.last_kernels()))
                    gf.assert_equal(got, a_expected(c, name, nq, k, mode_name), (str(metric), n, dim, name, nq, k, route, mode_name))
    finally:
        ix.close()


@pytest.mark.parametrize("n,dim", A_SHAPES)
@pytest.mark.parametrize("metric", FLOATS)
def test_filtered_listed_route_at_large_dims(gpu_required, metric, n, dim):
    run_a(metric, n, dim, va.FILTER_ROUTE_LISTED, want_listed=True)


@pytest.mark.parametrize("n,dim", [s for s in A_SHAPES if s[1] in (256, 512, 1024, 4096)])
def test_filtered_listed_route_cosine_mode_c_body_at_large_dims(gpu_required, n, dim):
    """engine 0: the mode-C listed body (the register-chunk instances, the LDS query scratch) serves a dot metric too"""
    va.set_sweep_engine(0)
    try:
        run_a(DM.Cosine, n, dim, va.FILTER_ROUTE_LISTED, want_listed=True, engine=0)
    finally:
        va.set_sweep_engine(1)


@pytest.mark.parametrize("n,dim", A_SHAPES)
@pytest.mark.parametrize("metric", FLOATS)
def test_filtered_mask_route_at_large_dims(gpu_required, metric, n, dim):
    run_a(metric, n, dim, va.FILTER_ROUTE_MASK, want_listed=False)


@pytest.mark.parametrize("n,dim", A_SHAPES)
@pytest.mark.parametrize("metric", FLOATS)
def test_filtered_routes_agree_at_large_dims(gpu_required, metric, n, dim):
    """AUTO gives what both forced routes give — and what the oracle gives"""
    ix = handle(dim, metric, n)
    try:
        c = a_case(metric, n, dim)
        ix.upload(c["ids"], c["rows"])
        for name in ("1pct", "half", "not10pct"):
            given, negate, _ = c["sets"][name]
            with ix.create_filter(c["ids"][given], negate=negate) as flt:
                for nq, k in ((1, 10), (17, 5), (70, 10)):
                    res = []
                    for route in (va.FILTER_ROUTE_AUTO, va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK):
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        res.append(ix.search_batch_brute_force_filtered(c["qs"][(nq, k)], k, flt))
                    for other in res[1:]:
                        assert np.array_equal(res[0][2], other[2])
                        assert np.array_equal(res[0][0], other[0]) and np.array_equal(gf.bits(res[0][1]), gf.bits(other[1])), (name, nq, k)
                    gf.assert_equal(res[0], a_expected(c, name, nq, k, mode_name_of(ix, metric, dim, k)), (name, nq, k))
    finally:
        ix.close()


@pytest.mark.parametrize("n,dim", [s for s in A_SHAPES if s[1] in (1536, 4096)])
@pytest.mark.parametrize("metric", FLOATS)
def test_filtered_rows_removed_after_the_filter_drop_out_at_large_dims(gpu_required, metric, n, dim):
    """three listed rows soft-deleted after create_filter: the `alive` read where a key would enter a list (listed route), the mask
    AND alive (mask substitution)"""
    ix = handle(dim, metric, n)
    try:
        c = a_case(metric, n, dim)
        ix.upload(c["ids"], c["rows"])
        given, negate, sel = c["sets"]["1pct"]
        with ix.create_filter(c["ids"][given], negate=negate) as flt:
            gone = sel[[1, len(sel) // 2, len(sel) - 1]]
            for r in gone:
                assert ix.remove(int(c["ids"][r]))
            left = np.setdiff1d(sel, gone)
            for rname, route in ROUTES.items():
                ix.set_option(va.OPT_FILTER_ROUTE, route)
                for nq, k in ((8, 10), (17, 5), (5, 200)):
                    got = ix.search_batch_brute_force_filtered(c["qs"][(nq, k)], k, flt)
                    if rname != "auto":
                        assert bool(ix.last_kernels() & va.KERNEL_SWEEP_LISTED) == (rname == "listed"), (rname, hex(ix.last_kernels()))
                    want = a_expected(c, "1pct", nq, k, mode_name_of(ix, metric, dim, k), sel=left)
                    gf.assert_equal(got, want, (str(metric), dim, rname, nq, k))
                    assert not set(c["ids"][gone].tolist()) & set(got[0][got[0] != np.uint64(0xFFFFFFFFFFFFFFFF)].tolist())
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [DM.Euclidean, DM.Cosine])
def test_filtered_beyond_every_lds_plan(gpu_required, metric):
    """dim 16 384 (the reference allows up to 65 536): no listed plan exists (one query is 64 KiB, above the listed sweep's 60 KiB
    window), so every route ends in the unfiltered exact path — the call does what search_batch_brute_force does at that dim: the
    oracle's bits, or VDB_ERR_UNSUPPORTED.  Never a launch failure, never another answer."""
    n, dim, k, nq = 64, 16384, 10, 8
    rng = np.random.default_rng(16384 + int(metric))
    rows, ids, Q = gf.rand_rows(rng, n, dim, metric), gf.ext_ids(n), gf.rand_rows(rng, nq, dim, metric)
    ix = handle(dim, metric, n)
    try:
        ix.upload(ids, rows)
        assert ix.sweep_arith_mode(k) == "C"

        def outcome(fn):
            try:
                return fn(), None
            except va.VelesHipError as e:
                assert e.code != HIP_ERROR, str(e)
                return None, e.code

        base, base_err = outcome(lambda: ix.search_batch_brute_force(Q, k))
        assert base_err in (None, UNSUPPORTED), base_err
        print(f"{metric} dim {dim}: search_batch_brute_force -> {'results' if base_err is None else base_err}")
        if base_err is None:
            gf.assert_equal(base, gf.oracle_subset(metric, rows, ids, Q, k, np.arange(n), po.MODE_C), "unfiltered")
        sets = {"all": np.arange(n), "half": np.sort(rng.choice(n, n // 2, replace=False)), "k-1": np.sort(rng.choice(n, k - 1, replace=False))}
        for rname, route in ROUTES.items():
            ix.set_option(va.OPT_FILTER_ROUTE, route)
            for name, sel in sets.items():
                with ix.create_filter(ids[sel]) as flt:
                    got, err = outcome(lambda: ix.search_batch_brute_force_filtered(Q, k, flt))
                    assert err == base_err, (rname, name, err, base_err)
                    if err is None:
                        assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                        gf.assert_equal(got, gf.oracle_subset(metric, rows, ids, Q, k, sel, po.MODE_C), (str(metric), rname, name))
    finally:
        ix.close()


# ================================================================================================ B. mask substitution, selection routes
@pytest.mark.parametrize("metric,dim", [(DM.Cosine, 2048), (DM.Euclidean, 2048), (DM.Cosine, 4096)])
def test_mask_substitution_through_the_large_dim_selection_routes(gpu_required, metric, dim):
    """tests/test_gpu_filtered.py::test_mask_route_through_the_selection_stage on the embedding-like corpus of tests/test_gpu_large_dim.py:
    dim 2 048 — WIDE + the gathered pass (Cosine), the augmented form (Euclidean), level 4; dim 4 096 Cosine — level 0, the exact
    vector-ALU kernels' shrunk tile, under a mask.  The "half" filter stays on the unfiltered call's level; below 1/16 allowed a
    filtered call leaves the selection stage by design."""
    rows, qs0 = ld.dense(dim)
    n, Q = rows.shape[0], qs0[:64]
    ids = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(77 + dim + int(metric))
    sets = {"half": np.sort(rng.choice(n, size=n // 2, replace=False)), "1/64": np.arange(5, n, 64), "7rows": np.sort(rng.choice(n, size=7, replace=False))}
    subset = {}   # (set, mode) -> the oracle's top-50 over the subset: a prefix serves k = 10 (the order is total)
    ix = ld.new_index(dim, metric, rows)
    try:
        ix.set_option(va.OPT_FILTER_ROUTE, va.FILTER_ROUTE_MASK)
        for k in (10, 50):
            level, mode = ld.expected_level(metric, dim, k), ld.mode_of(ix, metric, k)
            assert ix.sweep_arith_mode(k) == expected_mode(metric, dim, k)
            before = ld.check(ix, metric, rows, Q, k, ("dense", dim), level)          # level and oracle bits of the unfiltered call
            for name, sel in sets.items():
                if (name, mode) not in subset:
                    subset[(name, mode)] = gf.oracle_subset(metric, rows, ids, Q, 50, sel, mode)
                want = [(i[:k], s[:k]) for i, s in subset[(name, mode)]]
                with ix.create_filter(ids[sel]) as flt:
                    got = ix.search_batch_brute_force_filtered(Q, k, flt)
                    assert not ix.last_kernels() & va.KERNEL_SWEEP_LISTED
                    if name == "half":
                        assert ix.last_select_level() == level, (name, k, ix.last_select_level(), level)
                        if level == 0:    # (level 0 alone cannot tell the exact kernels from a call that left the stage: name the kernel)
                            assert ix.last_kernels() & va.KERNEL_SWEEP_VALU, hex(ix.last_kernels())
                    gf.assert_equal(got, want, (str(metric), dim, name, k))
            after = ld.check(ix, metric, rows, Q, k, ("dense", dim), level)           # a filtered call moved nothing
            assert np.array_equal(before[0], after[0]) and np.array_equal(ld.bits(before[1]), ld.bits(after[1]))
    finally:
        ix.close()
        for key in [key for key in ld._oracle if key[1] == ("dense", dim) and key[3] == 64]:
            del ld._oracle[key]


# ================================================================================================ C. half-precision exact search
C_SHAPES = [(2000, 1024), (1500, 1536), (1200, 2560), (1000, 4096), (1000, 4095)]
C_BATCHES = [(1, 10), (3, 64), (20, 10), (70, 5), (300, 10)]


def half_parity_case(prec, metric, n, dim):
    """tests/test_gpu_half_precision.py::test_half_precision_parity at another shape: its check (TOL = 1e-5), its kernel-mask rule"""
    rng = np.random.default_rng(n + dim + 17 * prec + metric)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    qsets = [rng.standard_normal((nq, dim)).astype(np.float32) for nq, _ in C_BATCHES]
    if metric == hr.EUCLIDEAN:      # near duplicates of four queries (1e-2 noise) and one row EQUAL to a query (distance exactly 0)
        q = qsets[-1]
        spots = rng.choice(n, 5, replace=False)
        rows[spots[:4]] = q[[0, 7, 150, 299]] + 1e-2 * rng.standard_normal((4, dim)).astype(np.float32)
        rows[spots[4]] = q[33]
    ix = handle(dim, hp.METRIC[metric], n)
    try:
        ix.upload(np.arange(n // 2), rows[: n // 2])
        ix.enable_half_precision(VP.F16 if prec == hr.F16 else VP.BF16)        # converts what is there ...
        ix.upload(np.arange(n // 2, n), rows[n // 2:])                          # ... and what arrives later
        for (nq, k), qs in zip(C_BATCHES, qsets):
            gi, gs, gc = hp.search(ix, qs, k, prec)
            hp.served_by(ix, hp.tier_bits(metric, prec, nq, n, dim, k))
            if metric != hr.EUCLIDEAN:                                          # exactly the tier: no other half kernel took part of the batch
                others = (va.KERNEL_GEMM_BF16 | va.KERNEL_GEMM_BF16_GLDS | va.KERNEL_SWEEP_MFMA_BF16 | va.KERNEL_SWEEP_HALF_L2) & ~hp.tier_bits(metric, prec, nq, n, dim, k)
                assert not ix.last_kernels() & others, hex(ix.last_kernels())
            hp.check(metric, prec, rows, qs, k, gi, gs, gc)
            if metric == hr.EUCLIDEAN and nq == 300:
                assert gs[33, 0] == 0.0 and gi[33, 0] == spots[4]
                for j, qi in enumerate([0, 7, 150, 299]):
                    assert gi[qi, 0] == spots[j]
    finally:
        ix.close()


@pytest.mark.parametrize("n,dim", C_SHAPES)
@pytest.mark.parametrize("prec,metric", hp.PARITY)
def test_half_precision_parity_at_large_dims(gpu_required, prec, metric, n, dim):
    """Euclidean: the LDS tile of 16 queries passes the default 64 KiB window at dim 1 024 and 1 536, drops to 4 queries from dim
    2 560 (40 KiB at 2 560, 64 KiB + lists at 4 096: the opt-in again).  Cosine / DotProduct: the f16 streaming kernel's tile
    shrinks with dim (6 -> 1 sixteen-query groups), the GEMM tiers take >= 64 queries where dim % 64 == 0 — not at 4 095."""
    half_parity_case(prec, metric, n, dim)


@pytest.mark.parametrize("prec", [hr.F16, hr.BF16])
def test_half_precision_euclidean_one_query_tile(gpu_required, prec):
    """dim 10 248: four queries are 160 KiB + lists — the sweep runs one query per pass (40 KiB)"""
    half_parity_case(prec, hr.EUCLIDEAN, 300, 10248)


@pytest.mark.parametrize("prec", [hr.F16, hr.BF16])
def test_half_precision_euclidean_bit_equal_at_dim_4096(gpu_required, prec):
    """Values on which every difference, square and partial sum of a 4 096-term squared distance is exact in f32, so every order of
    summation gives the reference's bits.  F16: 1 + j / 512, -15 <= j <= 16 (ten significant bits: f16 holds them, bf16 does not);
    differences are <= 31 units of 2^-9, sums <= 4 096 * 31^2 < 2^22 units of 2^-18.  BF16: integers |m| <= 31, sums <= 4 096 *
    62^2 < 2^24.  The bounds are asserted below, in integers."""
    dim, n = 4096, 1000
    rng = np.random.default_rng(4096 + prec)
    if prec == hr.F16:
        def make(shape):
            return ((512 + rng.integers(-15, 17, shape)) / 512.0).astype(np.float32)
        unit = 512
    else:
        def make(shape):
            return rng.integers(-31, 32, shape).astype(np.float32)
        unit = 1
    rows = make((n, dim))
    rows[[256, 257, 900]] = rows[[1, 1, 1]]          # exact ties, by row
    qsets = [make((nq, dim)) for nq in (1, 3, 20)]
    qsets[2][0] = rows[1]                            # distance exactly 0, three times
    u = np.rint(rows.astype(np.float64) * unit).astype(np.int64)
    assert np.array_equal(u / unit, rows) and np.array_equal(hr.round_half(rows, prec), rows)          # representable
    if prec == hr.F16:
        assert not np.array_equal(hr.round_half(rows, hr.BF16), rows)
    for qs in qsets:
        uq = np.rint(qs.astype(np.float64) * unit).astype(np.int64)
        assert np.array_equal(uq / unit, qs)
        span = max(int(u.max()), int(uq.max())) - min(int(u.min()), int(uq.min()))
        assert dim * span * span < 2 ** 24                                                              # every partial sum, whatever the order
    ix = handle(dim, DM.Euclidean, n)
    try:
        ix.upload(np.arange(n), rows)
        ix.enable_half_precision(VP.F16 if prec == hr.F16 else VP.BF16)
        for qs in qsets:
            gi = hp.assert_bits(ix, hr.EUCLIDEAN, prec, rows, qs, 10)
            hp.served_by(ix, va.KERNEL_SWEEP_HALF_L2, va.KERNEL_F16)
        assert gi[0, :4].tolist() == [1, 256, 257, 900]
        dead = [1, 257]
        for d in dead:
            assert ix.remove(d)
        alive = np.ones(n, bool)
        alive[dead] = False
        hp.assert_bits(ix, hr.EUCLIDEAN, prec, rows, qsets[2], 10, alive)
    finally:
        ix.close()


def test_half_precision_euclidean_refused_beyond_the_lds(gpu_required):
    """dim 40 960: one query is 160 KiB + its list — VDB_ERR_UNSUPPORTED with the sweep's own message, not a launch failure"""
    n, dim = 64, 40960
    rng = np.random.default_rng(40960)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    ix = handle(dim, DM.Euclidean, n)
    try:
        ix.upload(np.arange(n), rows)
        ix.enable_half_precision(VP.F16)
        with pytest.raises(va.VelesHipError) as e:
            hp.search(ix, rows[:3], 10, hr.F16)
        assert e.value.code == UNSUPPORTED and "half-precision Euclidean sweep" in str(e.value), (e.value.code, str(e.value))
    finally:
        ix.close()


# ================================================================================================ D. graph walks
@pytest.fixture(scope="module")
def half_worlds(tmp_path_factory):
    """tests/test_gpu_hnsw_half.py's World: one oracle graph and one handle per (metric, shape)"""
    root, cache = str(tmp_path_factory.mktemp("large_half_walk")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = gh.World(root, metric, shape)
        return cache[(metric, shape)]
    get.root = root
    yield get
    for w in cache.values():
        w.ix.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    """tests/test_gpu_filtered_graph.py's World (+ the "no filter" filter of tests/test_gpu_filters_graph.py)"""
    root, cache = str(tmp_path_factory.mktemp("large_filtered_graph")), {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = fg.World(root, metric, shape)
        return cache[(metric, shape)]
    yield get
    for w in cache.values():
        if getattr(w, "none", None) is not None:
            w.none.close()
        w.close()


# ---- the half walk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", gh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
@pytest.mark.parametrize("metric", [hr.DOT, hr.EUCLIDEAN])
def test_half_walk_at_the_large_shapes(gpu_required, half_worlds, metric, shape, precision):
    """ids, score bits and counters of the oracle's mode-C walk over the rounded vectors (ef 300: the LDS list)"""
    w = half_worlds(metric, shape)
    _, g_half = w.patched(precision)
    qr = hr.round_half(w.qs, precision)
    for k, ef in hw.KEF:
        res, stats, kern = w.answers(precision, k, ef)
        oid, obits, ostats = hw.oracle_walk(g_half, metric, qr, k, ef)
        gh.assert_same(res, oid, obits, (k, ef))
        assert stats == ostats, (k, ef, stats, ostats)
        assert kern & va.KERNEL_HNSW_HALF and not kern & (va.KERNEL_HNSW | va.KERNEL_HNSW_INT8), hex(kern)
        assert bool(kern & va.KERNEL_F16) == (precision == hr.F16), hex(kern)


def exact_grid(rng, shape, precision):
    """half_walk_ref.grid with the f16 amplitude cut for dims up to 4 099: m / 256 with |m| <= 16 and at most 8 elements per row of
    +-(1 + 1/256) — sums stay below 4 099 * 16^2 + 8 * 257^2 < 2^21 units of 2^-16.  BF16: its integers |m| <= 15 (4 099 * 225 < 2^20)."""
    if precision == hr.BF16:
        return hw.grid(rng, shape, precision)
    x = rng.integers(-16, 17, shape).astype(np.float32) / np.float32(256)
    special = rng.random(shape) < 0.0015
    special &= ~(np.cumsum(special, axis=-1) > 8)
    sign = np.where(rng.random(shape) < 0.5, np.float32(-1), np.float32(1))
    return np.where(special, sign * np.float32(1 + 1 / 256), x).astype(np.float32)


@pytest.mark.parametrize("precision", gh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
def test_half_walk_cosine_bit_exact_on_exact_data_at_the_large_shapes(gpu_required, half_worlds, shape, precision):
    n, dim, M, efc = shape
    rng = np.random.default_rng(50 + n + dim + precision)
    rows, qs = exact_grid(rng, (n, dim), precision), exact_grid(rng, (NQ, dim), precision)
    unit = 256 if precision == hr.F16 else 1
    ur, uq = np.abs(np.rint(rows.astype(np.float64) * unit)).astype(np.int64), np.abs(np.rint(qs.astype(np.float64) * unit)).astype(np.int64)
    assert np.array_equal(hr.round_half(rows, precision), rows) and np.array_equal(hr.round_half(qs, precision), qs)
    assert max(int((ur * ur).sum(1).max()), int((uq * uq).sum(1).max()), int((uq @ ur.T).max())) < 2 ** 24   # norms and every |partial dot|
    w = gh.World(half_worlds.root, hr.COSINE, shape, rows, qs, tag=f"grid{precision}")      # (its own handle, as the small-dim test)
    try:
        for k, ef in hw.KEF:
            res, stats, kern = w.answers(precision, k, ef)
            oid, obits, ostats = hw.oracle_walk(w.g, hr.COSINE, qs, k, ef)
            gh.assert_same(res, oid, obits, (k, ef))
            assert stats == ostats, (k, ef, stats, ostats)
            assert kern & va.KERNEL_HNSW_HALF and bool(kern & va.KERNEL_F16) == (precision == hr.F16), hex(kern)
    finally:
        w.ix.close()


@pytest.mark.parametrize("precision", gh.PRECISIONS)
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
def test_half_walk_cosine_within_tolerance_at_the_large_shapes(gpu_required, half_worlds, shape, precision):
    w = half_worlds(hr.COSINE, shape)
    full, _ = hr.truth64(hr.COSINE, precision, w.rows, w.qs)          # f64 cosine of the ROUNDED values
    for k, ef in hw.KEF:
        res, _, kern = w.answers(precision, k, ef)
        assert kern & va.KERNEL_HNSW_HALF and bool(kern & va.KERNEL_F16) == (precision == hr.F16), hex(kern)
        worst = 0.0
        for qi, one in enumerate(res):
            assert len(one) == k and len({i for i, _ in one}) == k
            for i, s in one:
                worst = max(worst, abs(s - min(max(full[qi, i], 0.0), 1.0)))     # transform_score clamps 1 - d to [0, 1]
        print(f"cosine n01 shape {shape} precision {precision} k {k} ef {ef}: worst |score - f64| {worst:.3g}")
        assert worst <= hp.TOL, (k, ef, worst)


# ---- the f32 walk (the one test of this file that tests/test_gpu_switches.py runs again under the latency-mode switches) ---------------
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_f32_walk_at_the_large_shapes(gpu_required, worlds, metric, shape):
    w = worlds(metric, shape)
    for k, ef in hw.KEF:
        ids, sc, cnt = w.ix._search_raw(w.qs, k, ef, va.MODE_HNSW)
        stats, kern = w.ix.last_search_stats(), w.ix.last_kernels()
        assert kern & va.KERNEL_HNSW and not kern & (va.KERNEL_HNSW_HALF | va.KERNEL_HNSW_INT8 | va.KERNEL_HNSW_FILTERED), hex(kern)
        oid, obits, ostats = hw.oracle_walk(w.g, metric, w.qs, k, ef)
        assert stats == ostats, (k, ef, stats, ostats)
        for qi in range(NQ):
            c = int(cnt[qi])
            assert ids[qi, :c].tolist() == oid[qi], (k, ef, qi)
            assert np.array_equal(sc[qi, :c].view(np.uint32), obits[qi]), (k, ef, qi)


# ---- the filtered walk and the exact pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_all_allowed_filter_is_the_unfiltered_walk_at_the_large_shapes(gpu_required, worlds, metric, shape):
    w = worlds(metric, shape)
    for k, ef in hw.KEF:
        (ids, sc, cnt), routes, stats = fg.run(w, "all", k, ef, va.ROUTE_WALK)
        kern = w.ix.last_kernels()
        assert kern & va.KERNEL_HNSW_FILTERED and not kern & (va.KERNEL_HNSW | va.KERNEL_FILTER_RANK), hex(kern)
        assert np.all(routes == 1)
        oid, obits, ostats = hw.oracle_walk(w.g, metric, w.qs, k, ef)
        assert stats == ostats, (k, ef, stats, ostats)
        for qi in range(NQ):
            c = int(cnt[qi])
            assert ids[qi, :c].tolist() == oid[qi], (k, ef, qi)
            assert np.array_equal(sc[qi, :c].view(np.uint32), obits[qi]), (k, ef, qi)


@pytest.mark.parametrize("name", ["half", "tenth", "clustered"])
@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_filtered_walk_equals_the_single_list_reference_at_the_large_shapes(gpu_required, worlds, metric, shape, name):
    w, k, ef = worlds(metric, shape), 10, 64
    allowed = w.filters[name]
    want = fg.expect_call(w, allowed, k, ef, va.ROUTE_WALK)
    assert want[2] == [1] * NQ, "the reference itself overflows at this shape"
    got = fg.run(w, name, k, ef, va.ROUTE_WALK)
    kern = w.ix.last_kernels()
    assert kern & va.KERNEL_HNSW_FILTERED and not kern & (va.KERNEL_HNSW | va.KERNEL_FILTER_RANK), hex(kern)
    fg.assert_call(got, want, (metric, shape, name))
    assert all(allowed[i] for row, c in zip(got[0][0], got[0][2]) for i in row[:int(c)])


@pytest.mark.parametrize("shape", hw.LARGE_SHAPES)
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_filtered_graph_routes_at_the_large_shapes(gpu_required, worlds, metric, shape):
    w, k, ef = worlds(metric, shape), 10, 64
    few = w.filters["few"]
    assert int(few.sum()) < ef
    # auto: the walk could never fill its result set -> the exact pass (the rank kernel) for every query
    got = fg.run(w, "few", k, ef, va.ROUTE_AUTO)
    kern = w.ix.last_kernels()
    assert kern & va.KERNEL_FILTER_RANK and not kern & (va.KERNEL_HNSW_FILTERED | va.KERNEL_HNSW), hex(kern)
    want = fg.expect_call(w, few, k, ef, va.ROUTE_AUTO)
    assert want[2] == [2] * NQ and want[3] == (NQ * int(few.sum()), 0)
    fg.assert_call(got, want, "auto, few")
    # walk: on these small graphs the list holds the component, the walk completes
    got_w = fg.run(w, "few", k, ef, va.ROUTE_WALK)
    kern = w.ix.last_kernels()
    assert kern & va.KERNEL_HNSW_FILTERED and not kern & va.KERNEL_FILTER_RANK, hex(kern)
    want_w = fg.expect_call(w, few, k, ef, va.ROUTE_WALK)
    assert want_w[2] == [1] * NQ, "the reference itself overflows at this shape"
    fg.assert_call(got_w, want_w, "walk, few")
    # exact pass on demand
    got_e = fg.run(w, "half", k, ef, va.ROUTE_EXACT)
    assert w.ix.last_kernels() & va.KERNEL_FILTER_RANK and not w.ix.last_kernels() & va.KERNEL_HNSW_FILTERED
    fg.assert_call(got_e, fg.expect_call(w, w.filters["half"], k, ef, va.ROUTE_EXACT), "exact, half")


# ---- one filter per query -------------------------------------------------------------------------------------------------------------
MIX = [None, "all", "half", "tenth", "few", "empty"]  # None = no filter


@pytest.mark.parametrize("shape", hw.LARGE_SHAPES[2:])
@pytest.mark.parametrize("metric", fg.F32_METRICS)
def test_mixed_filters_in_one_call_at_the_large_shapes(gpu_required, worlds, metric, shape):
    """query i of the mixed call gets what search_batch_filtered_graph returns for it alone (the contract of
    tests/test_gpu_filters_graph.py) — and what tests/filtered_walk_ref.py gives at its own filter's plan, at ef 64 (register list) and
    ef 300 (the LDS list; there "tenth" has fewer rows than ef as well, so the auto rule sends it to the exact pass)"""
    w = worlds(metric, shape)
    if getattr(w, "none", None) is None:
        w.none = w.ix.create_filter(np.empty(0, dtype=np.uint64), negate=True)  # what "no filter" is defined as
        assert w.none.matched == w.n
    assert int(w.filters["few"].sum()) < 64
    names = [MIX[i % len(MIX)] for i in range(NQ)]
    with w.ix.create_filter(np.empty(0, dtype=np.uint64)) as empty:
        assert empty.matched == 0
        given = [None if n is None else (empty if n == "empty" else w.flt(n)) for n in names]
        alone = [w.none if n is None else (empty if n == "empty" else w.flt(n)) for n in names]
        for k, ef in [(10, 64), (10, 300)]:
            got = fgs.batch(w.ix, w.qs, k, given, ef)
            fgs.assert_same(got, fgs.singles(w.ix, w.qs, k, alone, ef), (metric, shape, k, ef))
            (ids, sc, cnt), routes, stats, kern = got
            assert kern & va.KERNEL_HNSW_FILTERED and kern & va.KERNEL_FILTER_RANK and not kern & va.KERNEL_HNSW, hex(kern)
            nd = ne = 0
            for qi, name in enumerate(names):
                c = int(cnt[qi])
                if name == "empty":
                    assert c == 0 and routes[qi] == 0, qi
                    continue
                flt = np.ones(w.n, dtype=bool) if name is None else w.filters[name]
                wi, wb, wr, ws = fg.expect_call(w, flt, k, ef, va.ROUTE_AUTO, qs=w.qs[qi:qi + 1])
                exact = int(flt.sum()) < fw.ef_rule(k, ef)     # the auto rule: the walk could never fill its result set
                assert name != "few" or exact
                assert wr[0] == (2 if exact else 1), (qi, name, "the reference itself overflows at this shape")
                assert int(routes[qi]) == wr[0] and ids[qi, :c].tolist() == wi[0], (qi, name)
                assert np.array_equal(sc[qi, :c].view(np.uint32), wb[0]), (qi, name)
                nd, ne = nd + ws[0], ne + ws[1]
            assert tuple(stats) == (nd, ne), (stats, nd, ne)
