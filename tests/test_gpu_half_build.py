"""GPU tests of graph construction over the half-precision rows (vdb_hip_index_set_graph_precision; csrc/hnsw_build.hip
hnsw_insert_half_kernel / hnsw_ndist_half_kernel).

Bar: with graph precision P the graph is, link for link on every layer and with the same entry point, the oracle's mode-C graph over
round_half(rows, P) — sequential insert and the batch-synchronous build, every dim class, Cosine / Euclidean / DotProduct, f16 and
bf16.  tests/half_build_ref.py holds the shapes and the oracle recipes; tests/test_half_build_cpu.py checks that each case's oracle
graph differs from the one over the f32 rows, so a build that ignored the precision fails here.
"""
import numpy as np
import pytest

import build_shapes as bs
import half_build_ref as hb
import half_ref as hr
import half_walk_ref as hw

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM, VP, SQ = va.DistanceMetric, va.VectorPrecision, va.SearchQuality
METRIC = {"cosine": DM.Cosine, "euclidean": DM.Euclidean, "dot": DM.DotProduct}
HR_METRIC = {"cosine": hr.COSINE, "euclidean": hr.EUCLIDEAN, "dot": hr.DOT}
VPREC = {hr.F32: VP.F32, hr.F16: VP.F16, hr.BF16: VP.BF16}
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -7, -8


def new_index(metric, dim, M, efc, n, precision):
    ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
    if precision != hr.F32:
        ix.enable_half_precision(VPREC[precision])
        ix.set_graph_precision(VPREC[precision])
    assert ix.graph_precision() == VPREC[precision]
    return ix


def build(ix, rows, mode, first_id=0):
    n = rows.shape[0]
    if mode == "sequential":
        for i in range(n):
            ix.insert(first_id + i, rows[i])
    else:
        ix.upload(np.arange(first_id, first_id + n), rows)
        ix.build_graph(hb.MAX_BATCH)


# ---- 1. dim classes x metric x precision, sequential and batched ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", hb.MODES)
@pytest.mark.parametrize("precision", hb.PRECISIONS, ids=lambda p: hb.PNAME[p])
@pytest.mark.parametrize("metric", hb.METRICS)
@pytest.mark.parametrize("shape", hb.SHAPES, ids=lambda s: f"n{s[0]}_d{s[1]}")
def test_half_build_link_for_link(shape, metric, precision, mode):
    n, dim, M, efc = shape
    rows, _ = hb.case_rows(metric, shape)
    g = hb.case_oracle(metric, shape, precision, mode)
    ix = new_index(metric, dim, M, efc, n, precision)
    try:
        build(ix, rows, mode)
        bs.assert_same_graph(g, ix, n)
        assert ix.graph_precision() == VPREC[precision]
    finally:
        ix.close()


# ---- 2. the walk on its own graph -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hb.WALK_CASES, ids=lambda c: f"{c[0]}_d{c[1][1]}_{hb.PNAME[c[2]]}")
def test_half_walk_on_the_half_built_graph_equals_the_oracle(case):
    metric, shape, precision = case
    n, dim, M, efc = shape
    rows, qs = hb.case_rows(metric, shape)
    g = hb.case_oracle(metric, shape, precision, "batched")
    qr = hr.round_half(qs, precision)
    ix = new_index(metric, dim, M, efc, n, precision)
    try:
        build(ix, rows, "batched")
        for k, ef in hw.KEF:
            res = ix.search_batch_half_graph(qs, k, ef, VPREC[precision])
            stats, kern = ix.last_search_stats(), ix.last_kernels()
            oid, obits, ostats = hw.oracle_walk(g, HR_METRIC[metric], qr, k, ef)
            print(f"{case} k {k} ef {ef}: counters gpu {stats} oracle {ostats}")
            assert len(res) == len(oid)
            for qi, one in enumerate(res):
                assert [r[0] for r in one] == oid[qi], (k, ef, qi)
                assert np.array_equal(hw.bits([r[1] for r in one]), obits[qi]), (k, ef, qi)
            assert stats == ostats, (k, ef)
            assert kern & va.KERNEL_HNSW_HALF and bool(kern & va.KERNEL_F16) == (precision == hr.F16), hex(kern)
    finally:
        ix.close()


# ---- 3. switching the precision of a live graph ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hb.SWITCH_CASES, ids=lambda c: f"{c[0]}_{hb.PNAME[c[1]]}_to_{hb.PNAME[c[2]]}")
def test_switching_precision_on_a_live_graph(case, tmp_path):
    metric, before, after = case
    rows, more = hb.switch_data(metric)
    g, pruned, _ = hb.switch_oracle(metric, before, after, tmp_path, live=True)
    assert pruned >= 1
    n = hb.SWITCH_N + hb.SWITCH_MORE
    ix = va.HnswIndex(hb.SWITCH_DIM, METRIC[metric], va.HnswParams(hb.SWITCH_M, hb.SWITCH_EFC, n))
    try:
        ix.enable_half_precision(VPREC[before if before != hr.F32 else after])
        ix.set_graph_precision(VPREC[before])
        build(ix, rows, "sequential")
        ix.set_graph_precision(VPREC[after])           # the cached neighbour distances are refilled in the new precision
        assert ix.graph_precision() == VPREC[after]
        build(ix, more, "sequential", first_id=hb.SWITCH_N)
        bs.assert_same_graph(g, ix, n)
    finally:
        ix.close()


# ---- 4. inserts after load_reference_files, the precision set after the load ----------------------------------------------------------------------
@pytest.mark.parametrize("case", hb.LOAD_CASES, ids=lambda c: f"{c[0]}_{hb.PNAME[c[1]]}")
def test_inserts_after_a_load_at_a_half_precision(case, tmp_path):
    metric, precision = case
    _, more = hb.switch_data(metric)
    g, pruned, dump = hb.switch_oracle(metric, hr.F32, precision, tmp_path, live=False)
    assert pruned >= 1
    n = hb.SWITCH_N + hb.SWITCH_MORE
    ix = va.HnswIndex(hb.SWITCH_DIM, METRIC[metric], va.HnswParams(hb.SWITCH_M, hb.SWITCH_EFC, n))
    try:
        ix.load_reference_files(dump, hb.BASE)          # the f32 rows and the links chosen over them
        assert ix.graph_precision() == VP.F32           # not persisted: a loaded handle starts at F32
        ix.enable_half_precision(VPREC[precision])
        ix.set_graph_precision(VPREC[precision])
        build(ix, more, "sequential", first_id=hb.SWITCH_N)
        bs.assert_same_graph(g, ix, n)
    finally:
        ix.close()


# ---- 5. vacuum keeps the precision ------------------------------------------------------------------------------------------------------------------
def test_vacuum_rebuilds_at_the_graph_precision():
    rows, dead, live = hb.vacuum_data()
    n, dim = hb.VACUUM_N, hb.VACUUM_DIM
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    ix = new_index("cosine", dim, 8, 60, n, hr.F16)
    try:
        ix.insert_batch_parallel([(int(ids[i]), rows[i]) for i in range(n)], hb.MAX_BATCH)
        for d in dead:
            assert ix.remove(int(ids[d]))
        assert ix.vacuum() == n - hb.VACUUM_DEAD
        assert ix.graph_precision() == VP.F16
        # the rebuild: survivors in ascending old index, batch-synchronous, HnswParams::auto(48) — over the ROUNDED survivors
        g = bs.new_oracle(dim, "cosine", 24, 300)
        g.build_batched(hb.rounded(rows[live], hr.F16), 2048)
        g32 = bs.new_oracle(dim, "cosine", 24, 300)
        g32.build_batched(rows[live], 2048)
        assert hb.differing_lists(g, g32, n - hb.VACUUM_DEAD) >= 1
        bs.assert_same_graph(g, ix, n - hb.VACUUM_DEAD)
    finally:
        ix.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def refused(ix, precision, code):
    with pytest.raises(va.VelesHipError) as e:
        ix.set_graph_precision(precision)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals_leave_the_handle_as_it_was():
    shape = hb.SHAPES[1]
    n, dim, M, efc = shape
    rows, _ = hb.case_rows("euclidean", shape)
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, n))
    try:
        msg = refused(ix, VP.F16, ERR_STATE)
        assert "vdb_hip_index_enable_half_precision(VDB_PRECISION_F16) first" in msg
        msg = refused(ix, VP.BF16, ERR_STATE)
        assert "vdb_hip_index_enable_half_precision(VDB_PRECISION_BF16) first" in msg
        refused(ix, 7, ERR_INVALID_ARG)
        ix.enable_half_precision(VP.F16)
        refused(ix, VP.BF16, ERR_STATE)                  # the other image is not the matching one
        assert ix.graph_precision() == VP.F32
        build(ix, rows, "batched")                       # ... and a following F32 build is the f32 graph
        bs.assert_same_graph(hb.case_oracle("euclidean", shape, hr.F32, "batched"), ix, n)
    finally:
        ix.close()
    bits = va.HnswIndex(64, DM.Hamming, va.HnswParams(8, 40, 100))
    try:
        refused(bits, VP.F16, ERR_UNSUPPORTED)
        refused(bits, 7, ERR_INVALID_ARG)
        bits.set_graph_precision(VP.F32)                 # the default is always accepted
        assert bits.graph_precision() == VP.F32
    finally:
        bits.close()
    two = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, n), devices=[0, 0], shard_mode=va.SHARD_RANGE)
    try:
        refused(two, VP.F32, ERR_UNSUPPORTED)
        refused(two, VP.F16, ERR_UNSUPPORTED)
    finally:
        two.close()


# ---- 7. no collateral -----------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_that_never_sets_a_precision_builds_the_f32_graph():
    shape, metric = hb.SHAPES[4], "cosine"
    n, dim, M, efc = shape
    rows, qs = hb.case_rows(metric, shape)
    ix = va.HnswIndex(dim, METRIC[metric], va.HnswParams(M, efc, n))
    half = new_index(metric, dim, M, efc, n, hr.F16)
    try:
        ix.enable_half_precision(VP.F16)
        ix.enable_half_precision(VP.BF16)
        assert ix.graph_precision() == VP.F32
        build(ix, rows, "batched")
        bs.assert_same_graph(hb.case_oracle(metric, shape, hr.F32, "batched"), ix, n)
        build(half, rows, "batched")
        # searches are launched as on any other graph, whatever it was built over
        for h in (ix, half):
            h.search_batch_parallel(qs, 10, SQ.Custom(64))
            k32 = h.last_kernels()
            h.search_batch_half_graph(qs, 10, 64, VP.F16)
            k16 = h.last_kernels()
            assert k32 & va.KERNEL_HNSW and not k32 & va.KERNEL_HNSW_HALF, hex(k32)
            assert k16 & va.KERNEL_HNSW_HALF and k16 & va.KERNEL_F16 and not k16 & va.KERNEL_HNSW, hex(k16)
            if h is ix:
                want = (k32, k16)
            assert (k32, k16) == want
    finally:
        ix.close()
        half.close()
