"""tests/gathered_edge_cases.py on the CPU: every case has, by the tiers' own launch plan (va.half_gather_plan / va.bits_gather_plan at
256 CUs), the feature it is listed for, and the references are what they claim — integer data sums exactly in every order, the
float64 shortcut equals tests/half_ref.py, and the special-value cases hold NaN only where they say."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gathered_edge_cases as ge  # noqa: E402
import half_ref as hr  # noqa: E402

TIERS = ge.HALF + ge.BITS


def plans(case, d=None):
    """the plan of every (set, shape) of a case, chunk by chunk as the dispatch asks for them"""
    d = d or ge.data(case)
    for name in case.sets:
        count = len(d.sets[name][2])
        for nq, k in case.shapes:
            chunks, left = [], nq
            while left:
                p = ge.plan(case.tier, case.dim, k, count, left)
                assert p is not None, (case, name, nq, k)
                chunks.append(p)
                left -= p["nq_chunk"]
            yield name, count, nq, k, chunks


@pytest.mark.parametrize("tier", TIERS)
def test_chunk_cases_run_the_chunk_loop_twice(tier):
    seen = {}
    for case in ge.cases("chunks", [tier]):
        for name, count, nq, k, chunks in plans(case):
            assert len(chunks) == 2 and chunks[0]["nq_chunk"] == 1024 and chunks[0]["tn"] == 128, (case, name)
            seen[case.feature] = chunks[1]
            assert count == 65 or (256 < count <= 320 and count % 64)   # two tiles, the second one row long; five, the last partial
    assert seen["chunk-tn16"]["tn"] == 16 and seen["chunk-tn16"]["nq_chunk"] == 6
    assert seen["chunk-tn128"]["tn"] == 128 and seen["chunk-tn128"]["nq_chunk"] == 64
    Q = ge.data(ge.cases("chunks", [tier])[0]).Q
    assert len(np.unique(Q, axis=0)) == len(Q) == 1100    # pairwise distinct: an answer read from another offset differs
    own = ge.table_owners()
    assert ge.plan(tier, 72, 10, 65, int((own == 0).sum()))["nq_chunk"] == 1024 and (own == 1).sum() < 64 <= (own == 0).sum()


@pytest.mark.parametrize("tier", TIERS)
def test_fallback_cases_take_sixteen_query_tiles_at_64_or_more_queries(tier):
    feats = {}
    for case in ge.cases("fallback", [tier]):
        for name, count, nq, k, (p,) in plans(case):
            feats.setdefault(case.feature, []).append((name, nq, k, p, -(-count // 64)))
    (kb,) = {k for _, _, k, _, _ in feats["boundary-tn128"]}
    assert all(p["tn"] == 128 and nq == 130 for _, nq, _, p, _ in feats["boundary-tn128"])
    assert ge.plan(tier, 200, kb + 1, 9000, 130)["tn"] == 16 and ge.plan(tier, 200, kb, 9000, 130)["tn"] == 128   # the boundary itself
    for _, nq, k, p, _ in feats["fallback-9-tiles"]:
        assert k == kb + 1 and nq >= 64 and p["tn"] == 16 and p["qtiles"] == 9
    ((name, nq, k, p, ntiles),) = feats["fallback-64-tiles"]
    assert k == kb + 1 and nq == 1024 and p["tn"] == 16 and p["qtiles"] == 64 and name == "all"
    assert p["spans"] < ntiles and p["per_block"] >= 4    # a block walks several tiles; the three-slot rotation wraps
    # ... and at 130 queries the short list is one tile a block, the long ones two
    assert {p["per_block"] for n_, _, _, p, _ in feats["fallback-9-tiles"]} == {1, 2}


def test_dim_cases_cover_the_classes_the_issue_names():
    h, b = ge.HALF_DIMS, ge.BITS_DIMS
    assert any(d < 8 for d in h) and any(d % 8 and d > 64 for d in h) and any(d > 1024 and d % 64 for d in h)
    assert any(d < 32 for d in b) and 32 in b and any(d > 4096 and d % 32 for d in b)
    for tier in TIERS:
        assert sorted(c.dim for c in ge.cases("dims", [tier])) == (h if tier[0] == "half" else b)
        for case in ge.cases("dims", [tier]):
            for name, count, nq, k, (p,) in plans(case):
                assert p["tn"] == 16 and count % 64        # (40 queries: the 16-query instance; no list ends on a tile)


@pytest.mark.parametrize("tier", ge.HALF)
def test_integer_references_are_exact_in_every_order(tier):
    for case in ge.CASES:
        if case.tier != tier or case.group in ("tiny", "nan", "probes"):
            continue
        d = ge.data(case)
        assert ge.largest_partial_sum(d.rows, d.Q) < 2.0 ** 24, case
        assert np.array_equal(hr.round_half(d.rows, tier[1]), d.rows) and np.array_equal(hr.round_half(d.Q, tier[1]), d.Q)   # no rounding either
    d = ge.data(ge.cases("dims", [tier])[3])             # dim 67, the last column planted: the float64 shortcut IS hr.scores
    assert d.rows.shape[1] == 67 and np.abs(d.rows[:, 66]).max() == 32 and np.abs(d.Q[:, 66]).max() == 32
    a, b = ge.exact_scores(tier[2], tier[1], d.rows, d.Q), hr.scores(tier[2], tier[1], d.rows, d.Q)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    big = ge.data(ge.cases("dims", [tier])[-1])
    assert big.rows.shape[1] == 4100 and not np.isnan(big.sc).any()


@pytest.mark.parametrize("tier", ge.HALF)
def test_special_value_references(tier):
    (case,) = ge.cases("nan", [tier])
    d = ge.data(case)
    want = np.zeros(d.sc.shape, bool)
    want[:, list(ge.nan_rows_of(tier))] = True
    want[ge.NAN_Q, :] = True
    assert np.array_equal(np.isnan(d.sc), want)           # no NaN but the designated rows' and query's
    assert len(ge.nan_rows_of(tier)) <= 3 and all(set(ge.nan_rows_of(tier)) | {ge.INF_ROW} <= set(d.sets[s][2].tolist()) for s in case.sets)
    inf = d.sc[np.arange(130) != ge.NAN_Q, ge.INF_ROW]
    if tier[1] == hr.F16 and tier[2] == hr.DOT:
        assert np.all(np.isinf(inf)) and (inf > 0).any() and (inf < 0).any()
    elif tier[1] == hr.BF16:
        assert np.all(np.isfinite(inf))                   # bf16 keeps 65 536
    if tier[2] != hr.COSINE:
        return
    (case,) = ge.cases("tiny", [tier])
    d = ge.data(case)
    norms = hr.seq_norm(hr.round_half(d.rows[list(ge.TINY_ROWS)], tier[1]))
    assert np.all(norms > 0) and np.all(norms < hr.F32_EPSILON)              # non-zero and below the threshold
    assert np.all(d.sc[:, list(ge.TINY_ROWS)] == 0.0) and np.all(d.sc[ge.TINY_Q[1]] == 0.0)
    r, q = hr.round_half(d.rows[ge.TINY_ROWS[0]], tier[1]).astype(np.float64), hr.round_half(d.Q[ge.TINY_Q[0]], tier[1]).astype(np.float64)
    assert abs(r @ q / np.linalg.norm(r) / np.linalg.norm(q) - 1.0) < 1e-2   # parallel: without the rule the pair would score ~1.0
    assert 0 < (d.sc[ge.TINY_Q[0]] > 0).sum() and 0 < (d.sc[ge.TINY_Q[0], d.sets["65"][2]] < 0).sum()   # ... and 0.0 ranks inside the list


def test_probe_case_is_the_streaming_kernels_assertion():
    (case,) = ge.cases("probes")
    d = ge.data(case)
    assert np.array_equal(d.sc[0].view(np.uint32), d.extra["want"].view(np.uint32)) and np.isinf(d.extra["want"]).sum() >= 3
    assert [len(d.sets[s][2]) for s in case.sets] == [48, 24] and {k for _, k in case.shapes} == {48}
    assert [ge.plan(case.tier, case.dim, 48, 48, nq)["tn"] for nq, _ in case.shapes] == [16, 16, 128]


@pytest.mark.parametrize("tier", TIERS)
def test_appended_and_dead_cases(tier):
    (case,) = ge.cases("appended", [tier])
    d = ge.data(case)
    n0 = d.extra["n0"]
    assert len(d.rows) == n0 + 70 and all(d.sets[s][2].max() < n0 for s in case.sets)
    for qi, row in ((0, n0), (7, n0 + 33), (129, n0 + 69)):               # the copies would be the best row of their query
        best = d.sc[qi].argmin() if tier[0] == "bits" else d.sc[qi].argmax()
        assert d.sc[qi, row] == d.sc[qi, best]
    (case,) = ge.cases("dead", [tier])
    assert len(ge.data(case).sets["200"][2]) == 200      # tiles 0-3, the last one 8 rows long
