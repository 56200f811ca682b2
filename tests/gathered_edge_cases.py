"""The edges of the two gathered matrix-core tiers that tests/test_gpu_half_gathered.py and
tests/test_gpu_bits_gathered.py leave out — ONE table of cases, with their data and references, shared by
tests/test_gathered_edges_cpu.py (every case has the plan feature it is listed for; the references are what they claim) and
tests/test_gpu_gathered_edges.py (the kernels against them).  No GPU is touched here.

A case: the tier (("half", precision, metric) or ("bits", kind)), n, dim, the names of its filter sets, its (nq, k) shapes and the
plan feature it exists for.  Every k that sits on a plan boundary is taken from va.half_gather_plan, not from a constant.
References: tests/half_ref.py and the `scores` / `expected` of the two gathered test files; above dim 1 024 the half scores come from
a float64 matrix product (integer data: every summation order gives the same f32 — `exact_scores`, held to hr.scores by the CPU test)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_ref as hr  # noqa: E402
import test_gpu_bits_gathered as bg  # noqa: E402
import test_gpu_filtered as tf  # noqa: E402
import test_gpu_half_gathered as hg  # noqa: E402
import test_gpu_half_precision as hp  # noqa: E402

va = hg.va
N_CUS = 256                       # the plans below are asked for this many CUs (TN and nq_chunk do not depend on it)
HALF = [("half", p, m) for p, m in hg.CASES]
BITS = [("bits", kind) for kind in bg.KINDS]
Case = collections.namedtuple("Case", "group tier n dim sets shapes feature")


def plan(tier, dim, k, count, nq):
    return va.half_gather_plan(dim, k, count, nq, N_CUS) if tier[0] == "half" else va.bits_gather_plan(k, count, nq, N_CUS)


def boundary_k(tier, dim, count):
    """the largest k whose 128 k-lists fit the LDS at 130 queries; k + 1 falls back to TN = 16"""
    return next(k for k in range(1, 1 << 16) if plan(tier, dim, k + 1, count, 130)["tn"] == 16)


def dim_of(tier, half_dim, bits_dim):
    return half_dim if tier[0] == "half" else bits_dim


HALF_DIMS = [3, 17, 40, 67, 100, 1536, 4100]   # below one 8-element piece; pad columns inside the stride; below one slice; 64 + 3; 100; 24 slices; 64 slices + 4
BITS_DIMS = [17, 32, 2048, 4100]               # below one word; one word; eight slices; past sixteen slices with a masked word (4100 = 128 words + 4 bits)
CHUNK_NQ = [1030, 1088]                        # a second chunk of 6 queries (TN = 16) and of 64 (TN = 128)


def build_cases():
    out = []
    for tier in HALF + BITS:
        d = dim_of(tier, 72, 264)
        kb = boundary_k(tier, dim_of(tier, 200, 264), 9000)
        out.append(Case("chunks", tier, 600, d, ("65", "half"), [(1030, 10)], "chunk-tn16"))
        out.append(Case("chunks", tier, 600, d, ("65", "half"), [(1088, 10)], "chunk-tn128"))
        out.append(Case("fallback", tier, 9000, dim_of(tier, 200, 264), ("all", "65", "not10pct"), [(130, kb)], "boundary-tn128"))
        out.append(Case("fallback", tier, 9000, dim_of(tier, 200, 264), ("all", "65", "not10pct"), [(130, kb + 1)], "fallback-9-tiles"))
        out.append(Case("fallback", tier, 9000, dim_of(tier, 200, 264), ("all",), [(1024, kb + 1)], "fallback-64-tiles"))
        for dim in (HALF_DIMS if tier[0] == "half" else BITS_DIMS):
            out.append(Case("dims", tier, 1500, dim, ("65", "half", "not10pct"), [(1, 10), (17, 10), (40, 64)], "dim"))
        out.append(Case("appended", tier, 600, d, ("65", "not10pct"), [(17, 10), (130, 10)], "appended"))
        out.append(Case("dead", tier, 3000, d, ("200",), [(17, 10), (130, 10)], "dead-tiles"))
    for tier in HALF:
        if tier[2] == hr.COSINE:
            out.append(Case("tiny", tier, 600, 72, ("65", "half"), [(17, 65), (130, 65), (130, 10)], "tiny-norm"))
        out.append(Case("nan", tier, 600, 72, ("65", "half"), [(130, 10), (130, 65)], "nan-inf"))
    out.append(Case("probes", ("half", hr.F16, hr.DOT), 48, 128, ("every", "second"), [(1, 48), (20, 48), (130, 48)], "f16-probes"))
    return out


CASES = build_cases()


def cases(group, tiers=None):
    return [c for c in CASES if c.group == group and (tiers is None or c.tier in tiers)]


def seed_of(tier, n, dim):
    return [n, dim, 1 if tier[0] == "half" else 2] + [int(x) if not isinstance(x, str) else bg.KINDS.index(x) for x in tier[1:]]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def make(tier, rng, shape):
    return hp.ints(rng, shape) if tier[0] == "half" else bg.data(tier[1], rng, shape)


def stamp_distinct(tier, Q):
    """query i carries i in its first columns: pairwise distinct by construction, no period"""
    i = np.arange(len(Q))
    if tier[0] == "half":
        for c in range(4):
            Q[:, c] = (i // 9 ** c) % 9 - 4.0          # base-9 digits: 9^4 > 1 100 queries
    else:
        for c in range(11):
            bit = ((i >> c) & 1).astype(np.float32)    # 2^11 > 1 100
            Q[:, c] = 2.0 * bit - 1.0 if tier[1] == "binary" else bit
    return Q


def edge_sets(rng, n):
    """the tile-edge sets of the two gathered test files; "half" also holds rows 1 and 5 (the special-value plants need four common rows)"""
    sets = hg.tile_edge_sets(rng, n)
    h = np.union1d(sets["half"][2], [0, 1, 5, n - 1]).astype(np.int64)
    sets["half"] = (h, False, h)
    return sets


def exact_scores(metric, prec, rows, Q):
    """hr.scores for data whose every product and partial sum is an exact f32 (then the order of summation is free): the dot products
    and the squared norms from float64 matrix products, finished in f32 by hr.scores' rule"""
    r, q = hr.round_half(rows, prec).astype(np.float64), hr.round_half(Q, prec).astype(np.float64)
    dot = (q @ r.T).astype(np.float32)
    if metric == hr.DOT:
        return dot
    nq, nr = np.sqrt((q * q).sum(1).astype(np.float32)), np.sqrt((r * r).sum(1).astype(np.float32))
    with np.errstate(all="ignore"):
        out = dot / (nq[:, None] * nr[None, :])
    tiny = (nq[:, None] < hr.F32_EPSILON) | (nr[None, :] < hr.F32_EPSILON)
    return np.where(tiny, np.float32(0.0), out).astype(np.float32)


def largest_partial_sum(rows, Q):
    """an upper bound of every |partial sum| of every dot product and squared norm, in any order"""
    a, b = np.abs(rows.astype(np.float64)), np.abs(Q.astype(np.float64))
    return max((a.sum(1).max() * b.max()), (a * a).sum(1).max(), (b * b).sum(1).max())


def scores(tier, rows, Q):
    """[nq][n] f32 over ALL rows — half: larger = better (hr.topk); bits: smaller = better (bg.expected)"""
    if tier[0] == "bits":
        return bg.scores(tier[1], rows, Q)
    return exact_scores(tier[2], tier[1], rows, Q) if rows.shape[1] > 1024 else hr.scores(tier[2], tier[1], rows, Q)


def expected(tier, sc, ids, k, sel):
    return hg.expected(sc, ids, k, sel) if tier[0] == "half" else bg.expected(tier[1], sc, ids, k, sel)


Data = collections.namedtuple("Data", "rows ids Q sets sc extra")
_MADE = {}


def data_of(case, nq_made):
    """rows, ids, `nq_made` queries, the filter sets and the score matrix of a case: made once per (group, tier, n, dim), never changed"""
    key = (case.group, case.tier, case.n, case.dim, nq_made)
    if key not in _MADE:
        _MADE[key] = MAKERS[case.group](case, nq_made)
    return _MADE[key]


def plain(case, nq_made):
    """integer data / random bits with the plants of the existing gathered tests: zero rows, exact duplicates, a query equal to a row, a zero query"""
    tier, n, dim = case.tier, case.n, case.dim
    rng = np.random.default_rng(seed_of(tier, n, dim))
    rows, ids, Q = make(tier, rng, (n, dim)), tf.ext_ids(n), make(tier, rng, (nq_made, dim))
    rows[5] = 0.0
    rows[[256, 257]] = rows[[1, 1]]                      # duplicates: exact ties, by row
    Q[0] = rows[n - 1]
    if nq_made > 8:
        Q[8] = 0.0
    if case.group == "chunks":
        stamp_distinct(tier, Q)
    if case.group == "dims" and tier[0] == "half" and dim % 8:
        # the largest magnitudes in the LAST column: a pad or stride slip changes the ranking, not a low bit (32 is exact in bf16)
        rows[::3, dim - 1] = 32.0 * np.where(np.arange(0, n, 3) % 2 == 0, 1.0, -1.0)
        Q[::2, dim - 1] = 32.0 * np.where(np.arange(0, nq_made, 2) % 4 == 0, 1.0, -1.0)
    sets = edge_sets(rng, n)
    if case.group == "dead":
        s = np.sort(rng.choice(n, 200, replace=False)).astype(np.int64)
        sets = {"200": (s, False, s)}
    return Data(rows, ids, Q, sets, scores(tier, rows, Q), {})


def appended(case, nq_made):
    """n rows, then 70 more (three of them copies of queries) that arrive AFTER the filters were made: the scores cover all n + 70 rows,
    the sets only the first n"""
    tier, n, dim = case.tier, case.n, case.dim
    rng = np.random.default_rng(seed_of(tier, n + 70, dim))
    rows, ids, Q = make(tier, rng, (n + 70, dim)), tf.ext_ids(n + 70), make(tier, rng, (nq_made, dim))
    rows[[256, 257]] = rows[[1, 1]]
    rows[[n, n + 33, n + 69]] = Q[[0, 7, nq_made - 1]]    # the best row of three queries is one the filters cannot hold
    return Data(rows, ids, Q, edge_sets(rng, n), scores(tier, rows, Q), {"n0": n})


TINY_ROWS = (0, 5)          # in both sets ...
TINY_Q = (3, 11)            # ... parallel to query 3; query 11 is of the same kind


def tiny(case, nq_made):
    """Cosine: rows and a query whose norm is NON-ZERO and below kHalfNormEps = f32::EPSILON — f16: 2^-24 e0 (a subnormal, norm 6e-8);
    bf16: 1e-20 q (norm ~1e-19).  The rule gives them 0.0 whatever the dot product; an honest cosine would give 1.0 against query 3."""
    tier, n, dim = case.tier, case.n, case.dim
    rng = np.random.default_rng(seed_of(tier, n, dim) + [7])
    rows, ids, Q = hp.ints(rng, (n, dim)), tf.ext_ids(n), hp.ints(rng, (nq_made, dim))
    if tier[1] == hr.F16:
        Q[TINY_Q[0]] = 0.0
        Q[TINY_Q[0], 0] = 3.0
        small = np.zeros(dim, np.float32)
        small[0] = 2.0 ** -24
    else:
        small = (np.float32(1e-20) * Q[TINY_Q[0]]).astype(np.float32)
    rows[list(TINY_ROWS)] = small
    Q[TINY_Q[1]] = small
    return Data(rows, ids, Q, edge_sets(rng, n), scores(tier, rows, Q), {})


NAN_ROWS, INF_ROW, NAN_Q, INF_COL = (1, 5), 0, 77, 9


def nan_rows_of(tier):
    """the rows whose reference score is NaN against every query: the two that hold a NaN and, for f16 Cosine, the row that holds
    65 520 (inf in f16: its norm is inf and inf / inf is NaN; bf16 keeps 65 536, DotProduct keeps +-inf)"""
    return NAN_ROWS + ((INF_ROW,) if tier[1:] == (hr.F16, hr.COSINE) else ())


def nan(case, nq_made):
    tier, n, dim = case.tier, case.n, case.dim
    rng = np.random.default_rng(seed_of(tier, n, dim) + [9])
    rows, ids, Q = hp.ints(rng, (n, dim)), tf.ext_ids(n), hp.ints(rng, (nq_made, dim))
    rows[NAN_ROWS[0], 20] = np.nan
    rows[NAN_ROWS[1], 71] = np.nan
    rows[INF_ROW] = 0.0
    rows[INF_ROW, INF_COL] = 65520.0                    # alone in its row: the bf16 norm 65 536 and its products stay exact
    Q[:, INF_COL] = np.where(Q[:, INF_COL] == 0, 1.0, Q[:, INF_COL])   # (0 x inf would be one more NaN)
    Q[NAN_Q, 33] = np.nan
    return Data(rows, ids, Q, edge_sets(rng, n), scores(tier, rows, Q), {})


def probes(case, nq_made):
    """tests/test_gpu_half_precision.py::probe_small: hp.PROBES in column 0 of otherwise zero rows, every query e0"""
    n, dim = case.n, case.dim
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = np.resize(hp.PROBES, n)
    Q = np.zeros((nq_made, dim), np.float32)
    Q[:, 0] = 1.0
    ev, sec = np.arange(n, dtype=np.int64), np.arange(0, n, 2, dtype=np.int64)
    with np.errstate(over="ignore"):
        want = rows[:, 0].astype(np.float16).astype(np.float32)
    want[want == 0] = 0.0                               # (+0 + -0 = +0 in every summation order)
    return Data(rows, np.arange(n, dtype=np.uint64), Q, {"every": (ev, False, ev), "second": (sec, False, sec)}, hr.scores(hr.DOT, hr.F16, rows, Q),
                {"want": want})


MAKERS = {"chunks": plain, "fallback": plain, "dims": plain, "dead": plain, "appended": appended, "tiny": tiny, "nan": nan, "probes": probes}
NQ_MADE = {"chunks": 1100, "fallback": 130, "dims": 40, "dead": 130, "appended": 130, "tiny": 130, "nan": 130, "probes": 130}


def data(case):
    return data_of(case, NQ_MADE[case.group])


# the call with one filter per query of group a: filter A owns 1 030 of 1 100 queries, interleaved with 40 of filter B and 30 without one
def table_owners(nq=1100):
    own = np.zeros(nq, np.int64)                        # 0 = A
    own[np.arange(40) * 27 + 5] = 1                     # B
    own[np.arange(30) * 36 + 11] = 2                    # none
    assert (own == 0).sum() == 1030 and (own == 1).sum() == 40 and (own == 2).sum() == 30
    return own
