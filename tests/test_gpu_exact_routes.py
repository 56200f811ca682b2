"""Route pin of the exact-search dispatch (index.hip brute_dev / brute_mode_dev / brute_filtered_dev, select_stage.hip brute_bf16_dev,
storage_modes.hip, bits_gemm.hip): for a table of small cases, WHICH kernels answer a call and WHAT they return must stay what
tests/golden/exact_routes.json holds — the kernel-family bits (last_kernels), the selection level (last_select_level), the number of
timed launches (last_kernel_ms with OPT_KERNEL_TIMING on) and a SHA-256 over the returned ids, score bits and counts.

The golden file was recorded with this table (`python tests/test_gpu_exact_routes.py --record FILE`) before the dispatch was taken
apart into one function per tier, so a slip in a tier boundary, a chunk size or the order in which the stateful select_level_* rules
are asked shows as a failed assertion.  The data comes from seeded generators; every case uses a fresh handle (the adaptive hold
counters start equal) and the cases run in the order of the table, which is the order they were recorded in.

Two corpora keep every case to a second or two: A = 2 048 rows (dim 128; 256 where the query-LDS tile is wanted, 96 where
dim % 64 != 0 steers the half modes), B = 66 048 x 128 — just over kGemmBf16MinRows, the smallest size the selection stages, the
LDS-DMA schedule and the four-bit GEMM exist at."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

if __name__ == "__main__":  # (run as a script: no conftest.py puts the repository root on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
va = pytest.importorskip("velesdb_amd")
DM, SM, VP = va.DistanceMetric, va.StorageMode, va.VectorPrecision
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_routes.json")
NA, NB = 2048, 66048
TILE, ENGINE, SELECTOR, ROUTE = va.OPT_MAX_QUERY_TILE, va.OPT_SWEEP_ENGINE, va.OPT_SELECTOR_LEVEL, va.OPT_FILTER_ROUTE
LISTED, MASK = va.FILTER_ROUTE_LISTED, va.FILTER_ROUTE_MASK
COS, L2, DOT, HAM, JAC = DM.Cosine, DM.Euclidean, DM.DotProduct, DM.Hamming, DM.Jaccard


def case(name, metric, nq, k, n=NA, dim=128, mode="f32", opts=(), corpus="gauss", flt=None):
    """mode: f32 | bf16 | f16 | sq8 | binary; opts: ((option, value), ...); corpus: gauss | dups | ties;
    flt: None or (allowed rows, route option) — allowed = every `step`-th row when an int, the first `-step` rows of 16 dropped when negative"""
    return dict(name=name, metric=metric, nq=nq, k=k, n=n, dim=dim, mode=mode, opts=tuple(opts), corpus=corpus, flt=flt)


CASES = (
    # f32 Cosine / Dot on A: 1, 2, 3 MFMA tiles; GEMM; k past kGemmMaxK; two GEMM launches; no GEMM under a 48-query tile cap
    [case(f"cos_nq{nq}", COS, nq, 10) for nq in (1, 17, 40)]
    + [case("cos_nq64_gemm", COS, 64, 10), case("dot_nq64_k49_mfma", DOT, 64, 49), case("cos_nq1100_gemm2", COS, 1100, 10),
       case("cos_nq64_tile48", COS, 64, 10, opts=[(TILE, 48)]), case("dot_nq40_tile32", DOT, 40, 10, opts=[(TILE, 32)])]
    # ... the VALU engine: tiles of 1, 2, 4, 8, 8 + 1; query-LDS tiles of 16 / 32 at dim 256 (and below 12 queries: generic tiles)
    + [case(f"cos_valu_nq{nq}", COS, nq, 10, opts=[(ENGINE, 0)]) for nq in (1, 2, 4, 8, 9)]
    + [case(f"cos_valu_d256_nq{nq}", COS, nq, 10, dim=256, opts=[(ENGINE, 0)]) for nq in (11, 12, 24)]
    + [case("cos_valu_d256_nq24_tile16", COS, 24, 10, dim=256, opts=[(ENGINE, 0), (TILE, 16)])]
    # f32 Euclidean on A: VALU tiles; Euclid GEMM + re-rank; k + slack past kGemmMaxK; tie-heavy chunk; a few unproven queries
    + [case("l2_nq63_valu", L2, 63, 10), case("l2_nq64_gemm", L2, 64, 10), case("l2_nq64_k33", L2, 64, 33), case("l2_nq64_k12", L2, 64, 12),
       case("l2_nq64_dups", L2, 64, 10, corpus="dups"), case("l2_nq64_ties", L2, 64, 10, corpus="ties"),
       case("l2_nq64_valu_engine", L2, 64, 10, opts=[(ENGINE, 0)]), case("l2_d256_nq30_qlds", L2, 30, 10, dim=256)]
    # Hamming / Jaccard: fused (1, 2), VALU plan (3), no GEMM below kGemmBf16MinRows; on B: GEMM chunk + remainder
    + [case(f"{m.name.lower()}_nq{nq}", m, nq, 10) for m in (HAM, JAC) for nq in (1, 2, 3, 40)]
    + [case("ham_B_nq1027", HAM, 1027, 10, n=NB), case("jac_B_nq35", JAC, 35, 10, n=NB), case("ham_B_nq35_valu_engine", HAM, 35, 10, n=NB, opts=[(ENGINE, 0)]),
       case("ham_nq2_k17_unfused", HAM, 2, 17)]
    # B: WIDE at k 10 (selector 3, the default) and k 50; levels 2 / 1 / 0; Euclidean the same
    + [case("cos_B_nq16_k10", COS, 16, 10, n=NB), case("cos_B_nq16_k50", COS, 16, 50, n=NB),
       case("cos_B_nq16_sel2", COS, 16, 10, n=NB, opts=[(SELECTOR, 2)]), case("cos_B_nq16_sel1", COS, 16, 10, n=NB, opts=[(SELECTOR, 1)]),
       case("cos_B_nq16_sel0", COS, 16, 10, n=NB, opts=[(SELECTOR, 0)]), case("cos_B_nq15", COS, 15, 10, n=NB),
       case("l2_B_nq16_k10", L2, 16, 10, n=NB), case("l2_B_nq16_k50", L2, 16, 50, n=NB),
       case("l2_B_nq16_sel2", L2, 16, 10, n=NB, opts=[(SELECTOR, 2)]), case("l2_B_nq64_sel0", L2, 64, 10, n=NB, opts=[(SELECTOR, 0)])]
    # half modes: MFMA tiles of 1, 2, 4, 6 x 16; 128 x 128 GEMM; dim 96 keeps the tiles; B: LDS-DMA schedule (+ a remainder); Euclidean
    + [case(f"{p}_cos_nq{nq}", COS, nq, 10, mode=p) for p in ("bf16", "f16") for nq in (1, 17, 40, 64, 70)]
    + [case(f"{p}_cos_d96_nq64", COS, 64, 10, dim=96, mode=p) for p in ("bf16", "f16")]
    + [case(f"{p}_cos_B_nq224", COS, 224, 10, n=NB, mode=p) for p in ("bf16", "f16")]
    + [case("bf16_dot_B_nq300", DOT, 300, 10, n=NB, mode="bf16"), case("bf16_cos_nq64_tile48", COS, 64, 10, mode="bf16", opts=[(TILE, 48)])]
    + [case(f"{p}_l2_nq{nq}", L2, nq, 10, mode=p) for p in ("bf16", "f16") for nq in (1, 5, 17)]
    # SQ8: tiles of 1, 4, 8, 8 + 1; B: level 3 / WIDE, then the exact sweep for what they leave
    + [case(f"sq8_cos_nq{nq}", COS, nq, 10, mode="sq8") for nq in (1, 4, 8, 9)]
    + [case("sq8_l2_nq9", L2, 9, 10, mode="sq8"), case("sq8_B_nq16_k10", COS, 16, 10, n=NB, mode="sq8"), case("sq8_B_nq16_k50", COS, 16, 50, n=NB, mode="sq8"),
       case("sq8_B_nq16_sel2", COS, 16, 10, n=NB, mode="sq8", opts=[(SELECTOR, 2)]), case("sq8_B_nq5", DOT, 5, 10, n=NB, mode="sq8"),
       case("sq8_B_l2_nq16", L2, 16, 10, n=NB, mode="sq8")]
    # Binary: fused, VALU plan, GEMM chunk + remainder
    + [case("bin_nq1", COS, 1, 10, mode="binary"), case("bin_nq3", COS, 3, 10, mode="binary"), case("bin_nq40", L2, 40, 10, mode="binary"),
       case("bin_B_nq1027", COS, 1027, 10, n=NB, mode="binary"), case("bin_B_nq2", COS, 2, 10, n=NB, mode="binary")]
    # filtered: listed and mask routes in f32, SQ8, half Euclidean (and Binary, half Cosine: mask only); B: the mask keeps / loses the selection
    + [case("flt_cos_listed", COS, 5, 10, flt=(37, LISTED)), case("flt_cos_listed_nq40", COS, 40, 10, flt=(37, LISTED)),
       case("flt_cos_mask", COS, 5, 10, flt=(-2, MASK)), case("flt_cos_auto_sparse", COS, 5, 10, flt=(37, 0)), case("flt_cos_auto_dense", COS, 5, 10, flt=(-2, 0)),
       case("flt_l2_listed", L2, 3, 10, flt=(37, LISTED)), case("flt_l2_mask_gemm", L2, 64, 10, flt=(-2, MASK)),
       case("flt_ham_mask", HAM, 3, 10, flt=(-2, 0)), case("flt_ham_fused", HAM, 1, 10, flt=(37, 0)),
       case("flt_sq8_listed", COS, 2, 10, mode="sq8", flt=(37, LISTED)), case("flt_sq8_mask", COS, 9, 10, mode="sq8", flt=(-2, MASK)),
       case("flt_bf16_l2_listed", L2, 5, 10, mode="bf16", flt=(37, LISTED)), case("flt_f16_l2_mask", L2, 5, 10, mode="f16", flt=(-2, MASK)),
       case("flt_bf16_cos_mask", COS, 17, 10, mode="bf16", flt=(-2, 0)), case("flt_bin_mask", COS, 3, 10, mode="binary", flt=(-2, 0)),
       case("flt_cos_B_mask_keeps", COS, 16, 10, n=NB, flt=(-2, MASK)), case("flt_cos_B_mask_loses", COS, 16, 10, n=NB, flt=(37, MASK)),
       case("flt_l2_B_mask_keeps", L2, 16, 10, n=NB, flt=(-2, MASK)), case("flt_sq8_B_mask_keeps", COS, 16, 10, n=NB, mode="sq8", flt=(-2, MASK)),
       case("flt_sq8_B_mask_loses", COS, 16, 10, n=NB, mode="sq8", flt=(37, MASK))]
)
assert len({c["name"] for c in CASES}) == len(CASES)

_rows = {}


def corpus(kind, n, dim):
    """rows of a case (built once per shape and left unchanged) and the 1 100 queries every case takes its first nq from"""
    key = (kind, n, dim)
    if key not in _rows:
        rng = np.random.default_rng([n, dim, 20261021])
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        Q = rng.standard_normal((1100, dim)).astype(np.float32)
        if kind == "dups":    # 256 distinct rows, eight copies of each: every top-k ends inside a group of ties
            rows = np.tile(rows[:256], (n // 256, 1))
        elif kind == "ties":  # four queries each sit next to twenty identical rows (more than k + slack): those lack a proof, the other 60 have one
            for i in range(4):
                rows[100 + 32 * i: 100 + 32 * i + 20] = Q[i] + np.float32(0.01) * rows[100 + 32 * i]
        _rows[key] = (rows, Q)
    return _rows[key]


def run_case(c):
    rows, Q = corpus(c["corpus"], c["n"], c["dim"])
    n, nq, k, mode = c["n"], c["nq"], c["k"], c["mode"]
    ix = va.HnswIndex(c["dim"], c["metric"])
    try:
        ix.upload(np.arange(n, dtype=np.uint64) * 3 + 7, rows)
        if mode in ("bf16", "f16"):
            ix.enable_half_precision(VP.BF16 if mode == "bf16" else VP.F16)
        elif mode in ("sq8", "binary"):
            ix.set_storage_mode(SM.SQ8 if mode == "sq8" else SM.Binary)
        ix.set_option(va.OPT_KERNEL_TIMING, 1)
        for o, v in c["opts"]:
            ix.set_option(o, v)
        q = Q[:nq]
        if c["flt"] is None:
            call = {"f32": ix.search_batch_brute_force, "sq8": ix.search_batch_sq8, "binary": ix.search_batch_binary,
                    "bf16": lambda q_, k_: ix.search_batch_brute_force_half(q_, k_, VP.BF16),
                    "f16": lambda q_, k_: ix.search_batch_brute_force_half(q_, k_, VP.F16)}[mode]
            ids, sc, cnt = call(q, k)
        else:
            step, route = c["flt"]
            r = np.arange(n)
            allowed = r[::step] if step > 0 else r[r % 16 >= -step]
            ix.set_option(ROUTE, route)
            with ix.create_filter(allowed.astype(np.uint64) * 3 + 7) as f:
                call = {"f32": ix.search_batch_brute_force_filtered, "sq8": ix.search_batch_filtered_sq8, "binary": ix.search_batch_filtered_binary,
                        "bf16": lambda q_, k_, f_: ix.search_batch_filtered_half(q_, k_, f_, VP.BF16),
                        "f16": lambda q_, k_, f_: ix.search_batch_filtered_half(q_, k_, f_, VP.F16)}[mode]
                ids, sc, cnt = call(q, k, f)
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(cnt, dtype=np.uint32).tobytes())
        for i in range(nq):  # (what lies behind a query's count is padding)
            h.update(np.ascontiguousarray(ids[i, :cnt[i]]).tobytes())
            h.update(np.ascontiguousarray(sc[i, :cnt[i]]).view(np.uint32).tobytes())
        return {"kernels": ix.last_kernels(), "level": ix.last_select_level(), "launches": ix.last_kernel_ms()[1], "sha256": h.hexdigest()}
    finally:
        ix.close()


def test_exact_routes_match_the_recorded_dispatch(gpu_required):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert [g["name"] for g in golden] == [c["name"] for c in CASES], "the table and the golden file list different cases"
    bad = []
    for c, g in zip(CASES, golden):
        got = run_case(c)
        want = {f: g[f] for f in got if f in g}  # (a case without a digest in the golden file: its route triple alone is pinned)
        if {f: got[f] for f in want} != want:
            bad.append((c["name"], {f: (want[f], got[f]) for f in want if want[f] != got[f]}))
    assert not bad, f"(recorded, now) differ for: {bad}"


if __name__ == "__main__":  # --record FILE: run the table and write what it returned
    out = []
    for c_ in CASES:
        try:
            r_ = run_case(c_)
        except Exception as e_:  # noqa: BLE001 - a refused case is reported; anything the device raised ends the run
            print(f"{c_['name']:32s} ERROR {e_}", flush=True)
            if "hip" in str(e_).lower() or "illegal" in str(e_).lower():
                raise
            continue
        out.append({"name": c_["name"], **r_})
        print(f"{c_['name']:32s} kernels=0x{r_['kernels']:06x} level={r_['level']} launches={r_['launches']} {r_['sha256'][:12]}", flush=True)
    with open(sys.argv[sys.argv.index("--record") + 1], "w") as fh_:
        json.dump(out, fh_, indent=0)
        fh_.write("\n")
