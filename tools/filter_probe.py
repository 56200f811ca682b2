#!/usr/bin/env python3
"""GPU probe of the filtered exact search (vdb_hip_index_search_batch_filtered), single MI355X, host-pointer calls (the filtered
entry point has no device-resident variant yet, so every figure carries the query upload and the result download — the unfiltered
yardstick is measured through the same kind of call).  Prints and writes what DESIGN.md 4.1g quotes, per metric:

  for every selectivity (share of the rows the filter allows) and batch size, k = 10:
    ms per call on the forced listed route, on the forced mask route, under the auto rule, and of the unfiltered VDB_SEARCH_BRUTE
    call on the same handle in the same run (no unfiltered code differs from the parent: that is the yardstick);
    which forced route is faster, and how far auto is from it;
    one query on the listed route: count x dim x 4 B / time, as a fraction of the whole-row gather rate --gather-tbs;
  --rider: HnswIndex.search_filtered (the over-fetch rule) for one query with the number of results it actually returned
  (needs the graph: build_graph over every row first — minutes at 1 M rows, off by default).

  --graph: the GRAPH leg instead (vdb_hip_index_search_graph_filtered) over the bench's graph shape (--rows x --dim,
  M 32, ef_construction 400, built here with build_graph: minutes at 1 M rows): densities 1 ... 1/1024, --graph-nq queries, k = 10;
  per density queries/s, recall@10 against the exact filtered answer (route 2) and the mean n_dist per query of the auto, walk and
  exact routes, with the over-fetch rule through plain VDB_SEARCH_HNSW (k' = max(4k, k + 10), post-filtered on the host) as the
  baseline, its recall and the share of queries it answers short.  This table is what would replace the two guesses of the
  auto rule (the factor 2 of the density-sized list, the `matched < ef` cut).  NO RUN OF IT IS RECORDED YET.
  --graph --precision f16|bf16: the three filtered routes go through vdb_hip_index_search_graph_filters_half over that
  image of the rows (enable_half_precision on the same handle); the exact-route truth and the over-fetch baseline stay f32.  Every
  route also gets its ALGORITHMIC bytes per query, n_dist * row bytes + n_expand * M0 * 4 + admitted * 4 with row bytes =
  2 * stride (+ 4 for the Cosine norm) over an image and 4 * stride over the f32 rows, the strides taken as the dimension rounded
  up to 8 elements, and `admitted` (one bitmap word per admitted neighbour, not visible from outside) bounded by n_dist.
  Beside every route the f32 filtered call on the same handle (`f32_<route>_*`), its timing blocks alternating with the image's.
  One run of it is recorded: profiles/filter_probe_half_f16_100k.json (100 K x 768, densities 0.5 and 0.1).
  --graph --precision int8 [--ratio R]: the three filtered routes go through vdb_hip_index_search_graph_filters_int8
  over the u8 codes (train_quantizer on the same handle) at oversampling ratio R.  Algorithmic bytes per walked query:
  n_dist * (dim + 4) + n_expand * M0 * 4 + admitted * 4 + k * R * dim * 4 for the re-score; the exact route is the f32 exact pass
  and is counted as such.  The f32 filtered call runs beside it as above, and both get recall@k against the f32 exact answer.
  One run of it is recorded: profiles/filter_probe_int8_100k.json (same shape and protocol).
  --graph --precision f16|bf16 --rescore [--ratio R]: the three filtered routes go through
  vdb_hip_index_search_graph_filters_half_rescore: the half walk at ef_w = max(ef, k * R) with the k * R best allowed
  candidates re-scored over the f32 rows.  Beside every route, on the same handle with alternating timing blocks: the f32 filtered
  call at ef = ef_w (`f32_<route>_*`) and the half filtered call without re-score at ef = ef_w (`half_<route>_*`); all three get
  recall@k against the f32 exact answer.  Algorithmic bytes per walked query: n_dist * (2 * stride [+ 4]) + k * R * (4 * stride
  [+ 4]) + n_expand * M0 * 4 + admitted * 4; the exact route is the f32 exact pass and is counted as such.
  One run of it per precision is recorded: profiles/filter_probe_half_rescore_100k.json (100 K x 768, densities 1.0, 0.5 and 0.1).
  --graph --per-query F: the PER-QUERY leg instead (vdb_hip_index_search_graph_filters): at each density F distinct
  random filters of that density, the --graph-nq queries dealt round-robin over them; one call of search_batch_with_filters against
  the same queries as F calls of search_batch_filtered_graph, one per filter — what a caller does today with the same library, timed
  in the same run, the spread of the blocks beside each.  Also n_dist per query of both (they must agree: the same walks), and the
  launches each side needs AT LEAST (first attempts by LDS class plus one exact pass; re-runs are not visible from outside).

  --exact-per-query F[,F...]: the PER-QUERY EXACT leg instead (vdb_hip_index_search_batch_filters): at each density F
  distinct random filters of that density, --graph-nq queries (1 024) dealt round-robin over them, k = 10; one call of
  search_batch_brute_force_with_filters beside the only way the library had before it — a loop of search_batch_brute_force_filtered
  calls, one per filter, over the same queries —, the blocks of the two alternating (--repeats rounds, at least five), median and
  min / max of the blocks of each; once under the auto route rule and once with mask substitution forced.  The answers are held
  to agree bit for bit first.  Asserted: at F = 1 the new call's median lies inside the loop's own min-max spread (it is the same
  code path); everything else is recorded.  Defaults of this leg: --rows 100000, --densities 0.001,0.01,0.1.
  --exact-per-query F[,F...] --storage sq8|binary|f16|bf16: the same leg over that image of the rows
  (vdb_hip_index_search_batch_filters_mode) beside a loop of vdb_hip_index_search_batch_filtered_mode calls, one per
  filter — the only thing the library had before it —, once per forced route (listed, mask) and under the auto rule.  The answers
  are held to agree first: bit for bit where the mode declares its summation order (SQ8, Binary, Euclidean over a half image; and
  everywhere here, the loop's call over a filter's queries being exactly the group's job).  The F = 1 rows are the same code path
  on both sides and are gated as above.  One run per image is recorded: profiles/filter_probe_filters_modes_sq8_100k.json and
  profiles/filter_probe_filters_modes_f16_100k.json (in both the gate failed: the loop's own min - max is 0.1 - 0.4 % of its
  median, 10 of 27 F = 1 medians lie outside it by at most 0.2 %, in both directions).

  --exact --storage sq8|binary|f16|bf16: the exact leg over that image of the rows (vdb_hip_index_search_batch_filtered_mode, DESIGN
  4.1o): per metric, batch size and selectivity the forced listed route, the forced mask route, the auto rule and — what an
  over-fetching caller pays today, the parent has no filtered call in these modes — the UNFILTERED call in the same mode on the same
  handle, the blocks of the four going round (unfiltered, listed, mask, auto, unfiltered, ...) in the same run.  Median and
  (max - min) / median of the blocks of each; whether a listed kernel ran on the forced listed route (Binary and Cosine / DotProduct
  over a half image have none: the column then repeats the mask route); which route auto took.  The routes are held to agree first:
  bit for bit where the mode declares its summation order (SQ8, Binary, Euclidean over a half image), the same ids otherwise.

Every figure is the median of --repeats blocks, each block the mean over enough calls to last ~--block-ms; the spread is
(max - min) / median over the blocks.  Not part of the product or the test-suite."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import velesdb_amd as va  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--dim", type=int, default=768)
p.add_argument("--k", type=int, default=10)
p.add_argument("--metrics", default="cosine,euclidean")
p.add_argument("--selectivities", default="0.001,0.01,0.1,0.5")
p.add_argument("--nq", default="1,16,64,256,1024")
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--block-ms", type=float, default=40.0)
p.add_argument("--gather-tbs", type=float, default=5.7, help="whole-row gather rate to compare one-query listed calls with, TB/s")
p.add_argument("--rider", action="store_true")
p.add_argument("--graph", action="store_true", help="the filtered graph search leg instead of the exact one")
p.add_argument("--graph-nq", type=int, default=1024)
p.add_argument("--per-query", type=int, default=0, help="with --graph: F distinct filters per density in one call against F single-filter calls")
p.add_argument("--exact", action="store_true", help="the exact leg (the default leg; names it next to --storage)")
p.add_argument("--storage", default="", choices=["", "sq8", "binary", "f16", "bf16"], help="with --exact: the image of the rows the filtered exact call reads")
p.add_argument("--exact-per-query", default="", help="F[,F...]: distinct filters per call of the exact per-query-filters leg")
p.add_argument("--precision", default="f32", choices=["f32", "f16", "bf16", "int8"], help="with --graph: the rows the filtered walk reads")
p.add_argument("--ratio", type=int, default=4, help="with --precision int8, or with --rescore: the oversampling ratio")
p.add_argument("--rescore", action="store_true", help="with --graph --precision f16|bf16: the half walk with the f32 re-score")
p.add_argument("--ef", type=int, default=128)
p.add_argument("--densities", default="1,0.5,0.25,0.125,0.0625,0.03125,0.015625,0.0078125,0.00390625,0.001953125,0.0009765625")
p.add_argument("--out", default="")
a = p.parse_args()
if a.exact and (a.graph or a.exact_per_query):
    p.error("--exact names the exact leg: not with --graph / --exact-per-query")
if a.storage and (a.graph or not (a.exact or a.exact_per_query)):
    p.error("--storage goes with --exact or --exact-per-query (the exact legs over that image of the rows)")
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
METRICS = {"cosine": va.DistanceMetric.Cosine, "euclidean": va.DistanceMetric.Euclidean, "dot": va.DistanceMetric.DotProduct}


def build(metric):
    ix = va.HnswIndex(a.dim, metric, va.HnswParams(32, 400, a.rows))
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    for base in range(0, a.rows, 250_000):
        n = min(250_000, a.rows - base)
        c = torch.randn((n, a.dim), generator=g, device=dev)
        torch.cuda.synchronize()
        ix.upload_dev(base, c.data_ptr(), n, st)
        torch.cuda.synchronize()
        del c
    return ix


def measure(fn):
    """median ms per call over blocks, relative spread of the blocks"""
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    iters = int(min(200, max(3, a.block_ms * 1e-3 / one)))
    blocks = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        blocks.append((time.perf_counter() - t0) / iters * 1e3)
    med = statistics.median(blocks)
    return med, (max(blocks) - min(blocks)) / med


def measure_pair(fa, fb):
    """measure() for two calls whose blocks alternate (a, b, a, b, ...): both see the same clocks and the same neighbours"""
    for _ in range(3):
        fa()
        fb()
    t0 = time.perf_counter()
    fa()
    fb()
    one = max((time.perf_counter() - t0) / 2, 1e-6)
    iters = int(min(200, max(3, a.block_ms * 1e-3 / one)))
    blocks = ([], [])
    for _ in range(a.repeats):
        for which, fn in enumerate((fa, fb)):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            blocks[which].append((time.perf_counter() - t0) / iters * 1e3)
    return tuple((statistics.median(b), (max(b) - min(b)) / statistics.median(b)) for b in blocks)


def measure_many(fns):
    """measure_pair for any number of calls: the blocks go round (a, b, c, a, b, c, ...)"""
    for _ in range(3):
        for fn in fns:
            fn()
    t0 = time.perf_counter()
    for fn in fns:
        fn()
    one = max((time.perf_counter() - t0) / len(fns), 1e-6)
    iters = int(min(200, max(3, a.block_ms * 1e-3 / one)))
    blocks = [[] for _ in fns]
    for _ in range(a.repeats):
        for which, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            blocks[which].append((time.perf_counter() - t0) / iters * 1e3)
    return [(statistics.median(b), (max(b) - min(b)) / statistics.median(b)) for b in blocks]


def graph_leg():
    rows_out = []
    half_mode = {"f16": va.MODE_HNSW_F16, "bf16": va.MODE_HNSW_BF16}.get(a.precision)
    stride, m0 = (a.dim + 7) // 8 * 8, 2 * 32
    for mname in a.metrics.split(","):
        ix = build(METRICS[mname])
        ix.set_option(va.OPT_COMBINE_MAX_BATCH, 0)
        if half_mode is not None:
            ix.enable_half_precision(va.VectorPrecision.F16 if a.precision == "f16" else va.VectorPrecision.BF16)
        row_bytes = 4 * stride if half_mode is None else 2 * stride + (4 if mname == "cosine" else 0)
        int8 = a.precision == "int8"
        rescore = a.rescore and half_mode is not None
        ef_w = max(a.ef if a.ef else max(128, 4 * a.k), a.k * a.ratio) if rescore else a.ef  # what the comparison calls get as ef
        norm_bytes = 4 if mname == "cosine" else 0
        if int8:
            ix.train_quantizer()
            row_bytes = a.dim + 4  # the codes and the row's sum of squared codes

        def filtered(Q, flt, route):
            if int8:
                return ix.search_batch_filtered_graph_int8(Q, a.k, flt, ef=a.ef, oversampling=a.ratio, route=route)
            if half_mode is None:
                return ix.search_batch_filtered_graph(Q, a.k, flt, ef=a.ef, route=route)
            if rescore:
                return ix.search_batch_filtered_graph_half_rescore(Q, a.k, flt, half_mode, ef=a.ef, oversampling=a.ratio, route=route)
            return ix.search_batch_filtered_graph_half(Q, a.k, flt, half_mode, ef=a.ef, route=route)
        t0 = time.perf_counter()
        ix.build_graph(0)
        print(f"# {mname}: graph over {a.rows} rows in {time.perf_counter() - t0:.1f} s", flush=True)
        rng = np.random.default_rng(7)
        Q = rng.standard_normal((a.graph_nq, a.dim)).astype(np.float32)
        kk = max(4 * a.k, a.k + 10)
        for dens in [float(x) for x in a.densities.split(",")]:
            count = max(1, int(a.rows * dens))
            allowed = np.sort(rng.choice(a.rows, size=count, replace=False)).astype(np.uint64)
            mask = np.zeros(a.rows, dtype=bool)
            mask[allowed.astype(np.int64)] = True
            with ix.create_filter(allowed) as flt:
                row = dict(leg="graph", metric=mname, precision=a.precision, rows=a.rows, dim=a.dim, k=a.k, ef=a.ef, nq=a.graph_nq,
                           density=dens, count=count)
                if rescore:
                    row.update(rescore=True, ratio=a.ratio, ef_w=ef_w)
                (eid, _, ecnt), _ = ix.search_batch_filtered_graph(Q, a.k, flt, ef=a.ef, route=va.ROUTE_EXACT)
                truth = [set(eid[i, :ecnt[i]].tolist()) for i in range(a.graph_nq)]

                def recall(ids, cnt):
                    return float(np.mean([len(truth[i] & set(ids[i][:cnt[i]])) / max(1, len(truth[i])) for i in range(a.graph_nq)]))
                for name, route in (("auto", va.ROUTE_AUTO), ("walk", va.ROUTE_WALK), ("exact", va.ROUTE_EXACT)):
                    try:
                        (ids, _, cnt), routes = filtered(Q, flt, route)
                    except va.VelesHipError as e:  # the walk route refuses queries whose list would not fit
                        row[name + "_error"] = str(e)
                        continue
                    n_dist, n_expand = ix.last_search_stats()[:2]
                    row[name + "_n_dist"] = n_dist / a.graph_nq
                    row[name + "_algo_bytes"] = (n_dist * row_bytes + n_expand * m0 * 4 + n_dist * 4) / a.graph_nq
                    row[name + "_walked"] = float(np.mean(routes == 1))
                    row[name + "_recall"] = recall(ids.tolist(), cnt.tolist())
                    if int8:  # the exact pass reads f32 rows; a walked query re-scores k * ratio of them
                        if route == va.ROUTE_EXACT:
                            row[name + "_algo_bytes"] = (n_dist * 4 * stride + n_dist * 4) / a.graph_nq
                        else:
                            row[name + "_algo_bytes"] += row[name + "_walked"] * a.k * a.ratio * a.dim * 4
                    if rescore:  # the exact pass reads f32 rows; a walked query re-scores k * ratio of them
                        if route == va.ROUTE_EXACT:
                            row[name + "_algo_bytes"] = (n_dist * 4 * stride + n_dist * 4) / a.graph_nq
                        else:
                            row[name + "_algo_bytes"] += row[name + "_walked"] * a.k * a.ratio * (4 * stride + norm_bytes)
                        # beside it: the f32 filtered walk and the half filtered walk without re-score, both at ef = ef_w
                        f32_call = lambda: ix.search_batch_filtered_graph(Q, a.k, flt, ef=ef_w, route=route)  # noqa: E731
                        half_call = lambda: ix.search_batch_filtered_graph_half(Q, a.k, flt, half_mode, ef=ef_w, route=route)  # noqa: E731
                        for tag, call, rb in (("f32_", f32_call, 4 * stride), ("half_", half_call, row_bytes)):
                            (oids, _, ocnt), _ = call()
                            od, oe = ix.last_search_stats()[:2]
                            row[tag + name + "_recall"] = recall(oids.tolist(), ocnt.tolist())
                            row[tag + name + "_n_dist"] = od / a.graph_nq
                            row[tag + name + "_algo_bytes"] = (od * rb + oe * m0 * 4 + od * 4) / a.graph_nq
                        (ms, sp), (fms, fsp), (hms, hsp) = measure_many([lambda: filtered(Q, flt, route), f32_call, half_call])
                        row["f32_" + name + "_qps"], row["f32_" + name + "_spread"] = a.graph_nq / (fms * 1e-3), fsp
                        row["half_" + name + "_qps"], row["half_" + name + "_spread"] = a.graph_nq / (hms * 1e-3), hsp
                    elif half_mode is None and not int8:
                        ms, sp = measure(lambda: filtered(Q, flt, route))
                    else:  # the f32 filtered walk of the same build on the same handle, blocks alternating
                        (fids, _, fcnt), _ = ix.search_batch_filtered_graph(Q, a.k, flt, ef=a.ef, route=route)
                        fd, fe = ix.last_search_stats()[:2]
                        row["f32_" + name + "_recall"] = recall(fids.tolist(), fcnt.tolist())
                        row["f32_" + name + "_n_dist"] = fd / a.graph_nq
                        row["f32_" + name + "_algo_bytes"] = (fd * 4 * stride + fe * m0 * 4 + fd * 4) / a.graph_nq
                        (ms, sp), (fms, fsp) = measure_pair(lambda: filtered(Q, flt, route),
                                                            lambda: ix.search_batch_filtered_graph(Q, a.k, flt, ef=a.ef, route=route))
                        row["f32_" + name + "_qps"], row["f32_" + name + "_spread"] = a.graph_nq / (fms * 1e-3), fsp
                    row[name + "_qps"], row[name + "_spread"] = a.graph_nq / (ms * 1e-3), sp
                # the over-fetch rule: plain VDB_SEARCH_HNSW at k' = max(4k, k + 10), the caller drops what the filter rejects
                pid, _, pcnt = ix._search_raw(Q, kk, 0, va.MODE_HNSW)
                row["overfetch_n_dist"] = ix.last_search_stats()[0] / a.graph_nq
                kept = [[int(x) for x in pid[i, :pcnt[i]] if mask[int(x)]][:a.k] for i in range(a.graph_nq)]
                row["overfetch_recall"] = recall(kept, [len(x) for x in kept])
                row["overfetch_short"] = float(np.mean([len(x) < min(a.k, count) for x in kept]))
                ms, sp = measure(lambda: ix._search_raw(Q, kk, 0, va.MODE_HNSW))
                row["overfetch_qps"], row["overfetch_spread"] = a.graph_nq / (ms * 1e-3), sp
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        ix.close()
    return rows_out


def per_query_leg():
    F, rows_out = a.per_query, []
    for mname in a.metrics.split(","):
        ix = build(METRICS[mname])
        ix.set_option(va.OPT_COMBINE_MAX_BATCH, 0)
        t0 = time.perf_counter()
        ix.build_graph(0)
        print(f"# {mname}: graph over {a.rows} rows in {time.perf_counter() - t0:.1f} s", flush=True)
        rng = np.random.default_rng(7)
        Q = rng.standard_normal((a.graph_nq, a.dim)).astype(np.float32)
        of = np.arange(a.graph_nq) % F
        parts = [np.flatnonzero(of == j) for j in range(F)]
        Qs = [np.ascontiguousarray(Q[p]) for p in parts]
        for dens in [float(x) for x in a.densities.split(",")]:
            count = max(1, int(a.rows * dens))
            flts = [ix.create_filter(np.sort(rng.choice(a.rows, size=count, replace=False)).astype(np.uint64)) for _ in range(F)]
            per_q = [flts[j] for j in of]
            row = dict(leg="per_query", metric=mname, rows=a.rows, dim=a.dim, k=a.k, ef=a.ef, nq=a.graph_nq, filters=F, density=dens, count=count)

            def one_call():
                return ix.search_batch_with_filters(Q, a.k, per_q, ef=a.ef)

            def single_calls():
                return [ix.search_batch_filtered_graph(Qs[j], a.k, flts[j], ef=a.ef) for j in range(F) if len(parts[j])]
            (ids, sc, cnt), routes = one_call()
            row["n_dist"] = ix.last_search_stats()[0] / a.graph_nq
            row["walked"] = float(np.mean(routes == 1))
            nd, exact_calls = 0, 0
            for j in range(F):  # the answers agree bit for bit (a probe that times different answers measures nothing)
                if not len(parts[j]):
                    continue
                (i1, s1, c1), r1 = ix.search_batch_filtered_graph(Qs[j], a.k, flts[j], ef=a.ef)
                nd += ix.last_search_stats()[0]
                exact_calls += bool(np.any(r1 == 2))
                assert np.array_equal(i1, ids[parts[j]]) and np.array_equal(s1.view(np.uint32), sc[parts[j]].view(np.uint32)), (mname, dens, j)
                assert np.array_equal(c1, cnt[parts[j]]) and np.array_equal(r1, routes[parts[j]]), (mname, dens, j)
            row["single_n_dist"] = nd / a.graph_nq
            # every filter of a density has the same size, so the same first list: one walk launch for the call, one per single call
            used = sum(1 for p in parts if len(p))
            row["launches_at_least"] = int(np.any(routes == 1)) + int(np.any(routes == 2))
            row["single_launches_at_least"] = (used if np.any(routes == 1) else 0) + exact_calls
            ms, sp = measure(one_call)
            row["ms"], row["spread"], row["qps"] = ms, sp, a.graph_nq / (ms * 1e-3)
            ms1, sp1 = measure(single_calls)
            row["single_ms"], row["single_spread"], row["single_qps"] = ms1, sp1, a.graph_nq / (ms1 * 1e-3)
            row["single_over_one_call"] = ms1 / ms
            for f in flts:
                f.close()
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        ix.close()
    return rows_out


def measure_alternating(fa, fb):
    """blocks of the two calls alternate (a, b, a, b, ...); per call the median, min and max ms of its blocks"""
    for _ in range(2):
        fa()
        fb()
    t0 = time.perf_counter()
    fa()
    fb()
    one = max((time.perf_counter() - t0) / 2, 1e-6)
    iters = int(min(200, max(1, a.block_ms * 1e-3 / one)))
    blocks = ([], [])
    for _ in range(max(a.repeats, 5)):
        for which, fn in enumerate((fa, fb)):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            blocks[which].append((time.perf_counter() - t0) / iters * 1e3)
    return tuple(dict(median=statistics.median(b), min=min(b), max=max(b)) for b in blocks)


def exact_per_query_leg():
    rows_out = []
    nq = a.graph_nq
    for mname in a.metrics.split(","):
        ix = build(METRICS[mname])
        ix.set_option(va.OPT_COMBINE_MAX_BATCH, 0)
        mode = {"": va.MODE_BRUTE, "sq8": va.MODE_BRUTE_SQ8, "binary": va.MODE_BRUTE_BINARY, "f16": va.MODE_BRUTE_F16, "bf16": va.MODE_BRUTE_BF16}[a.storage]
        if a.storage in ("sq8", "binary"):
            ix.set_storage_mode(va.StorageMode.SQ8 if a.storage == "sq8" else va.StorageMode.Binary)
        elif a.storage:
            ix.enable_half_precision(va.VectorPrecision.F16 if a.storage == "f16" else va.VectorPrecision.BF16)
        rng = np.random.default_rng(7)
        Q = rng.standard_normal((nq, a.dim)).astype(np.float32)
        for F in [int(x) for x in a.exact_per_query.split(",")]:
            of = np.arange(nq) % F
            parts = [np.flatnonzero(of == j) for j in range(F)]
            Qs = [np.ascontiguousarray(Q[p]) for p in parts]
            for dens in [float(x) for x in a.densities.split(",")]:
                count = max(1, int(a.rows * dens))
                flts = [ix.create_filter(np.sort(rng.choice(a.rows, size=count, replace=False)).astype(np.uint64)) for _ in range(F)]
                per_q = [flts[j] for j in of]

                # both sides are timed AT THE C ENTRY POINTS with their tables and output arrays prepared once: building a
                # 1 024-entry filter table in Python costs ~0.1 ms per call, which is the binding's, not the library's
                L, vp = va._ffi.lib(), (lambda x: x.ctypes.data_as(C.c_void_p))
                handles = (C.c_void_p * F)(*[f._h for f in flts])
                fq = np.ascontiguousarray(of, dtype=np.uint32)
                o_ids, o_sc, o_cnt = np.empty((nq, a.k), np.uint64), np.empty((nq, a.k), np.float32), np.zeros(nq, np.uint32)
                outs = [(np.empty((len(p), a.k), np.uint64), np.empty((len(p), a.k), np.float32), np.zeros(len(p), np.uint32)) for p in parts]

                if a.storage:  # (the two mode calls take the mode in front of the queries)
                    new_fn, loop_fn = L.vdb_hip_index_search_batch_filters_mode, L.vdb_hip_index_search_batch_filtered_mode
                    new_args = (ix._h, handles, F, vp(fq), mode, vp(Q), nq, a.k, vp(o_ids), vp(o_sc), vp(o_cnt))
                    loop_args = [(ix._h, flts[j]._h, mode, vp(Qs[j]), len(parts[j]), a.k, vp(outs[j][0]), vp(outs[j][1]), vp(outs[j][2]))
                                 for j in range(F)]
                else:
                    new_fn, loop_fn = L.vdb_hip_index_search_batch_filters, L.vdb_hip_index_search_batch_filtered
                    new_args = (ix._h, handles, F, vp(fq), vp(Q), nq, a.k, va.MODE_BRUTE, vp(o_ids), vp(o_sc), vp(o_cnt))
                    loop_args = [(ix._h, flts[j]._h, vp(Qs[j]), len(parts[j]), a.k, va.MODE_BRUTE, vp(outs[j][0]), vp(outs[j][1]), vp(outs[j][2]))
                                 for j in range(F)]

                def one_call():
                    va._ffi.check(new_fn(*new_args))
                    return o_ids, o_sc, o_cnt

                def loop():
                    for args in loop_args:
                        va._ffi.check(loop_fn(*args))
                    return outs
                routes = (("auto", va.FILTER_ROUTE_AUTO), ("mask", va.FILTER_ROUTE_MASK))
                if a.storage:
                    routes = (("listed", va.FILTER_ROUTE_LISTED),) + routes
                for rname, route in routes:
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    row = dict(leg="exact_per_query", storage=a.storage or "f32", metric=mname, arith=ix.sweep_arith_mode(a.k), rows=a.rows, dim=a.dim, k=a.k, nq=nq, filters=F,
                               density=dens, count=count, route=rname)
                    ids, sc, cnt = one_call()
                    row["plan"] = list(ix.last_filters_exact_plan())
                    for j, (i1, s1, c1) in enumerate(loop()):  # a probe that times different answers measures nothing
                        pj = parts[j]
                        assert len(pj) and np.array_equal(c1, cnt[pj]) and np.array_equal(i1, ids[pj]), (mname, F, dens, rname, j)
                        assert np.array_equal(s1.view(np.uint32), sc[pj].view(np.uint32)), (mname, F, dens, rname, j)
                    new, old = measure_alternating(one_call, loop)
                    row["one_call_ms"], row["loop_ms"] = new, old
                    row["loop_over_one_call"] = old["median"] / new["median"]
                    if F == 1:  # the same code path
                        row["f1_inside_loop_spread"] = bool(old["min"] <= new["median"] <= old["max"])
                    rows_out.append(row)
                    print(json.dumps(row), flush=True)
                for f in flts:
                    f.close()
        ix.close()
    bad = [r for r in rows_out if r["filters"] == 1 and not r["f1_inside_loop_spread"]]
    return rows_out, bad


def storage_leg():
    rows_out = []
    for mname in [m for m in a.metrics.split(",") if m]:
        ix = build(METRICS[mname])
        ix.set_option(va.OPT_COMBINE_MAX_BATCH, 0)  # the unfiltered yardstick launches alone too
        if a.storage == "sq8":
            ix.set_storage_mode(va.StorageMode.SQ8)
            plain, filtered = ix.search_batch_sq8, ix.search_batch_filtered_sq8
        elif a.storage == "binary":
            ix.set_storage_mode(va.StorageMode.Binary)
            plain, filtered = ix.search_batch_binary, ix.search_batch_filtered_binary
        else:
            prec = va.VectorPrecision.F16 if a.storage == "f16" else va.VectorPrecision.BF16
            ix.enable_half_precision(prec)
            plain, filtered = (lambda Q, k: ix.search_batch_brute_force_half(Q, k, prec)), (lambda Q, k, f: ix.search_batch_filtered_half(Q, k, f, prec))
        declared = a.storage in ("sq8", "binary") or mname == "euclidean"  # the mode's summation order is declared: the routes agree bit for bit
        rng = np.random.default_rng(7)
        for nq in [int(x) for x in a.nq.split(",")]:
            Q = rng.standard_normal((nq, a.dim)).astype(np.float32)
            for sel in [float(x) for x in a.selectivities.split(",")]:
                count = max(1, int(a.rows * sel))
                allowed = np.sort(rng.choice(a.rows, size=count, replace=False)).astype(np.uint64)
                with ix.create_filter(allowed) as flt:
                    row = dict(storage=a.storage, metric=mname, rows=a.rows, dim=a.dim, k=a.k, nq=nq, selectivity=sel, count=count)
                    ref = None
                    for name, route in (("listed", va.FILTER_ROUTE_LISTED), ("mask", va.FILTER_ROUTE_MASK), ("auto", va.FILTER_ROUTE_AUTO)):
                        ix.set_option(va.OPT_FILTER_ROUTE, route)
                        got = filtered(Q, a.k, flt)
                        ran = bool(ix.last_kernels() & va.KERNEL_SWEEP_LISTED)
                        if name == "listed":
                            row["listed_kernel_ran"] = ran
                        if name == "auto":
                            row["auto_took"] = "listed" if ran else "mask"
                        if ref is None:
                            ref = got
                        else:  # (a probe that times wrong answers measures nothing)
                            assert np.array_equal(ref[0], got[0]), (mname, nq, sel, name)
                            assert not declared or np.array_equal(ref[1].view(np.uint32), got[1].view(np.uint32)), (mname, nq, sel, name)

                    def call(route):
                        def fn():
                            ix.set_option(va.OPT_FILTER_ROUTE, route)
                            filtered(Q, a.k, flt)
                        return fn
                    res = measure_many([lambda: plain(Q, a.k), call(va.FILTER_ROUTE_LISTED), call(va.FILTER_ROUTE_MASK), call(va.FILTER_ROUTE_AUTO)])
                    for name, (ms, sp) in zip(("unfiltered", "listed", "mask", "auto"), res):
                        row[name + "_ms"], row[name + "_spread"] = ms, sp
                    best = min(("listed", "mask"), key=lambda r: row[r + "_ms"])
                    row["better"] = best
                    row["auto_over_better"] = row["auto_ms"] / row[best + "_ms"]
                    row["listed_over_unfiltered"] = row["listed_ms"] / row["unfiltered_ms"]
                    rows_out.append(row)
                    print(json.dumps(row), flush=True)
        ix.close()
    return rows_out


table = []
f1_outside = []
if a.storage and not a.exact_per_query:
    table = storage_leg()
    a.metrics = ""
elif a.exact_per_query:
    if a.rows == 1_000_000:
        a.rows = 100_000
    if a.densities.startswith("1,0.5"):
        a.densities = "0.001,0.01,0.1"
    table, f1_outside = exact_per_query_leg()
    a.metrics = ""
elif a.graph:
    table = per_query_leg() if a.per_query > 0 else graph_leg()
    a.metrics = ""
for mname in [m for m in a.metrics.split(",") if m]:
    ix = build(METRICS[mname])
    ix.set_option(va.OPT_COMBINE_MAX_BATCH, 0)  # the unfiltered yardstick launches alone too
    rng = np.random.default_rng(7)
    if a.rider:
        t0 = time.perf_counter()
        ix.build_graph()
        print(f"# {mname}: graph over {a.rows} rows in {time.perf_counter() - t0:.1f} s", flush=True)
    for nq in [int(x) for x in a.nq.split(",")]:
        Q = rng.standard_normal((nq, a.dim)).astype(np.float32)
        plain, plain_sp = measure(lambda: ix.search_batch_brute_force(Q, a.k))
        for sel in [float(x) for x in a.selectivities.split(",")]:
            count = max(1, int(a.rows * sel))
            allowed = np.sort(rng.choice(a.rows, size=count, replace=False)).astype(np.uint64)
            with ix.create_filter(allowed) as flt:
                row = dict(metric=mname, rows=a.rows, dim=a.dim, k=a.k, nq=nq, selectivity=sel, count=count, unfiltered_ms=plain, unfiltered_spread=plain_sp)
                ref = None
                for name, route in (("listed", va.FILTER_ROUTE_LISTED), ("mask", va.FILTER_ROUTE_MASK), ("auto", va.FILTER_ROUTE_AUTO)):
                    ix.set_option(va.OPT_FILTER_ROUTE, route)
                    got = ix.search_batch_brute_force_filtered(Q, a.k, flt)
                    if name == "auto":
                        row["auto_took"] = "listed" if ix.last_kernels() & va.KERNEL_SWEEP_LISTED else "mask"
                    if ref is None:
                        ref = got
                    else:  # the routes agree bit for bit (a probe that times wrong answers measures nothing)
                        assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1].view(np.uint32), got[1].view(np.uint32)), (mname, nq, sel, name)
                    row[name + "_ms"], row[name + "_spread"] = measure(lambda: ix.search_batch_brute_force_filtered(Q, a.k, flt))
                best = min(("listed", "mask"), key=lambda r: row[r + "_ms"])
                row["better"] = best
                row["auto_over_better"] = row["auto_ms"] / row[best + "_ms"]
                if nq == 1:
                    row["listed_gather_tbs"] = count * a.dim * 4 / (row["listed_ms"] * 1e-3) / 1e12
                    row["listed_gather_fraction"] = row["listed_gather_tbs"] / a.gather_tbs
                if a.rider and nq == 1:
                    keep = set(int(x) for x in allowed)
                    t0 = time.perf_counter()
                    res = ix.search_filtered(Q[0], a.k, lambda i: i in keep)
                    row["rider_ms"], row["rider_results"] = (time.perf_counter() - t0) * 1e3, len(res)
                table.append(row)
                print(json.dumps(row), flush=True)
    ix.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=va.device_name(0), table=table), f, indent=1)
# (after the table is written: the one gate of the per-query exact leg)
assert not f1_outside, ("F = 1: the new call's median lies outside the loop's min-max spread", f1_outside)
