#!/usr/bin/env python3
"""GPU probe of the hybrid search (vdb_hip_index_hybrid_search), single MI355X, host-pointer calls.  For k 10 / 50 / 100
and 1 / 128 / 1 024 user queries per call, with text lists of 2k random live ids about half of which also sit in the query's vector
list, it times over the same index and queries in the same run:

  fused   one call of hybrid_search_batch: the walks at 2k, the text ids mapped to rows, hybrid_fuse_kernel, k records per query back;
  host    what a caller of this library does without it: search_batch (VDB_SEARCH_HNSW, ef = 0) at 2k, every list back on the host,
          then the fusion there — the compiled host model of the product's rule (tests/hybrid_model.cpp over csrc/vdb_hybrid.hpp,
          built with g++ -O2), one query after the other on one thread;
  and the share of `host` that is the host fusion alone.

Both sides must return the same records (checked bit for bit before anything is timed).  Every figure is the median of --repeats
blocks, each block the mean over enough calls to last ~--block-ms; the spread is (max - min) / median over the blocks.
There is no pass bar.  One run is recorded: DESIGN.md 4.1p, profiles/hybrid_probe_100k.log.

--per-query F[,F...] (--walk-rows names the rows forms, --rows being the corpus size here): instead of the table above,
for every F the --queries user queries (the largest value) are spread over F distinct filters of --density and, at the first --k, it
times on ONE handle in alternating blocks
  new     hybrid_search_batch_filters with the per-query table, once per rows form of --walk-rows;
  loop    what a caller does without the table: one hybrid_search_batch(flt) call per distinct filter over that filter's queries (f32);
  and for F = 1 also `one`: hybrid_search_batch(flt) itself, the call `new` must cost what it costs.
The f32 rows of `new` and `loop` must return the same records (checked before anything is timed).  Raw records: --out.
Not part of the product or the test-suite."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import velesdb_amd as va  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=100_000)
p.add_argument("--dim", type=int, default=768)
p.add_argument("--k", default="10,50,100")
p.add_argument("--queries", default="1,128,1024")
p.add_argument("--weight", type=float, default=0.5)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--block-ms", type=float, default=40.0)
p.add_argument("--out", default="")
p.add_argument("--per-query", default="", help="numbers of distinct filters, e.g. 1,16,128,1024: the per-query leg instead of the table")
p.add_argument("--walk-rows", default="f32,f16,int8,f16_rescore", help="rows forms of the per-query leg")
p.add_argument("--density", type=float, default=0.1)
a = p.parse_args()
WALK_ROWS = {"f32": va.WALK_ROWS_F32, "f16": va.WALK_ROWS_F16, "bf16": va.WALK_ROWS_BF16, "int8": va.WALK_ROWS_INT8,
             "f16_rescore": va.WALK_ROWS_F16_RESCORE, "bf16_rescore": va.WALK_ROWS_BF16_RESCORE}


def host_model():
    so = os.path.join(tempfile.gettempdir(), "vdb_hybrid_probe_%d" % os.getuid(), "libhybrid_model_o2.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "hybrid_model.cpp")])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.hybrid_model_fuse_batch.restype, L.hybrid_model_fuse_batch.argtypes = C.c_int, [vp, vp, u32, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    return L


def timed(fn):
    fn()
    t0 = time.perf_counter()
    fn()
    once = max(time.perf_counter() - t0, 1e-6)
    calls = max(1, int(a.block_ms / 1e3 / once))
    blocks = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        blocks.append((time.perf_counter() - t0) / calls * 1e3)
    med = statistics.median(blocks)
    return med, (max(blocks) - min(blocks)) / med


def alternating(fns):
    """{name: fn} timed in alternating blocks on one handle: per name the median over --repeats blocks and (max - min) / median"""
    calls = {}
    for name, fn in fns.items():
        fn()
        t0 = time.perf_counter()
        fn()
        calls[name] = max(1, int(a.block_ms / 1e3 / max(time.perf_counter() - t0, 1e-6)))
    blocks = {name: [] for name in fns}
    for _ in range(a.repeats):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                fn()
            blocks[name].append((time.perf_counter() - t0) / calls[name] * 1e3)
    return {name: (statistics.median(b), (max(b) - min(b)) / statistics.median(b), b) for name, b in blocks.items()}


def per_query_leg(ix, rng):
    k = int(a.k.split(",")[0])
    nq = max(int(x) for x in a.queries.split(","))
    kf = max(4 * k, k + 10)
    forms = [x for x in a.walk_rows.split(",") if x]
    if any("f16" in x for x in forms):
        ix.enable_half_precision(va.VectorPrecision.F16)
    if any("bf16" in x for x in forms):
        ix.enable_half_precision(va.VectorPrecision.BF16)
    if "int8" in forms:
        ix.train_quantizer()
    qs = rng.standard_normal((nq, a.dim)).astype(np.float32)
    text = rng.integers(0, a.rows, size=(nq, kf)).astype(np.uint64)
    w = np.full(nq, a.weight, dtype=np.float32)
    records = []
    print(f"# per-query filters: {nq} user queries, k {k}, text lists of {kf} ids, filters of density {a.density}")
    print("      F  side           ms (spread)   / loop")
    for F in [int(x) for x in a.per_query.split(",")]:
        flts = [ix.create_filter(rng.choice(a.rows, size=max(1, int(a.density * a.rows)), replace=False).astype(np.uint64)) for _ in range(F)]
        of = np.arange(nq) % F
        per = [flts[i] for i in of]
        groups = [np.flatnonzero(of == f) for f in range(F)]
        state = {}

        def loop():
            ids = np.empty((nq, k), np.uint64)
            sc = np.empty((nq, k), np.float32)
            cnt = np.empty(nq, np.uint32)
            for f, g in enumerate(groups):
                if g.size:
                    ids[g], sc[g], cnt[g] = ix.hybrid_search_batch(qs[g], text[g], k, w[g], flts[f])
            state["loop"] = (ids, sc, cnt)

        fns = {"loop": loop}
        for name in forms:
            fns["new " + name] = (lambda r: lambda: state.__setitem__(r, ix.hybrid_search_batch_filters(qs, text, k, w, per, WALK_ROWS[r])))(name)
        if F == 1:
            fns["one"] = lambda: ix.hybrid_search_batch(qs, text, k, w, flts[0])
        loop()
        if "f32" in forms:
            fns["new f32"]()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(state["loop"], state["f32"])), "the call and the loop differ"
        res = alternating(fns)
        for name, (med, spread, blocks) in res.items():
            records.append({"filters": F, "side": name, "ms": med, "spread": spread, "blocks_ms": blocks})
            print(f"{F:7d}  {name:14s} {med:9.3f} ({spread:5.2f})  {med / res['loop'][0]:7.3f}")
        for f in flts:
            f.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": va.device_name(0), "rows": a.rows, "dim": a.dim, "queries": nq, "k": k, "density": a.density,
                       "vector_weight": a.weight, "per_query": records}, f, indent=1)


def main():
    rng = np.random.default_rng(42)
    rows = rng.standard_normal((a.rows, a.dim)).astype(np.float32)
    ix = va.HnswIndex(a.dim, va.DistanceMetric.Cosine, va.HnswParams(32, 400, a.rows))
    ix.upload(np.arange(a.rows, dtype=np.uint64), rows)
    t0 = time.perf_counter()
    ix.build_graph()
    print(f"# {va.device_name(0)}: {a.rows} x {a.dim} cosine, graph built in {time.perf_counter() - t0:.1f} s, vector_weight {a.weight}")
    if a.per_query:
        return per_query_leg(ix, rng)
    L = host_model()
    table = []
    print("    k  queries  fused ms (spread)   host ms (spread)   of which host fusion ms   fused / host")
    for k in [int(x) for x in a.k.split(",")]:
        kf = 2 * k
        for nq in [int(x) for x in a.queries.split(",")]:
            qs = rng.standard_normal((nq, a.dim)).astype(np.float32)
            vids, _, vcnt = ix._search_raw(qs, kf, 0, va.MODE_HNSW)
            # 2k text hits per query: about half from the query's own vector list, the rest random live ids; shuffled
            text = np.empty((nq, kf), dtype=np.uint64)
            for q in range(nq):
                own = rng.permutation(vids[q, :int(vcnt[q])])[:kf // 2]
                rest = rng.integers(0, a.rows, size=kf - own.size).astype(np.uint64)
                text[q] = rng.permutation(np.concatenate([own, rest]))
            tn = np.full(nq, kf, dtype=np.uint32)
            w = np.full(nq, a.weight, dtype=np.float32)
            oi = np.empty((nq, k), dtype=np.uint64)
            ob = np.empty((nq, k), dtype=np.uint32)
            on = np.empty(nq, dtype=np.uint32)
            state = {}

            def search():
                state["lists"] = ix._search_raw(qs, kf, 0, va.MODE_HNSW)

            def fuse_host():
                ids, _, cnt = state["lists"]
                rc = L.hybrid_model_fuse_batch(ids.ctypes.data, cnt.ctypes.data, ids.shape[1], text.ctypes.data, tn.ctypes.data, kf, w.ctypes.data, nq, k,
                                               oi.ctypes.data, ob.ctypes.data, on.ctypes.data)
                assert rc == 0

            def host():
                search()
                fuse_host()

            def fused():
                state["fused"] = ix.hybrid_search_batch(qs, text, k, w)

            host()
            fused()
            fi, fs, fn_ = state["fused"]
            assert np.array_equal(fn_, on) and np.array_equal(fi, oi) and np.array_equal(fs.view(np.uint32), ob), "the two sides differ"
            t_f, s_f = timed(fused)
            t_h, s_h = timed(host)
            t_hf, _ = timed(fuse_host)
            table.append({"k": k, "queries": nq, "fused_ms": t_f, "fused_spread": s_f, "host_ms": t_h, "host_spread": s_h, "host_fusion_ms": t_hf})
            print(f"{k:5d}  {nq:7d}  {t_f:9.3f} ({s_f:5.2f})  {t_h:9.3f} ({s_h:5.2f})  {t_hf:12.3f}             {t_f / t_h:6.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": va.device_name(0), "rows": a.rows, "dim": a.dim, "vector_weight": a.weight, "table": table}, f, indent=1)


if __name__ == "__main__":
    main()
