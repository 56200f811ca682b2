#!/usr/bin/env python3
"""What does graph construction over the half-precision rows gain?  A probe, not a bar.

One data set — 100 000 x 768 Cosine, M 32, ef_construction of HnswParams::auto (400), the seeded device generator of bench.py's
graph leg (corpus seed 42, queries seed 43) — built on fresh handles with graph precision F32, F16 and BF16
(vdb_hip_index_set_graph_precision).  Per build, one line:

  * inserts/s over the wall time of build_graph (ends in a device synchronise);
  * build_stats: rows evaluated, distance phases, select_neighbors rows (per insert);
  * the fraction of HBM peak by the byte model of the build's precision: the rows search_layer gathers,
    (rows - select rows) x (bytes per element x stride + 4 for the Cosine norm), over the wall time;
  * recall@10 at ef 128 of the f32 walk and of the same-precision half walk on the finished graph, against the exact f32 top-10 of
    1 000 queries.

Rules of the measurement: a small build per precision first (code objects loaded, scratch allocated), then --rounds rounds of the
three builds in alternating order, every build printed — the spread between rounds is the noise a difference has to exceed.

    python tools/half_build_probe.py [--rows 100000] [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, as bench.py
D, M, K, EF, NQ = 768, 32, 10, 128, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the lines as JSON here")
    a = ap.parse_args()

    import numpy as np
    import torch
    import velesdb_amd as va

    if va.device_count() == 0:
        sys.exit("half_build_probe needs a GPU")
    VP, SQ = va.VectorPrecision, va.SearchQuality
    dev = torch.device("cuda:0")
    params = va.HnswParams.auto(D)
    assert params.max_connections == M, params
    efc = params.ef_construction
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    corpus = torch.randn((a.rows, D), generator=g, device=dev, dtype=torch.float32)
    g.manual_seed(43)
    queries = torch.randn((NQ, D), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def one(precision, n):
        ix = va.HnswIndex(D, va.DistanceMetric.Cosine, va.HnswParams(M, efc, n))
        try:
            ix.upload_dev(0, corpus.data_ptr(), n, stream)
            ix.enable_half_precision(VP.F16)               # both images on every handle: the three builds differ in the precision alone
            ix.enable_half_precision(VP.BF16)
            ix.set_graph_precision(precision)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.build_graph(0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rows, phases, nodes, sel = ix.build_stats()
            bpe = 4 if precision == VP.F32 else 2
            gather = (rows - sel) * (bpe * D + 4)
            gt, _, _ = ix.search_batch_brute_force(queries, K)

            def recall(res):
                return float(np.mean([len({r[0] for r in one_} & set(gt[i].tolist())) / K for i, one_ in enumerate(res)]))
            r32 = recall(ix.search_batch_parallel(queries, K, SQ.Custom(EF)))
            rp = r32 if precision == VP.F32 else recall(ix.search_batch_half_graph(queries, K, EF, precision))
            return {"graph_precision": precision.name, "rows": n, "build_seconds": round(dt, 3), "inserts_per_s": round(n / dt, 1),
                    "rows_evaluated_per_insert": round(rows / nodes, 1), "distance_phases_per_insert": round(phases / nodes, 1),
                    "select_rows_per_insert": round(sel / nodes, 1), "gather_bytes_per_row": bpe * D + 4,
                    "hbm_gbs": round(gather / dt / 1e9, 1), "hbm_frac": round(gather / dt / 1e9 / HBM_PEAK_GBS, 4),
                    "recall_at_10_f32_walk": round(r32, 4), "recall_at_10_same_precision_walk": round(rp, 4)}
        finally:
            ix.close()

    order = [VP.F32, VP.F16, VP.BF16]
    for p in order:                                        # warm-up: every kernel family once, not reported
        one(p, min(a.rows, 4000))
    lines = []
    for r in range(a.rounds):
        for p in (order if r % 2 == 0 else order[::-1]):
            line = dict(one(p, a.rows), round=r, device=va.device_name(0), M=M, ef_construction=efc, ef=EF, queries=NQ)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
