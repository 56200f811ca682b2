#!/usr/bin/env python3
"""GPU probe of the graph search over the half-precision rows (VDB_SEARCH_HNSW_F16 / VDB_SEARCH_HNSW_BF16), single MI355X,
device-resident queries and outputs.  Prints what DESIGN.md 4.5b quotes: on ONE handle in ONE process, interleaved, the f32 walk
(VDB_SEARCH_HNSW, the comparison point), the two half walks and the int8 walk — queries per second, the kernel's own counters
(distance evaluations and expansions per query), each mode's algorithmic HBM bytes as a fraction of 8 TB/s, and recall@10 against the
exact f32 sweep of the same handle.

Corpora: --corpus gaussian (iid N(0,1): no neighbourhood structure, the gather-bound worst case) and --corpus embedding (the
low-rank + noise corpus of bench.py's recall leg, same generator arguments).

Not part of the product or the test-suite."""
import argparse
import os
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
p.add_argument("--nq", type=int, default=8192)
p.add_argument("--M", type=int, default=32)
p.add_argument("--efc", type=int, default=400)
p.add_argument("--ef", type=int, default=128)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--recall-queries", type=int, default=1000)
p.add_argument("--corpus", choices=("gaussian", "embedding"), default="gaussian")
p.add_argument("--latent", type=int, default=32)
p.add_argument("--latent-noise", type=float, default=0.25)
p.add_argument("--metric", choices=("cosine", "euclidean", "dot"), default="cosine")
a = p.parse_args()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
VP = va.VectorPrecision
metric = {"cosine": va.DistanceMetric.Cosine, "euclidean": va.DistanceMetric.Euclidean, "dot": va.DistanceMetric.DotProduct}[a.metric]
HBM = 8.0e12

g = torch.Generator(device=dev)
ix = va.HnswIndex(a.dim, metric, va.HnswParams(a.M, a.efc, a.rows))
if a.corpus == "gaussian":
    g.manual_seed(42)
    for base in range(0, a.rows, 250_000):
        n = min(250_000, a.rows - base)
        c = torch.randn((n, a.dim), generator=g, device=dev)
        torch.cuda.synchronize()
        ix.upload_dev(base, c.data_ptr(), n, st)
        torch.cuda.synchronize()
        del c
    g.manual_seed(43)
    queries = torch.randn((a.nq, a.dim), generator=g, device=dev)
else:  # bench.py's embedding-like leg
    g.manual_seed(44)
    proj = torch.randn((a.latent, a.dim), generator=g, device=dev)
    rows = torch.randn((a.rows, a.latent), generator=g, device=dev) @ proj
    rows += a.latent_noise * torch.randn((a.rows, a.dim), generator=g, device=dev)
    queries = torch.randn((a.nq, a.latent), generator=g, device=dev) @ proj
    queries += a.latent_noise * torch.randn((a.nq, a.dim), generator=g, device=dev)
    torch.cuda.synchronize()
    ix.upload_dev(0, rows.data_ptr(), a.rows, st)
    torch.cuda.synchronize()
    del rows
torch.cuda.empty_cache()
t0 = time.perf_counter()
ix.build_graph(0)
torch.cuda.synchronize()
print(f"{a.corpus} corpus {a.rows} x {a.dim}, {a.metric}, M {a.M}, ef_construction {a.efc}: graph built in {time.perf_counter() - t0:.1f} s", flush=True)
ix.enable_half_precision(VP.F16)
ix.enable_half_precision(VP.BF16)
ix.train_quantizer(0)

ids = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
sc = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
cnt = torch.empty((a.nq,), dtype=torch.int32, device=dev)


def batch(mode):
    torch.cuda.synchronize()
    t = time.perf_counter()
    ix.search_batch_dev(queries.data_ptr(), a.nq, a.k, a.ef, mode, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st)
    torch.cuda.synchronize()
    return time.perf_counter() - t


RQ = min(a.recall_queries, a.nq)
gt = ix.search_batch_brute_force(queries[:RQ].cpu().numpy(), a.k)[0]      # the exact f32 sweep
stride_half = (a.dim + 7) // 8 * 8
M0 = 2 * a.M
norm = 4 if a.metric == "cosine" else 0
modes = [("f32  (VDB_SEARCH_HNSW)", va.MODE_HNSW, lambda nd, ne: nd * (a.dim * 4 + norm) + ne * M0 * 4),
         ("f16  (VDB_SEARCH_HNSW_F16)", va.MODE_HNSW_F16, lambda nd, ne: nd * (2 * stride_half + norm) + ne * M0 * 4),
         ("bf16 (VDB_SEARCH_HNSW_BF16)", va.MODE_HNSW_BF16, lambda nd, ne: nd * (2 * stride_half + norm) + ne * M0 * 4),
         ("int8 (VDB_SEARCH_HNSW_INT8)", va.MODE_HNSW_INT8, lambda nd, ne: nd * (a.dim + 4) + ne * M0 * 4 + a.k * 4 * a.dim * 4)]
info = {}
for name, mode, alg in modes:                                             # warm-up + counters + recall, once per mode
    batch(mode)
    nd, ne = ix.last_search_stats()
    got = ids[:RQ].cpu().numpy().astype(np.uint64)
    rec = float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / a.k for i in range(RQ)]))
    info[mode] = (nd / a.nq, ne / a.nq, alg(nd, ne) / a.nq, rec, ix.last_kernels())
runs = {mode: [] for _, mode, _ in modes}
for _ in range(a.repeats):                                                # interleaved: every mode sees the same machine state
    for _, mode, _ in modes:
        runs[mode].append(batch(mode))
for name, mode, _ in modes:
    r = np.array(runs[mode])
    nd, ne, by, rec, kern = info[mode]
    med = float(np.median(r))
    print(f"{name}: {a.nq} queries, k {a.k}, ef {a.ef}: ms per batch {' '.join('%.2f' % (x * 1e3) for x in r)} | median {med * 1e3:.2f} ms = "
          f"{a.nq / med / 1e3:.1f} K q/s | n_dist {nd:.0f} n_expand {ne:.1f} per query | {by / 1e6:.2f} MB per query = "
          f"{by * a.nq / med / 1e12:.2f} TB/s = {by * a.nq / med / HBM:.3f} of 8 TB/s | recall@{a.k} {rec:.4f} ({RQ} queries, vs the exact f32 sweep) | "
          f"kernels {kern:#x}", flush=True)
ix.close()
