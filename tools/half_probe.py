#!/usr/bin/env python3
"""GPU probe of the half-precision result modes (VDB_SEARCH_BRUTE_F16 / VDB_SEARCH_BRUTE_BF16), single MI355X, device-resident
queries and outputs.  Prints what DESIGN.md 4.5 quotes:

  1. F16 Cosine next to BF16 Cosine on ONE handle, 1 024 queries, k = 10: time per batch, several repeats of each, interleaved;
  2. half-row Euclidean (f16 and bf16 rows), ONE query, next to the f32 Euclidean single query of the same handle: time, GB/s of the
     bytes each reads, fraction of 8 TB/s;
  3. half-row Euclidean, 1 024 queries: time per batch.

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
p.add_argument("--nq", type=int, default=1024)
p.add_argument("--repeats", type=int, default=7)
a = p.parse_args()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
VP = va.VectorPrecision


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
    ix.enable_half_precision(VP.F16)
    ix.enable_half_precision(VP.BF16)
    return ix


def timed(ix, q, nq, mode, iters):
    ids = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
    sc = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ix.search_batch_dev(q.data_ptr(), nq, a.k, 0, mode, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, ids


def kernel_ms(ix, q, nq, mode):
    va.set_kernel_timing(True)
    timed(ix, q, nq, mode, 1)
    ms, launches = ix.last_kernel_ms()
    va.set_kernel_timing(False)
    return ms, launches


g = torch.Generator(device=dev)
g.manual_seed(43)
queries = torch.randn((a.nq, a.dim), generator=g, device=dev)

# ---- 1. F16 Cosine next to BF16 Cosine --------------------------------------------------------------------------------------------
ix = build(va.DistanceMetric.Cosine)
for mode in (va.MODE_BRUTE_BF16, va.MODE_BRUTE_F16):
    timed(ix, queries, a.nq, mode, 2)
runs = {va.MODE_BRUTE_BF16: [], va.MODE_BRUTE_F16: []}
for _ in range(a.repeats):
    for mode in (va.MODE_BRUTE_BF16, va.MODE_BRUTE_F16):
        ms, ids = timed(ix, queries, a.nq, mode, 5)
        runs[mode].append(ms)
        if mode == va.MODE_BRUTE_BF16:
            bf_ids = ids.cpu().numpy()
        else:
            f_ids = ids.cpu().numpy()
for mode, name in ((va.MODE_BRUTE_BF16, "bf16"), (va.MODE_BRUTE_F16, "f16 ")):
    r = np.array(runs[mode])
    print(f"cosine {name} result mode, {a.rows} x {a.dim}, {a.nq} queries, k = {a.k}: ms per batch (5 batches each, interleaved) "
          f"{' '.join('%.3f' % x for x in r)} | min {r.min():.3f} median {np.median(r):.3f} max {r.max():.3f} | kernels {ix.last_kernels():#x}"
          f" | {2.0 * a.rows * a.dim * a.nq / (np.median(r) * 1e-3) / 1e12:.0f} TFLOP/s", flush=True)
print("top-%d overlap of the f16 and bf16 answers: %.4f" % (a.k, float(np.mean([len(set(bf_ids[i]) & set(f_ids[i])) / a.k for i in range(a.nq)]))),
      flush=True)
ix.close()
del ix
torch.cuda.empty_cache()

# ---- 2. / 3. half-row Euclidean -------------------------------------------------------------------------------------------------------
ix = build(va.DistanceMetric.Euclidean)
stride2 = (a.dim + 7) // 8 * 8 * 2
for mode, name, row_bytes in ((va.MODE_BRUTE, "f32 rows (sweep_topk_f32)", a.dim * 4), (va.MODE_BRUTE_F16, "f16 rows (sweep_topk_half_l2)", stride2),
                              (va.MODE_BRUTE_BF16, "bf16 rows (sweep_topk_half_l2)", stride2)):
    timed(ix, queries, 1, mode, 3)
    r = np.array([timed(ix, queries, 1, mode, 20)[0] for _ in range(a.repeats)])
    kms, nl = kernel_ms(ix, queries, 1, mode)
    nbytes = a.rows * row_bytes
    print(f"euclidean ONE query, {name}: ms per call (20 calls each) {' '.join('%.4f' % x for x in r)} | min {r.min():.4f} median {np.median(r):.4f} | "
          f"sweep kernel alone {kms:.4f} ms x{nl} = {nbytes / (kms * 1e-3) / 1e9:.0f} GB/s of {nbytes / 1e9:.3f} GB "
          f"({nbytes / (kms * 1e-3) / 1e9 / 8000:.3f} of 8 TB/s) | kernels {ix.last_kernels():#x}", flush=True)
for mode, name in ((va.MODE_BRUTE_F16, "f16"), (va.MODE_BRUTE_BF16, "bf16")):
    timed(ix, queries, a.nq, mode, 1)
    r = np.array([timed(ix, queries, a.nq, mode, 1)[0] for _ in range(3)])
    print(f"euclidean {a.nq} queries, {name} rows (streaming difference chain, {-(-a.nq // 16)} corpus passes): ms per batch {' '.join('%.2f' % x for x in r)} | "
          f"kernels {ix.last_kernels():#x}", flush=True)
r = np.array([timed(ix, queries, a.nq, va.MODE_BRUTE, 1)[0] for _ in range(4)][1:])
print(f"euclidean {a.nq} queries, f32 rows (exact mode, selection stage): ms per batch {' '.join('%.2f' % x for x in r)} | kernels {ix.last_kernels():#x}", flush=True)
ix.close()
