"""What the tests of the half-precision graph walk (VDB_SEARCH_HNSW_F16 / _BF16) share.

The walk's declared summation order is mode C of the f32 walk, so over an image H it must be bit for bit the oracle's mode-C
NativeHnsw::search over the f32 vectors dequant(H) with the rounded query.  Such an oracle graph is made without any new oracle
code: dump a graph built on the f32 rows (`file_dump`, format v1: backend_adapter.rs:184-261), rewrite the `.vectors` file with the
rounded rows and `file_load` it — same links, rounded vectors.
"""
import os
import shutil

import numpy as np

import half_ref as hr
from oracle import pyoracle as po

VECTORS_HEADER = 16  # u32 version = 1 | u64 count | u32 dim, little-endian; then count * dim raw f32 (backend_adapter.rs:199-215)
SHAPES = [(3000, 96, 8, 60), (1500, 768, 16, 100), (1200, 37, 6, 40)]  # (n, dim, M, efc): CPL 0 (dim % 256), CPL 3, dim % 4 != 0
# the register-chunk instances CPL 1 / 2 / 4, then dims whose query lives in LDS scratch (1 536, the default max_dimensions 4 096,
# and dim % 4 != 0 above the register layout): tests/test_gpu_large_dim_features.py, tests/test_gpu_int8.py
LARGE_SHAPES = [(1500, 256, 8, 60), (1500, 512, 8, 60), (1500, 1024, 8, 60),
                (1200, 1536, 8, 60), (1000, 4096, 8, 40), (1000, 4099, 6, 40)]
KEF = [(10, 64), (1, 16), (25, 50), (10, 300)]                        # ef > 192: the LDS list
NQ = 20
PO_METRIC = {hr.COSINE: po.COSINE, hr.EUCLIDEAN: po.EUCLIDEAN, hr.DOT: po.DOT}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def patch_vectors(src_dir, dst_dir, basename, precision):
    """Copy `basename`.graph and write `basename`.vectors with every float rounded to `precision`; returns the rounded rows."""
    os.makedirs(dst_dir, exist_ok=True)
    shutil.copyfile(os.path.join(src_dir, basename + ".graph"), os.path.join(dst_dir, basename + ".graph"))
    raw = open(os.path.join(src_dir, basename + ".vectors"), "rb").read()
    version, = np.frombuffer(raw, "<u4", 1, 0)
    count, = np.frombuffer(raw, "<u8", 1, 4)
    dim, = np.frombuffer(raw, "<u4", 1, 12)
    assert version == 1 and len(raw) == VECTORS_HEADER + int(count) * int(dim) * 4
    rows = np.frombuffer(raw, "<f4", int(count) * int(dim), VECTORS_HEADER).reshape(int(count), int(dim))
    rounded = hr.round_half(rows, precision)
    with open(os.path.join(dst_dir, basename + ".vectors"), "wb") as f:
        f.write(raw[:VECTORS_HEADER])
        f.write(rounded.astype("<f4").tobytes())
    return rounded


def load_graph(directory, basename, metric, dim):
    g = po.NativeHnsw.file_load(directory, basename, PO_METRIC[metric], po.MODE_C)
    g.dim = dim
    return g


def build_graph(rows, metric, M, efc):
    g = po.NativeHnsw(rows.shape[1], PO_METRIC[metric], M, efc, po.MODE_C)
    for v in rows:
        g.insert(v)
    return g


def grid(rng, shape, precision):
    """Values whose products, squares, differences and partial sums are all exact in f32 at dim <= 768, so every summation order of
    dot, norms and squared distance gives the same bits.  F16: m / 256 with integer |m| <= 64, and — rarely, < 1 % of the elements —
    +-(1 + 1/256), which f16 holds and bf16 does not: sums stay below 768 * 64^2 + 8 * 257^2 < 2^24 units of 2^-16.
    BF16: integers |m| <= 15."""
    if precision == hr.BF16:
        return rng.integers(-15, 16, shape).astype(np.float32)
    x = rng.integers(-64, 65, shape).astype(np.float32) / np.float32(256)
    special = rng.random(shape) < 0.008
    # at most 8 per row keep the bound above whatever the draw
    over = np.cumsum(special, axis=-1) > 8
    special &= ~over
    sign = np.where(rng.random(shape) < 0.5, np.float32(-1), np.float32(1))
    return np.where(special, sign * np.float32(1 + 1 / 256), x).astype(np.float32)


def oracle_walk(g, metric, qs_rounded, k, ef):
    """ids [nq][<=k], transformed score bits, (n_dist, n_expand) of NativeHnsw::search under HnswIndex's mapping (max(ef, k),
    transform_score), canonical tie order."""
    ids, ds, cnt, nd, ne = g.search_batch(qs_rounded, k, max(ef, k), po.TIE_CANONICAL)
    out_ids, out_bits = [], []
    for i in range(qs_rounded.shape[0]):
        c = int(cnt[i])
        out_ids.append(ids[i, :c].tolist())
        out_bits.append(bits([po.transform_score(PO_METRIC[metric], float(x)) for x in ds[i, :c]]))
    return out_ids, out_bits, (nd, ne)
