"""Reference of the half-precision distances (half_precision.rs:94-101, 199-308) in numpy, exact by construction:

  * `x.astype(np.float16).astype(np.float32)` is IEEE round-to-nearest-even with overflow to +-inf beyond 65 504 and gradual underflow —
    what `half::f16::from_f32` does; bf16 is the upper half of the f32 pattern, rounded to nearest even (`half::bf16::from_f32`);
  * a loop over the dimension on f32 arrays, one multiply and one add per step (numpy never fuses them), is the reference's
    `iter().zip().map(..).sum()` chain bit for bit, vectorised over (query, row) pairs.

The oracle has no f16; tests/test_half_precision_cpu.py checks this module against the reference's own literals and against the
oracle's bf16 functions where they overlap.  BF16 Euclidean in the reference is `euclidean_auto` over the converted vectors (a SIMD
order); here it is the same sequential chain as F16 — tests compare it by tolerance, and bit for bit only where every partial sum is
exact (then the order does not matter).
"""
import numpy as np

F32, F16, BF16 = 0, 1, 2            # VectorPrecision (half_precision.rs:36-44)
COSINE, EUCLIDEAN, DOT = 0, 1, 2    # DistanceMetric discriminants
F32_EPSILON = np.float32(1.1920929e-07)


def round_half(x, precision):
    """The f32 values a VectorData of `precision` holds for the f32 input x."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if precision == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    if precision == BF16:
        u = x.view(np.uint32).astype(np.uint64)
        nan = (u & 0x7FFFFFFF) > 0x7F800000
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        r = np.where(nan, ((u >> 16) | 0x40) << 16, r)
        return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(x.shape)
    return x.copy()


def seq_dot(q, r):
    """[nq, n] sequential f32 sums of q[i] * r[i] (half_precision.rs:210-214)."""
    acc = np.zeros((q.shape[0], r.shape[0]), np.float32)
    rt = np.ascontiguousarray(r.T)
    with np.errstate(all="ignore"):
        for i in range(q.shape[1]):
            acc = acc + q[:, i, None] * rt[i][None, :]
    return acc


def seq_l2(q, r):
    """[nq, n] sqrt of the sequential f32 sums of (q[i] - r[i])^2, the difference taken in f32 (half_precision.rs:274-279)."""
    acc = np.zeros((q.shape[0], r.shape[0]), np.float32)
    rt = np.ascontiguousarray(r.T)
    with np.errstate(all="ignore"):
        for i in range(q.shape[1]):
            d = q[:, i, None] - rt[i][None, :]
            acc = acc + d * d
        return np.sqrt(acc)


def seq_norm(x):
    """sqrt of the sequential f32 sum of x[i]^2 per row (norm_squared, half_precision.rs:290-308)."""
    acc = np.zeros(x.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            acc = acc + x[:, i] * x[:, i]
        return np.sqrt(acc)


def scores(metric, precision, rows, qs):
    """[nq, n] f32 raw scores of the reference for rows and queries both rounded to `precision`."""
    r, q = round_half(rows, precision), round_half(qs, precision)
    if metric == EUCLIDEAN:
        return seq_l2(q, r)
    dot = seq_dot(q, r)
    if metric == DOT:
        return dot
    nq, nr = seq_norm(q), seq_norm(r)
    with np.errstate(all="ignore"):
        out = dot / (nq[:, None] * nr[None, :])
    tiny = (nq[:, None] < F32_EPSILON) | (nr[None, :] < F32_EPSILON)     # half_precision.rs:247-248
    return np.where(tiny, np.float32(0.0), out).astype(np.float32)


def total_order_key(s):
    """u32 keys whose unsigned order is f32::total_cmp order."""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def topk(sc, k, higher_is_better, alive=None):
    """Best-first (ids, scores) per query; equal scores by ascending row (the library's declared tie-break)."""
    n = sc.shape[1]
    kk = min(k, n if alive is None else int(alive.sum()))
    ids = np.zeros((sc.shape[0], k), np.uint64)
    out = np.zeros((sc.shape[0], k), np.float32)
    for qi in range(sc.shape[0]):
        key = total_order_key(sc[qi]).astype(np.uint64)
        if higher_is_better:
            key = np.uint64(0xFFFFFFFF) - key
        key = (key << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        if alive is not None:
            key = key[alive]
        best = np.sort(key)[:kk] & np.uint64(0xFFFFFFFF)
        ids[qi, :kk] = best
        out[qi, :kk] = sc[qi, best.astype(np.int64)]
    return ids, out, kk


def scan_topk(metric, precision, rows, qs, k, alive=None):
    return topk(scores(metric, precision, rows, qs), k, metric != EUCLIDEAN, alive)


def truth64(metric, precision, rows, qs):
    """float64 scores of the ROUNDED values and the scale a 1e-5 tolerance is relative to (absolute on a cosine, |q||v| on a dot
    product, the distance itself for Euclidean)."""
    r, q = round_half(rows, precision).astype(np.float64), round_half(qs, precision).astype(np.float64)
    if metric == EUCLIDEAN:
        q2, r2 = (q * q).sum(1), (r * r).sum(1)
        full = np.empty((q.shape[0], r.shape[0]))
        for i in range(q.shape[0]):            # difference form: the expanded form cancels for near rows, in f64 as well
            d = r - q[i]
            full[i] = np.sqrt((d * d).sum(1))
        del q2, r2
        return full, full.copy()
    full = q @ r.T
    scale = np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(r, axis=1)[None, :]
    if metric == COSINE:
        with np.errstate(all="ignore"):
            full = np.where(scale > 0, full / scale, 0.0)
        return full, np.ones_like(full)
    return full, scale
