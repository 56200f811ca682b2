"""Device-resident step sequences: `vdb_hip_index_search_batch_dev` called back to back on one handle, a different query slice per
step, on a caller's stream, with no host synchronisation in between — what bench.py measures and the Rust shim binds — and EVERY
step's ids, score bits and counts held to the oracle, not only the last one's.

What a handle carries from one call to the next, and what only a sequence can show an error in: the verdict block in pinned host
memory that the device writes and the next call reads without waiting, the four hold counters (csrc/vdb_select_hold.hpp), scratch
that grows with nq and k while earlier steps are still in flight, images built at first use on the caller's stream, scratch shared
between the WIDE selection and the gathered fallback.  `run_sequence` gives every step its own poisoned output buffers between two
guard rows, enqueues the lot, synchronises once, and compares.

The bar is bit equality with oracle/pyoracle.py in the mode the handle reports (`sweep_arith_mode`), with one exception the existing
tests of that mode state: Cosine / DotProduct over a half image, whose matrix instruction sums in an undocumented order — there the
rule and the constant of tests/test_gpu_half_precision.py (`check`, `TOL`) apply.

`vdb_hip_batch_distance_dev` (the host variant stages into aligned buffers, so only this entry reaches the scalar path of a
dim % 4 == 0 row) is covered at the end.
"""
import numpy as np
import pytest

import half_ref as hr
import half_walk_ref as hw
import test_gpu_half_precision as thp
from oracle import pyoracle as po
from select_hold_traces import CALLS, TRACES

pytestmark = pytest.mark.gpu

va = pytest.importorskip("velesdb_amd")
DM = va.DistanceMetric
VP = va.VectorPrecision
SM = va.StorageMode
PM = {DM.Cosine: po.COSINE, DM.Euclidean: po.EUCLIDEAN, DM.DotProduct: po.DOT, DM.Hamming: po.HAMMING, DM.Jaccard: po.JACCARD}

N, DIM = 66_000, 128        # the smallest corpus the selection stage takes: n >= 65 536, dim % 64 == 0, dim >= 128
POISON_ID, POISON_SCORE, POISON_COUNT = 0xDEADDEADDEADDEAD, 0x7FC0DEAD, 0xFFFFFFFE   # (the score: a NaN with a payload)
OVERFLOW = 0xFFFFFFFF       # d_out_n of a graph walk whose candidate list overflowed (include/velesdb_hip.h)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poisoned(torch, shape, value, np_type, as_type):
    return torch.from_numpy(np.full(shape, value, dtype=np_type).view(as_type)).cuda()


# ---- the oracle, once per distinct (queries, k, mode) ------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_rows(tag, compute, pool, lo, hi):
    """compute(queries) -> (ids, scores) over the first queries of `pool`, cached under `tag` and cut to [lo, hi)"""
    have = _ORACLE.get(tag)
    if have is None or have[0].shape[0] < hi:
        upto = min(pool.shape[0], (hi + 63) // 64 * 64)
        have = _ORACLE[tag] = compute(pool[:upto])
    return have[0][lo:hi], have[1][lo:hi]


def arith(ix, k):
    return po.MODE_M if ix.sweep_arith_mode(k) == "M" else po.MODE_C


def exact(eid, esc, ecnt=None):
    """The checker of a step whose answer is known bit for bit: counts, then ids and score bits of the first count entries per query."""
    eid, eb = np.ascontiguousarray(eid, dtype=np.uint64), bits(esc)
    cnt = np.full(eid.shape[0], eid.shape[1], np.uint32) if ecnt is None else np.asarray(ecnt, np.uint32)

    def check(gid, gsc, gcnt, msg):
        assert not np.any(gcnt == OVERFLOW), f"{msg}: overflow marker in the counts"
        assert np.array_equal(gcnt, cnt), f"{msg}: counts {gcnt[:8]} ..., expected {cnt[:8]} ..."
        m = np.arange(eid.shape[1])[None, :] < cnt[:, None]
        bad = np.nonzero(np.any((gid != eid) & m, axis=1) | np.any((bits(gsc) != eb) & m, axis=1))[0]
        assert bad.size == 0, (f"{msg}: {bad.size} of {eid.shape[0]} queries differ from the oracle, first {bad[0]}: ids {gid[bad[0]][:6]} / "
                               f"{eid[bad[0]][:6]}, score bits {bits(gsc)[bad[0]][:4]} / {eb[bad[0]][:4]}")
    return check


def brute_check(ix, tag, metric, rows, pool, lo, hi, k):
    mode = arith(ix, k)
    nt = po.host_threads()
    return exact(*oracle_rows((tag, int(metric), k, mode), lambda q: po.scan_topk(PM[metric], rows, q, k, mode, nthreads=nt), pool, lo, hi))


class Step:
    """One call: `nq` queries from row `lo` of the device pool `dpool` (numpy twin `pool`), checked by `check(ids, scores, counts, msg)`.
    host = True: the host entry (vdb_hip_index_search_batch) in the middle of the sequence instead."""

    def __init__(self, dpool, pool, lo, nq, k, check, mode=va.MODE_BRUTE, ef=0, host=False, name=""):
        self.dpool, self.pool, self.lo, self.nq, self.k, self.check, self.mode, self.ef, self.host = dpool, pool, lo, nq, k, check, mode, ef, host
        self.name = name or f"mode {mode}"


def run_sequence(ix, steps, stream, after_enqueue=None):
    """Enqueues every step on `stream` with no host synchronisation in between (`after_enqueue(i)`, if given, may add one), synchronises
    once, compares every step with its oracle and every guard row with the poison.  Returns the trace of last_select_level()."""
    import torch
    bufs = []
    for s in steps:
        kk = max(s.k, 1)
        bufs.append(None if s.host else (poisoned(torch, (s.nq + 2, kk), POISON_ID, np.uint64, np.int64),
                                         poisoned(torch, (s.nq + 2, kk), POISON_SCORE, np.uint32, np.float32),
                                         poisoned(torch, (s.nq + 2,), POISON_COUNT, np.uint32, np.int32)))
    torch.cuda.synchronize()
    levels, host_out = [], {}
    for i, s in enumerate(steps):
        row_bytes = s.dpool.shape[1] * 4
        d_q = s.dpool.data_ptr() + s.lo * row_bytes
        assert d_q % 16 == 0 and s.lo + s.nq <= s.dpool.shape[0]
        if s.host:
            host_out[i] = ix._search_raw(np.ascontiguousarray(s.pool[s.lo:s.lo + s.nq]), s.k, s.ef, s.mode)
        else:
            ids, sc, cnt = bufs[i]
            ix.search_batch_dev(d_q, s.nq, s.k, s.ef, s.mode, ids[1:].data_ptr(), sc[1:].data_ptr(), cnt[1:].data_ptr(), stream.cuda_stream)
        levels.append(ix.last_select_level())     # host state: no synchronisation
        if after_enqueue is not None:
            after_enqueue(i)
    stream.synchronize()
    for i, s in enumerate(steps):
        msg = f"step {i} of {len(steps)} ({s.name}, nq {s.nq}, k {s.k}, queries from {s.lo}); level trace {levels}"
        if s.host:
            s.check(*host_out[i], msg)
            continue
        ids, sc, cnt = (t.cpu().numpy() for t in bufs[i])
        ids, sc, cnt = ids.view(np.uint64), sc.view(np.uint32), cnt.view(np.uint32)
        for g in (0, -1):
            assert np.all(ids[g] == POISON_ID) and np.all(sc[g] == POISON_SCORE) and cnt[g] == POISON_COUNT, f"{msg}: guard row {g} was written"
        assert not np.any(cnt[1:-1] == POISON_COUNT), f"{msg}: counts were not written"
        s.check(ids[1:-1], sc[1:-1].view(np.float32), cnt[1:-1], msg)
    return levels


@pytest.fixture(scope="module")
def gauss():
    """N(0,1) rows and a pool of 320 queries, with their device twin"""
    import torch
    rng = np.random.default_rng(2024)
    rows = rng.standard_normal((N, DIM), dtype=np.float32)
    pool = rng.standard_normal((320, DIM), dtype=np.float32)
    return rows, pool, torch.from_numpy(pool).cuda()


def handle(metric, rows):
    ix = va.HnswIndex(rows.shape[1], metric, va.HnswParams(8, 50, rows.shape[0]))
    ix.upload(np.arange(rows.shape[0], dtype=np.uint64), rows)
    return ix


# ---- bench.py's own step rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [DM.Cosine, DM.DotProduct, DM.Euclidean])
def test_bench_shaped_steps(gpu_required, gauss, metric, k):
    import torch
    rows, pool, dpool = gauss
    Q, npool = 64, 256          # bench.py: a pool of 4 Q queries, step i takes the Q queries at (i * Q) % (pool - Q + 1)
    ix = handle(metric, rows)
    try:
        steps = []
        for i in range(12):
            off = (i * Q) % (npool - Q + 1)
            steps.append(Step(dpool, pool, off, Q, k, brute_check(ix, "gauss", metric, rows, pool[:npool], off, off + Q, k), name=str(metric)))
        levels = run_sequence(ix, steps, torch.cuda.Stream())
        assert levels[-1] == 4, f"level trace {levels}"
    finally:
        ix.close()


# ---- nq and k change from step to step: scratch regrowth with earlier steps in flight, the WIDE / exact boundary at k = 128 | 129, the
# ---- selection / exact boundary at nq = 16 | 15 -------------------------------------------------------------------------------------------
SHAPES = [(64, 10), (17, 50), (300, 1), (16, 128), (15, 10), (1, 10), (64, 129), (256, 100), (64, 10)]


@pytest.mark.parametrize("metric", [DM.Cosine, DM.Euclidean])
def test_shapes_change_in_flight(gpu_required, gauss, metric):
    import torch
    rows, pool, dpool = gauss
    ix = handle(metric, rows)
    try:
        steps = []
        for i, (nq, k) in enumerate(SHAPES):
            off = 0 if nq >= 256 else (i * 7) % (64 - min(nq, 63))       # every step another slice (a row of dim 128 is 512 bytes: aligned)
            steps.append(Step(dpool, pool, off, nq, k, brute_check(ix, "gauss", metric, rows, pool, off, off + nq, k), name=str(metric)))
        levels = run_sequence(ix, steps, torch.cuda.Stream())
        # below 16 queries and above k = 128 the exact kernels answer whatever the handle has seen before
        assert levels[0] == 4 and levels[4:7] == [0, 0, 0], f"level trace {levels}"
    finally:
        ix.close()


# ---- the exact modes of one handle interleaved; images built at first use in mid-sequence ----------------------------------------------------
def half_check(prec, rows, pool, lo, nq, k):
    """Cosine over a half image: the tolerance rule of tests/test_gpu_half_precision.py (its `check`, its TOL) on a sample of the batch"""
    def check(gid, gsc, gcnt, msg):
        assert np.all(gcnt == k), msg
        try:
            thp.check(hr.COSINE, prec, rows, pool[lo:lo + nq], k, gid, gsc, gcnt, sample=np.arange(0, nq, max(1, nq // 6)))
        except AssertionError as e:
            raise AssertionError(f"{msg}: {e}") from e
    return check


def test_modes_interleaved_on_one_handle(gpu_required, gauss):
    import torch
    rows, pool, dpool = gauss
    nt = po.host_threads()
    k = 10
    a = handle(DM.Cosine, rows)          # f32 rows + both half images + the SQ8 codes: four modes on one handle
    b = handle(DM.Euclidean, rows)       # one storage mode at a time: the sign-bit codes live on a second handle
    try:
        a.enable_bf16()
        a.enable_half_precision(VP.F16)
        a.set_storage_mode(SM.SQ8)
        b.set_storage_mode(SM.Binary)

        def step_a(mode, lo, nq, host=False):
            if mode == va.MODE_BRUTE:
                chk = brute_check(a, "gauss", DM.Cosine, rows, pool, lo, lo + nq, k)
            elif mode == va.MODE_BRUTE_SQ8:
                chk = exact(*oracle_rows(("gauss-sq8", k), lambda q: po.scan_topk_sq8(po.COSINE, rows, q, k, nthreads=nt), pool, lo, lo + nq))
            else:
                chk = half_check(hr.BF16 if mode == va.MODE_BRUTE_BF16 else hr.F16, rows, pool, lo, nq, k)
            return Step(dpool, pool, lo, nq, k, chk, mode=mode, host=host)

        def step_b(mode, lo, nq, host=False):
            if mode == va.MODE_BRUTE:
                chk = brute_check(b, "gauss", DM.Euclidean, rows, pool, lo, lo + nq, k)
            else:
                chk = exact(*oracle_rows(("gauss-binary", k), lambda q: po.scan_topk_binary(rows, q, k), pool, lo, lo + nq))
            return Step(dpool, pool, lo, nq, k, chk, mode=mode, host=host)

        B, B16, F16, SQ8, BIN = va.MODE_BRUTE, va.MODE_BRUTE_BF16, va.MODE_BRUTE_F16, va.MODE_BRUTE_SQ8, va.MODE_BRUTE_BINARY
        # round 1 over queries 0 ... 63 (every selection image is built at its first use, with the steps before it in flight), one
        # host-entry call, round 2 over queries 64 ... 127 in another order
        seq_a = [step_a(m, 0, 64) for m in (B, B16, F16, SQ8)] + [step_a(B, 128, 32, host=True)] + [step_a(m, 64, 64) for m in (SQ8, F16, B, B16)]
        seq_b = [step_b(m, 0, 64) for m in (BIN, B)] + [step_b(B, 128, 32, host=True)] + [step_b(m, 64, 64) for m in (B, BIN)]
        la = run_sequence(a, seq_a, torch.cuda.Stream())
        lb = run_sequence(b, seq_b, torch.cuda.Stream())
        print(f"level traces: {la} {lb}")
        assert la[0] == 4 and lb[1] == 4, (la, lb)       # (each handle's first f32 batch took the selection stage)
    finally:
        a.close()
        b.close()


# ---- the graph walks of one handle interleaved ------------------------------------------------------------------------------------------------
def test_graph_modes_interleaved(gpu_required, tmp_path):
    import torch
    n, dim, M, efc, k, ef = 3000, 64, 8, 60, 10, 64
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((n, dim)).astype(np.float32)     # (no two distances tie: no candidate list overflows)
    pool = rng.standard_normal((300, dim)).astype(np.float32)
    dpool = torch.from_numpy(pool).cuda()
    g = hw.build_graph(rows, hr.EUCLIDEAN, M, efc)
    d32, d16 = str(tmp_path / "f32"), str(tmp_path / "f16")
    (tmp_path / "f32").mkdir()
    g.file_dump(d32, "native_hnsw")
    hw.patch_vectors(d32, d16, "native_hnsw", hr.F16)
    g16 = hw.load_graph(d16, "native_hnsw", hr.EUCLIDEAN, dim)      # the same links over the rounded rows
    ix = va.HnswIndex(dim, DM.Euclidean, va.HnswParams(M, efc, n))
    try:
        ix.load_reference_files(d32, "native_hnsw")
        ix.train_quantizer()
        ix.enable_half_precision(VP.F16)
        sq = po.ScalarQuantizer(rows[:1000])
        codes = sq.quantize(rows)

        def padded(id_lists, bit_lists):
            ids, sb = np.zeros((len(id_lists), k), np.uint64), np.zeros((len(id_lists), k), np.uint32)
            for i, (a, b) in enumerate(zip(id_lists, bit_lists)):
                ids[i, :len(a)], sb[i, :len(a)] = a, b
            return ids, sb.view(np.float32), np.array([len(a) for a in id_lists], np.uint32)

        def f32_walk(q):
            oid, obits, _ = hw.oracle_walk(g, hr.EUCLIDEAN, q, k, ef)
            return padded(oid, obits)

        def f16_walk(q):
            oid, obits, _ = hw.oracle_walk(g16, hr.EUCLIDEAN, hr.round_half(q, hr.F16), k, ef)
            return padded(oid, obits)

        def int8_walk(q):
            oid, obits = [], []
            for one in q:
                i, d, _, _ = po.dual_search_int8(g, sq, codes, one, k, ef, 4, po.TIE_CANONICAL)
                oid.append(i.tolist())
                obits.append(bits([po.transform_score(po.EUCLIDEAN, float(x)) for x in d]))
            return padded(oid, obits)

        walks = {va.MODE_HNSW: f32_walk, va.MODE_HNSW_INT8: int8_walk, va.MODE_HNSW_F16: f16_walk}
        whole = {m: w(pool) for m, w in walks.items()}             # once per mode over the whole pool; a step checks its slice
        steps = []
        for i in range(12):                                         # 3 modes x 4 batch sizes: every pair once
            mode, nq = (va.MODE_HNSW, va.MODE_HNSW_INT8, va.MODE_HNSW_F16)[i % 3], (1, 7, 64, 300)[i % 4]
            lo = 0 if nq == 300 else 11 * i
            eid, esc, ecnt = (x[lo:lo + nq] for x in whole[mode])
            assert np.all(ecnt == k)
            steps.append(Step(dpool, pool, lo, nq, k, exact(eid, esc, ecnt), mode=mode, ef=ef))
        run_sequence(ix, steps, torch.cuda.Stream())
    finally:
        ix.close()


# ---- batches that defeat the selection in the middle of a sequence: when the hold starts depends on timing, the bits never do ---------------
@pytest.mark.parametrize("metric,k", [(DM.Cosine, 10), (DM.Cosine, 20), (DM.Euclidean, 10)])
def test_defeating_batches_mid_sequence(gpu_required, gauss, metric, k):
    import torch
    rng = np.random.default_rng(31)
    rows = gauss[0].copy()
    centre = rng.standard_normal(DIM).astype(np.float32)
    rows[60_000:] = centre + 1e-3 * rng.standard_normal((N - 60_000, DIM)).astype(np.float32)      # a cluster tighter than the bound
    pool = np.concatenate([gauss[1][:64], centre + 1e-3 * rng.standard_normal((32, DIM)).astype(np.float32)])  # good A, good B, bad
    dpool = torch.from_numpy(pool).cuda()
    ix = handle(metric, rows)
    try:
        tag = f"cluster6000-{int(metric)}-{k}"
        chk = {name: brute_check(ix, tag, metric, rows, pool, lo, lo + 32, k) for name, lo in (("bad", 64), ("A", 0), ("B", 32))}
        lo = {"A": 0, "B": 32, "bad": 64}
        order = ["A", "A", "bad"] + ["A", "B"] * 35 + ["bad", "A"]
        steps = [Step(dpool, pool, lo[s], 32, k, chk[s], name=s) for s in order]
        levels = run_sequence(ix, steps, torch.cuda.Stream())
        assert levels[0] == 4, f"level trace {levels}"
    finally:
        ix.close()


# ---- the hold, entered and left: one synchronisation per call makes the trace deterministic -------------------------------------------------
@pytest.fixture(scope="module")
def one_cluster():
    import torch
    rng = np.random.default_rng(5)
    centre = rng.standard_normal(DIM).astype(np.float32)
    rows = centre + 1e-4 * rng.standard_normal((N, DIM)).astype(np.float32)
    pool = rng.standard_normal((32, DIM), dtype=np.float32)
    return rows, pool, torch.from_numpy(pool).cuda()


@pytest.mark.parametrize("config", sorted(TRACES))
def test_hold_trace_with_a_sync_per_call(gpu_required, one_cluster, config):
    """A corpus that is one tight cluster defeats every selection level.  With each call finished before the next is enqueued, the
    level that answers call i is fixed by the rules of csrc/vdb_select_hold.hpp alone: tests/select_hold_traces.py, the traces the
    CPU model (tests/test_select_hold_cpu.py) prints.  Call 65 is the first after WIDE's hold of 64 batches: the handle returns to the
    selection.  (Before each selector kept its own seen-sequence, WIDE consumed every verdict and the three k = 10 traces read
    4, then 64 x 2 / 2 / 3: the level below WIDE never parked.)  A hold counts search calls: the Euclidean calls at level 0 go to the
    vector-ALU sweep 8 queries at a time and ask the rules again for the 24 and the 16 that remain, which counts once.  Every call's
    bits are the oracle's whatever level answers."""
    import torch
    rows, pool, dpool = one_cluster
    metric = DM.Euclidean if config.startswith("euclidean") else DM.Cosine
    k = 20 if config.endswith("k20") else 10
    sq8 = config.startswith("sq8")
    ix = handle(metric, rows)
    try:
        if sq8:
            ix.set_storage_mode(SM.SQ8)
            nt = po.host_threads()
            chk = exact(*oracle_rows(("one-cluster-sq8", k), lambda q: po.scan_topk_sq8(po.COSINE, rows, q, k, nthreads=nt), pool, 0, 32))
        else:
            chk = brute_check(ix, "one-cluster", metric, rows, pool, 0, 32, k)
        steps = [Step(dpool, pool, 0, 32, k, chk, mode=va.MODE_BRUTE_SQ8 if sq8 else va.MODE_BRUTE, name=config) for _ in range(CALLS)]
        stream = torch.cuda.Stream()
        first = []

        def finish_the_call(i):
            stream.synchronize()
            if i == 0:
                first.append(ix.last_split_stats())

        levels = run_sequence(ix, steps, stream, after_enqueue=finish_the_call)
        queries, unproven = first[0]
        assert queries == 32 and unproven * 16 > queries, f"premise: call 0 left {unproven} of {queries} queries unproven"
        assert levels == TRACES[config], f"level trace {levels}"
    finally:
        ix.close()


# ---- vdb_hip_batch_distance_dev ----------------------------------------------------------------------------------------------------------------
KIND_ENGINE, KIND_RAW, KIND_SQUARED = 0, 1, 2      # enum vdb_distance_kind
KINDS = [(m, kind) for m in (DM.Cosine, DM.Euclidean, DM.DotProduct, DM.Hamming, DM.Jaccard) for kind in (KIND_ENGINE, KIND_RAW)] + [(DM.Euclidean, KIND_SQUARED)]


@pytest.mark.parametrize("metric,kind", KINDS)
def test_batch_distance_dev(gpu_required, metric, kind):
    """Every metric x kind the entry accepts, n in {1, 257} x dim in {1, 3, 128, 131}, at three placements — both pointers 16-byte
    aligned, the query 4 bytes past that, the rows 4 bytes past that (dim 128 then takes the scalar loads the host variant, which
    stages into aligned buffers, never reaches) — on a caller's stream, bit-equal to the oracle in mode C and so to the host entry."""
    import torch
    rng = np.random.default_rng(100 * int(metric) + kind)
    F_POISON = 0x7FC0BEEF
    stream = torch.cuda.Stream()
    eng = va.HipDistance(metric)
    cases = []
    for n in (1, 257):
        for dim in (1, 3, 128, 131):
            if metric in (DM.Hamming, DM.Jaccard):
                rows, q = (rng.random((n, dim)) > 0.6915).astype(np.float32), (rng.random(dim) > 0.6915).astype(np.float32)
            else:
                rows, q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
            if kind == KIND_ENGINE:
                want = po.batch_distance(PM[metric], q, rows, po.MODE_C)
            elif kind == KIND_RAW:
                want = po.batch_compute_distance(PM[metric], q, rows, po.MODE_C)
            else:
                want = np.float32([po.sql2(q, r, po.MODE_C) for r in rows])
            for q_off, r_off in ((4, 4), (5, 4), (4, 5)):          # in floats from a 16-byte boundary
                dq = torch.zeros(dim + 8, dtype=torch.float32, device="cuda")
                dr = torch.zeros(n * dim + 8, dtype=torch.float32, device="cuda")
                assert dq.data_ptr() % 16 == 0 and dr.data_ptr() % 16 == 0
                dq[q_off:q_off + dim] = torch.from_numpy(q).cuda()
                dr[r_off:r_off + n * dim] = torch.from_numpy(rows.reshape(-1)).cuda()
                out = poisoned(torch, (n + 2,), F_POISON, np.uint32, np.float32)
                cases.append((n, dim, q_off, r_off, dq, dr, out, want))
    empty = poisoned(torch, (4,), F_POISON, np.uint32, np.float32)
    torch.cuda.synchronize()
    for n, dim, q_off, r_off, dq, dr, out, _ in cases:
        pq, pr = dq.data_ptr() + 4 * q_off, dr.data_ptr() + 4 * r_off
        assert (pq % 16, pr % 16) == ((q_off % 4) * 4, (r_off % 4) * 4)
        eng.batch_distance_dev(pq, pr, n, dim, out.data_ptr() + 4, stream.cuda_stream, kind)
    n, dim, _, _, dq, dr, _, _ = cases[0]
    eng.batch_distance_dev(dq.data_ptr(), dr.data_ptr(), 0, dim, empty.data_ptr(), stream.cuda_stream, kind)   # n = 0: OK, nothing written
    stream.synchronize()
    assert np.all(empty.cpu().numpy().view(np.uint32) == F_POISON)
    for n, dim, q_off, r_off, _, _, out, want in cases:
        got = out.cpu().numpy().view(np.uint32)
        where = f"{metric} kind {kind} n {n} dim {dim} query +{4 * (q_off - 4)} B rows +{4 * (r_off - 4)} B"
        assert got[0] == F_POISON and got[-1] == F_POISON, f"{where}: a guard element was written"
        assert np.array_equal(got[1:-1], bits(want)), f"{where}: {got[1:5]} / {bits(want)[:4]}"
