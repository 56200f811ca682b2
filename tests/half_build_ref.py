"""What the tests of graph construction over the half-precision rows share (vdb_hip_index_set_graph_precision, csrc/hnsw_build.hip:
hnsw_insert_half_kernel / hnsw_ndist_half_kernel).

With graph precision P every distance of construction is half_precision::* over the image rows in mode C's summation order, the
inserted node's query its own image row dequantised.  That is, bit for bit, the f32 construction over the f32 rows
round_half(rows, P) — the argument tests/half_walk_ref.py makes for the walk — so the reference needs no new oracle code: the oracle
graph for precision P is a mode-C NativeHnsw fed round_half(rows, P), by sequential `insert` or by `build_batched`, matching the GPU
call, and the comparison is link for link (tests/build_shapes.py assert_same_graph).

A graph whose precision changes while it has nodes has links chosen under one row format and distances taken under another from then
on.  The oracle gets there through its files: dump, rewrite the `.vectors` file with the rows of the new format, load, insert more
(`switch_oracle`).  A load restarts the level stream (backend_adapter.rs:373) and a live handle does not; `advance_level_stream` puts the
loaded oracle's stream where the live graph's stands, with the one call of the oracle that steps it without inserting.
"""
import functools
import os
import shutil

import numpy as np

import build_shapes as bs
import half_ref as hr
import half_walk_ref as hw
from oracle import pyoracle as po

BASE = "native_hnsw"
PRECISIONS = (hr.F16, hr.BF16)
PNAME = {hr.F32: "f32", hr.F16: "f16", hr.BF16: "bf16"}
METRICS = bs.FLOATS                                   # "cosine", "euclidean", "dot"
# (n, dim, M, efc): CPL 0 with dim % 4 != 0, CPL 0, CPL 1, 2, 3, 4, the LDS query between and above the register layouts
SHAPES = [(700, 37, 6, 40), (900, 96, 8, 60), (600, 256, 8, 60), (600, 512, 8, 60), (600, 768, 16, 100), (500, 1024, 8, 60),
          (400, 1536, 8, 40), (300, 4099, 6, 40)]
MAX_BATCH = 64                                        # build_graph(64): batches of 1, 1, ... 2, 3, ... 37 .. 56 of the linked / 16 schedule
MODES = ("sequential", "batched")
WALK_CASES = [("euclidean", SHAPES[0], hr.F16), ("cosine", SHAPES[4], hr.BF16), ("dot", SHAPES[5], hr.F16)]

# switching the precision of a live graph / after a load: M 6 so that layer-0 lists (12 links) are full long before the switch
SWITCH_N, SWITCH_MORE, SWITCH_DIM, SWITCH_M, SWITCH_EFC = 400, 300, 96, 6, 40
SWITCH_CASES = [("euclidean", hr.F32, hr.F16), ("cosine", hr.F32, hr.BF16), ("dot", hr.F32, hr.BF16),
                ("euclidean", hr.F16, hr.F32), ("cosine", hr.BF16, hr.F32)]
LOAD_CASES = [("euclidean", hr.F16), ("cosine", hr.BF16), ("dot", hr.F16)]
VACUUM_N, VACUUM_DIM, VACUUM_DEAD = 600, 48, 120      # a fifth removed; HnswParams::auto(48) = M 24, efc 300 (params.rs:41-57)


def rounded(rows, precision):
    """The f32 rows a construction of `precision` takes its distances over.  Every row norm is far above f32::EPSILON, so the
    reference's half-precision Cosine rule (`< EPSILON`, half_precision.rs:247) and the oracle's (`== 0`) agree."""
    r = hr.round_half(rows, precision)
    norms = np.sqrt((r.astype(np.float64) ** 2).sum(axis=1))
    assert np.isfinite(r).all() and norms.min() > 1e3 * float(hr.F32_EPSILON), norms.min()
    return r


def case_rows(metric, shape):
    n, dim, _M, _efc = shape
    rng = np.random.default_rng(4100 + dim + 17 * bs.METRIC[metric])
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((hw.NQ, dim)).astype(np.float32)


def build_oracle(rows, metric, M, efc, mode):
    g = bs.new_oracle(rows.shape[1], metric, M, efc)
    if mode == "sequential":
        for v in rows:
            g.insert(v)
    else:
        g.build_batched(rows, MAX_BATCH)
    return g


@functools.lru_cache(maxsize=None)
def case_oracle(metric, shape, precision, mode):
    """The oracle graph of one case, built once per process; precision F32 = the graph an implementation that ignored the graph
    precision would build."""
    _n, _dim, M, efc = shape
    return build_oracle(rounded(case_rows(metric, shape)[0], precision), metric, M, efc, mode)


def differing_lists(ga, gb, n):
    a, b = bs.layer0_lists(ga, n), bs.layer0_lists(gb, n)
    return sum(x != y for x, y in zip(a, b))


# ---- a graph whose rows change format under it -----------------------------------------------------------------------------------
def write_vectors(directory, basename, rows):
    """The `.vectors` file of format v1 (backend_adapter.rs:199-215) for `rows`."""
    rows = np.ascontiguousarray(rows, dtype="<f4")
    with open(os.path.join(directory, basename + ".vectors"), "wb") as f:
        f.write(np.uint32(1).tobytes() + np.uint64(rows.shape[0]).tobytes() + np.uint32(rows.shape[1]).tobytes())
        f.write(rows.tobytes())


def advance_level_stream(g, steps, probe):
    """Steps the oracle's level stream without inserting: search_multi_entry with two probes draws exactly one id from the stream
    random_layer advances (graph.rs:320-334), one xorshift step, like one level."""
    assert len(g) > 10                                 # (graph.rs:318: fewer nodes draw nothing)
    for _ in range(steps):
        g.search_multi_entry(probe, 1, 1, 2)


def switch_data(metric):
    rng = np.random.default_rng(8800 + 17 * bs.METRIC[metric])
    return (rng.standard_normal((SWITCH_N, SWITCH_DIM)).astype(np.float32),
            rng.standard_normal((SWITCH_MORE, SWITCH_DIM)).astype(np.float32))


def switch_oracle(metric, before, after, directory, live):
    """SWITCH_N rows linked one by one at precision `before`, SWITCH_MORE more at precision `after` -> (graph, pruned).
    live: the graph was never saved (set_graph_precision on a handle with nodes): the level stream goes on where it stood; otherwise
    it restarts, as after load_reference_files.  pruned = nodes whose layer-0 list was full at the switch and differs afterwards: a
    full list only changes through a prune, and a prune after the switch ranks the list by distances of the NEW precision
    (the reference recomputes them from the vectors it holds, graph.rs:608-637; the GPU refills its cache, graph_fill_ndist)."""
    rows, more = switch_data(metric)
    g0 = build_oracle(rounded(rows, before), metric, SWITCH_M, SWITCH_EFC, "sequential")
    d0, d1 = os.path.join(str(directory), "before"), os.path.join(str(directory), "after")
    os.makedirs(d0, exist_ok=True)
    os.makedirs(d1, exist_ok=True)
    g0.file_dump(d0, BASE)                              # (what a GPU handle loads in the after-load case: rows as they were)
    shutil.copyfile(os.path.join(d0, BASE + ".graph"), os.path.join(d1, BASE + ".graph"))
    write_vectors(d1, BASE, rounded(rows, after))
    g = bs.reload_oracle(d1, BASE, SWITCH_DIM, metric)
    if live:
        advance_level_stream(g, SWITCH_N, rows[0])
        assert g.rng_state() == g0.rng_state()
    start = bs.layer0_lists(g, SWITCH_N)
    assert start == bs.layer0_lists(g0, SWITCH_N)
    for v in rounded(more, after):
        g.insert(v)
    end = bs.layer0_lists(g, SWITCH_N)
    pruned = sum(len(a) == 2 * SWITCH_M and a != b for a, b in zip(start, end))
    return g, pruned, d0


def unswitched_oracle(metric, precision):
    """The same SWITCH_N + SWITCH_MORE rows at one precision throughout: what a switch that did nothing would build."""
    rows, more = switch_data(metric)
    return build_oracle(rounded(np.concatenate([rows, more]), precision), metric, SWITCH_M, SWITCH_EFC, "sequential")


def vacuum_data():
    rng = np.random.default_rng(91)
    rows = rng.standard_normal((VACUUM_N, VACUUM_DIM)).astype(np.float32)
    dead = rng.choice(VACUUM_N, VACUUM_DEAD, replace=False)
    live = np.ones(VACUUM_N, bool)
    live[dead] = False
    return rows, dead, live
