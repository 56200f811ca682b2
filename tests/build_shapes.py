"""Shapes for the link-for-link tests of graph construction (tests/test_gpu_build_shapes.py) and the oracle-only
checks that each shape still reaches the edge it was chosen for (tests/test_build_shapes_cpu.py).

Every case is built for one path of velesdb_amd/csrc/hnsw_build.hip (or of the link-request sort in radix_sort.hip) that
a 2 500-row Gaussian build never takes.  A case comes with a *condition*: a property of the oracle's graph that says the
path was taken — group sizes, zero-distance pairs, layer count, full-list share, visited counts, pruned-after-load counts.
The conditions are floors, not measurements: if one stops holding, the data has to change, not the floor.

Plain module, no fixtures: both test files import it, and the oracle graphs that nothing mutates are built once per
process (`oracle_build`).
"""
import functools
import struct

import numpy as np

from oracle import pyoracle as po

METRIC = {"cosine": po.COSINE, "euclidean": po.EUCLIDEAN, "dot": po.DOT, "hamming": po.HAMMING, "jaccard": po.JACCARD}
FLOATS = ("cosine", "euclidean", "dot")
BITS = ("hamming", "jaccard")
K, EF, NQ = 10, 64, 16          # the traversal every test runs over the finished graph

VLOG_CAP = 16384                # kVlogCap in hnsw_build.hip: visited nodes an insert can log before CMD_CLEAN clears the bitmap


def is_bits(metric):
    return metric in BITS


def data(rng, n, d, metric):
    """Gaussian rows, or dense bit rows like tests/test_gpu_build.py::data for Hamming / Jaccard."""
    if is_bits(metric):
        return (rng.random((n, d)) > 0.6915).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)


def new_oracle(dim, metric, M, efc):
    g = po.NativeHnsw(dim, METRIC[metric], M, efc, po.MODE_C)
    g.set_build_tie(po.TIE_CANONICAL)
    g.set_build_threads(po.host_threads())
    return g


def reload_oracle(directory, basename, dim, metric):
    """NativeHnsw::file_load: the level stream restarts (backend_adapter.rs:373), like load_reference_files on the GPU."""
    g = po.NativeHnsw.file_load(directory, basename, METRIC[metric], po.MODE_C)
    g.dim = dim
    g.set_build_tie(po.TIE_CANONICAL)
    g.set_build_threads(po.host_threads())
    return g


def schedule(n, max_batch, linked=0):
    """Batch sizes of a build of n rows on top of `linked` nodes: build_batch_size's rule (a sixteenth of the linked
    nodes, at least 1, at most max_batch; the library's 0 means 2 048), one node alone into an empty graph."""
    cap = max_batch if max_batch else 2048
    out = []
    while n:
        b = 1 if linked == 0 else min(max(linked // 16, 1), cap, n)
        out.append(b)
        linked += b
        n -= b
    return out


# ---- comparison ------------------------------------------------------------------------------------------------
def read_graph_file(path):
    """The .graph file of format v1 (backend_adapter.rs:184-261) -> (num_layers, max_layer, entry_point, count, lists) with
    lists[layer][node] a tuple of neighbour ids (nodes a layer does not hold read as empty)."""
    raw = open(path, "rb").read()
    version, num_layers, _M, _M0, _efc, ep, max_layer, count = struct.unpack_from("<IIIIIQIQ", raw, 0)
    assert version == 1
    off = 40
    lists = []
    for _ in range(num_layers):
        (nn,) = struct.unpack_from("<Q", raw, off)
        off += 8
        # one pass over the 32-bit words of the layer: [k, k ids] per node
        words = np.frombuffer(raw, dtype="<u4", offset=off, count=(len(raw) - off) // 4).tolist()
        layer, i = [], 0
        for _node in range(nn):
            k = words[i]
            layer.append(tuple(words[i + 1:i + 1 + k]))
            i += 1 + k
        off += 4 * i
        layer.extend(() for _ in range(count - nn))
        lists.append(layer)
    assert off == len(raw), "trailing bytes in the graph file"
    return num_layers, max_layer, ep, count, lists


def assert_same_graph(g, ix, n, via_files=None):
    """Entry point, max layer, number of layers and the adjacency list of every node on every layer.  `via_files`: a
    directory — both sides write the reference's file format there and the files are compared list by list; for the
    70 000-node cases, where one C ABI call per (layer, node) would cost more than the build."""
    nl, ml, ep = ix.graph_info()
    assert (ml, ep) == (g.max_layer, g.entry_point)
    assert nl == g.num_layers
    if via_files is None:
        for layer in range(g.num_layers):
            for node in range(n):
                a, b = ix.neighbors(layer, node), g.neighbors(layer, node)
                assert a == b, f"layer {layer} node {node}:\n gpu {a}\n ora {b}"
        return
    ix.save(str(via_files), "gpu")
    g.file_dump(str(via_files), "ora")
    gl, gm, ge, gc, glists = read_graph_file(f"{via_files}/gpu.graph")
    ol, om, oe, oc, olists = read_graph_file(f"{via_files}/ora.graph")
    assert (gl, gm, ge, gc) == (ol, om, oe, oc) == (g.num_layers, g.max_layer, g.entry_point, n)
    for layer in range(ol):
        if glists[layer] != olists[layer]:
            node = next(i for i in range(n) if glists[layer][i] != olists[layer][i])
            raise AssertionError(f"layer {layer} node {node}:\n gpu {list(glists[layer][node])}\n ora {list(olists[layer][node])}")


def assert_same_search(g, ix, qs, va):
    """NQ queries, k 10, ef 64 over the finished graph: ids == the oracle's search on its own graph."""
    res = ix.search_batch_parallel(qs, K, va.SearchQuality.Custom(EF))
    for i, (q, r) in enumerate(zip(qs, res)):
        oid, _ = g.search(q, K, EF, po.TIE_CANONICAL)
        assert [x[0] for x in r] == oid.tolist(), f"query {i}"


def layer0_lists(g, n):
    return [g.neighbors(0, i) for i in range(n)]


def full_share(g, n, M):
    """Share of layer-0 lists that hold all M0 = 2 M neighbours (graph.rs:62): only a full list is ever pruned."""
    return sum(len(x) == 2 * M for x in layer0_lists(g, n)) / n


# ---- 1. dim classes x metrics, batched -----------------------------------------------------------------------------
# CPL 1 / 2 / 4 (256 / 512 / 1024), the generic LDS-query layout below, between and above them, dims with dim % 4 != 0;
# one word, a ragged word and many words for the bit metrics
DIMS_FLOAT = (100, 256, 512, 1024, 1001, 1280, 2048, 4099)
DIMS_BITS = (31, 32, 33, 1000, 4099)
DIM_CASES = [(m, d) for m in FLOATS for d in DIMS_FLOAT] + [(m, d) for m in BITS for d in DIMS_BITS]
DIM_M, DIM_EFC, DIM_MB, DIM_MORE = 8, 40, 64, 200


def dim_case_n(dim):
    return 1500 if dim >= 2048 else 2500


def dim_case_data(metric, dim):
    rng = np.random.default_rng(1000 + dim + 17 * METRIC[metric])
    n = dim_case_n(dim)
    return data(rng, n, dim, metric), data(rng, DIM_MORE, dim, metric), data(rng, NQ, dim, metric)


# ---- 2. the batch schedule at its real size / 3. the layer cap ---------------------------------------------------------
# name -> (metric, n, dim, M, efc, max_batch of build_graph, max_batch of the oracle's build_batched, seed)
# At 70 000 rows a cap of 4 096 binds only for the last batch (from 65 536 linked nodes), which has 3 141 rows left: its
# node field is 17 bits wide, its batch field 12.  "schedule_4096_full" goes on to 72 000 rows, where one batch really
# holds 4 096 rows (a 13-bit batch field).
BIG_CASES = {
    "schedule_2048": ("euclidean", 70_000, 16, 6, 24, 0, 2048, 2),
    "schedule_4096": ("cosine", 70_000, 16, 6, 24, 4096, 4096, 3),
    "schedule_4096_full": ("cosine", 72_000, 16, 6, 24, 4096, 4096, 3),
    "layer_cap": ("euclidean", 70_000, 8, 2, 16, 0, 2048, 1),
}
SCHEDULE_CASES = ("schedule_2048", "schedule_4096", "schedule_4096_full")
FULL_BATCH_CASES = ("schedule_2048", "schedule_4096_full", "layer_cap")     # a whole batch of the cap's size is linked


def schedule_facts(name):
    """-> (batch sizes, nodes linked before the last batch, the cap) of a BIG_CASES build"""
    _, n, _, _, _, mb, omb, _ = BIG_CASES[name]
    assert (mb or 2048) == omb, "both sides must run one schedule"
    sizes = schedule(n, mb)
    return sizes, n - sizes[-1], omb


def big_case_data(name):
    metric, n, dim, _M, _efc, _mb, _omb, seed = BIG_CASES[name]
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((NQ, dim)).astype(np.float32)


# ---- 4. hubs and duplicates ------------------------------------------------------------------------------------------
HUB_N, HUB_DIM, HUB_M, HUB_EFC, HUB_MB = 3000, 64, 8, 40, 256
HUB_GROUP_MIN = 4 * 2 * HUB_M     # four times the layer-0 stride: the link kernel's wave appends, then prunes dozens of times
DUP_PAIRS_MIN = 1000
HUB_CASES = {"star_euclidean": "euclidean", "star_dot": "dot", "dups_euclidean": "euclidean", "dups_cosine": "cosine"}


def hub_case_data(name):
    """star: unit-norm Gaussian rows whose first 12 sit next to the origin (Euclidean: everybody's nearest neighbours) or
    far out along their direction (DotProduct: the largest products) — a dozen targets collect most of a batch's requests.
    dups: 3 000 draws from 375 distinct rows — zero distances and exact ties in every list.
    -> (rows, queries, source): source[i] = the distinct row that row i copies (dups), else None."""
    rng = np.random.default_rng(40 + sorted(HUB_CASES).index(name))
    if name.startswith("star"):
        rows = rng.standard_normal((HUB_N, HUB_DIM))
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        rows[:12] *= 0.01 if name == "star_euclidean" else 10.0
        rows, src = rows.astype(np.float32), None
    else:
        base = rng.standard_normal((375, HUB_DIM)).astype(np.float32)
        src = rng.integers(0, 375, HUB_N)
        rows = base[src]
    return rows, rng.standard_normal((NQ, HUB_DIM)).astype(np.float32), src


def hub_case_oracle(name):
    """The oracle's build, stepped batch by batch on the GPU's schedule -> (graph, largest layer-0 group): after each batch,
    for every layer-0 target the number of the batch's new nodes that list it = the size of its (layer 0, target) group in
    the link kernel."""
    rows, _, _ = hub_case_data(name)
    g = new_oracle(HUB_DIM, HUB_CASES[name], HUB_M, HUB_EFC)
    pos, largest = 0, 0
    for b in schedule(HUB_N, HUB_MB):
        g.insert_batch_sync(rows[pos:pos + b])
        targets = [t for node in range(pos, pos + b) for t in g.neighbors(0, node)]
        if targets:
            largest = max(largest, int(np.bincount(np.asarray(targets, dtype=np.int64)).max()))
        pos += b
    return g, largest


def zero_distance_pairs(g, src):
    """(node, neighbour) pairs of layer 0 whose two rows are copies of one row"""
    return sum(int(np.count_nonzero(src[np.asarray(nb, dtype=np.int64)] == src[i])) for i, nb in enumerate(layer0_lists(g, len(src))) if nb)


# ---- 5. list widths and small ef ----------------------------------------------------------------------------------------
# strides of 4 .. 256: a prune ranks stride + 1 entries in 1 .. 5 rounds of its lane ownership (lane + 64 r); strides that are no multiple of 64
# (66, 200), efc below the stride (nbmax from the stride), efc 1, efc at and around multiples of 64
# name -> (metric, n, dim, M, efc)
WIDTH_CASES = {f"m{M}_efc{efc}": ("euclidean", 2500, 32, M, efc)
               for M, efc in ((2, 8), (3, 1), (8, 4), (32, 400), (33, 100), (48, 128), (64, 192), (96, 200), (100, 193))}
WIDTH_CASES.update({
    "preset_m64_efc800": ("cosine", 3000, 128, 64, 800),          # params.rs:72-147, mirrored in velesdb_amd/params.py
    "preset_m96_efc1200": ("cosine", 3000, 256, 96, 1200),
    "preset_m128_efc2000": ("euclidean", 3000, 768, 128, 2000),
})


def width_case_data(name):
    metric, n, dim, M, efc = WIDTH_CASES[name]
    rng = np.random.default_rng(500 + 7 * M + efc)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((NQ, dim)).astype(np.float32)


def width_case_must_fill(name):
    _, _, _, M, efc = WIDTH_CASES[name]
    return efc >= M


# ---- 6. visited-log overflow ----------------------------------------------------------------------------------------------
VLOG_CASE = ("euclidean", 26_000, 96, 32, 1300)
VLOG_PROBES = 40


def vlog_case_data():
    _, n, dim, _, _ = VLOG_CASE
    rng = np.random.default_rng(6)
    return (rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((VLOG_PROBES, dim)).astype(np.float32),
            rng.standard_normal((NQ, dim)).astype(np.float32))


def vlog_visited(g, probes):
    """Rows a search at ef = ef_construction evaluates on the finished graph: what an insert of one more row visits."""
    out = []
    for p in probes:
        g.search(p, 1, VLOG_CASE[4])
        out.append(g.last_stats()[0])
    return out


# ---- the oracle graphs nothing mutates: one build per process ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_build(name):
    if name in BIG_CASES:
        metric, n, dim, M, efc, _mb, omb, _seed = BIG_CASES[name]
        rows = big_case_data(name)[0]
    elif name in WIDTH_CASES:
        metric, n, dim, M, efc = WIDTH_CASES[name]
        rows, omb = width_case_data(name)[0], 2048
    else:
        assert name == "vlog"
        metric, n, dim, M, efc = VLOG_CASE
        rows, omb = vlog_case_data()[0], 2048
    g = new_oracle(dim, metric, M, efc)
    g.build_batched(rows, omb)
    return g


# ---- 7. insert after load ---------------------------------------------------------------------------------------------------
LOAD_N, LOAD_MORE, LOAD_M, LOAD_EFC, LOAD_MB = 1500, 400, 8, 40, 64
LOAD_PRUNED_MIN = 100
LOAD_CASES = [(m, d) for m in FLOATS for d in (100, 256, 512, 768, 1024, 2048)] + [(m, d) for m in BITS for d in (33, 1000)]
LOAD_ONE_BY_ONE = [("cosine", 768), ("euclidean", 256), ("dot", 1024), ("hamming", 33), ("jaccard", 1000)]


def load_case_data(metric, dim):
    rng = np.random.default_rng(7000 + dim + 17 * METRIC[metric])
    return data(rng, LOAD_N, dim, metric), data(rng, LOAD_MORE, dim, metric), data(rng, NQ, dim, metric)


def load_case_oracle(metric, dim, directory, one_by_one=False):
    """Build LOAD_N rows, dump, load again, insert LOAD_MORE -> (graph, pruned): pruned = loaded nodes whose layer-0 list was
    full at the load and differs afterwards; a full list only changes through a prune, and a prune after a load ranks
    the list by the distances graph_fill_ndist computed."""
    rows, more, _ = load_case_data(metric, dim)
    g0 = new_oracle(dim, metric, LOAD_M, LOAD_EFC)
    g0.build_batched(rows, LOAD_MB)
    g0.file_dump(str(directory), "native_hnsw")
    g = reload_oracle(str(directory), "native_hnsw", dim, metric)
    before = layer0_lists(g, LOAD_N)
    if one_by_one:
        for v in more:
            g.insert(v)
    else:
        g.build_batched(more, LOAD_MB)
    after = layer0_lists(g, LOAD_N)
    pruned = sum(len(a) == 2 * LOAD_M and a != b for a, b in zip(before, after))
    return g, pruned
