"""The yardstick of the filtered graph walk validates itself on the CPU (tests/filtered_walk_ref.py): with every row allowed the
two-heap form IS the oracle's NativeHnsw::search — ids, distance bits, counts and the two counters — and the single-list form (the
kernel's) agrees with the two-heap form whenever it does not report an overflow."""
import numpy as np
import pytest

import filtered_walk_ref as fw
from oracle import pyoracle as po

N, DIM, M, EFC, NQ = 700, 24, 6, 40, 8
KEF = [(10, 64), (1, 16), (25, 50)]


def make(metric, seed=5):
    rng = np.random.default_rng(seed)
    if metric == po.HAMMING:  # sign-bit data: the packed-bit metrics read bit = (x > 0.5)
        rows = (rng.standard_normal((N, DIM)) > 0).astype(np.float32)
        qs = (rng.standard_normal((NQ, DIM)) > 0).astype(np.float32)
    else:
        rows = rng.standard_normal((N, DIM)).astype(np.float32)
        qs = rng.standard_normal((NQ, DIM)).astype(np.float32)
    g = po.NativeHnsw(DIM, metric, M, EFC, po.MODE_C)
    g.set_build_tie(po.TIE_CANONICAL)
    for v in rows:
        g.insert(v)
    return fw.Graph(g, rows, metric), qs, rng


@pytest.fixture(scope="module", params=[po.COSINE, po.EUCLIDEAN, po.DOT, po.HAMMING], ids=["cosine", "euclidean", "dot", "hamming"])
def world(request):
    return make(request.param)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("k,ef", KEF)
def test_two_heap_form_with_every_row_allowed_is_the_oracle_search(world, k, ef):
    G, qs, _ = world
    allowed = np.ones(G.n, dtype=bool)
    ids, ds, cnt, nd, ne = G.g.search_batch(qs, k, fw.ef_rule(k, ef), po.TIE_CANONICAL)
    tot_d = tot_e = 0
    for i, q in enumerate(qs):
        wi, wd, a, b = fw.walk_two_heap(G, q, k, fw.ef_rule(k, ef), allowed)
        assert wi == ids[i, :cnt[i]].tolist() and len(wi) == cnt[i]
        assert bits(wd) == bits(ds[i, :cnt[i]])
        tot_d, tot_e = tot_d + a, tot_e + b
    assert (tot_d, tot_e) == (nd, ne)


def filters(G, rng):
    out = {f"1/{int(1 / d)}": fw.random_filter(rng, G.n, d) for d in (1.0, 0.5, 0.1, 0.01)}
    out["clustered"] = G.rows[:, 0] > 0
    return out


@pytest.mark.parametrize("k,ef", [(10, 64), (1, 16)])
def test_single_list_form_agrees_with_the_two_heap_form_unless_it_overflows(world, k, ef):
    G, qs, rng = world
    ef_eff = fw.ef_rule(k, ef)
    for name, allowed in filters(G, rng).items():
        sized = fw.sized_list(ef_eff, int(allowed.sum()), G.n)
        for cap in (fw.min_list(ef_eff), sized, 4 * sized):
            clean = 0
            for q in qs:
                a = fw.walk_two_heap(G, q, k, ef_eff, allowed)
                b = fw.walk_single_list(G, q, k, ef_eff, allowed, cap)
                # overflow <=> an entry the two-heap form still needs fell off: unexpanded, or allowed while results were short
                needed = any(not (f & fw.EXPANDED) or ((f & fw.ALLOWED) and not full) for _, f, full in b[5]["lost"])
                assert b[4] == needed, (name, cap)
                assert b[5]["peak"] <= cap
                if b[4]:
                    continue
                clean += 1
                assert b[0] == a[0] and bits(b[1]) == bits(a[1]) and b[2:4] == a[2:4], (name, cap)
                assert all(allowed[i] for i in b[0])
            if cap >= G.n:  # the list holds the whole graph: nothing can fall off
                assert clean == len(qs), (name, cap)


def test_a_short_list_overflows_and_a_long_one_does_not(world):
    G, qs, rng = world
    allowed = fw.random_filter(rng, G.n, 0.01)  # 7 rows: the walk admits the whole component before its results fill
    over = [fw.walk_single_list(G, q, 5, 64, allowed, 128)[4] for q in qs]
    assert all(over)
    for q in qs:
        b = fw.walk_single_list(G, q, 5, 64, allowed, fw.round64(G.n))
        e = fw.exact_pass(G, q, 5, allowed)
        assert not b[4]
        if b[3] == G.n:  # the walk reached every node: its answer is the exact one, same distance bits
            assert b[0] == e[0] and bits(b[1]) == bits(e[1])
