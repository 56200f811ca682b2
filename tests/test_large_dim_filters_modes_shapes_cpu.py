"""Every shape of tests/test_gpu_large_dim_filters_modes.py still sits at the edge it was chosen for — seen here, where no GPU is
needed.  The literal tables are the GPU file's (imported, not copied).

Sections B and C (SQ8, half-row Euclidean): mode_listed_plan of velesdb_amd/csrc/vdb_filter_route.hpp — the text the library compiles —
run by tests/large_dim_plan_model.cpp (stand-alone, ASan + UBSan, its own runtime linked in) at every (mode, dim, k, nq) the GPU tests
call: B, nq_pass, lds and blocks against the tables.

Section A (f32): sweep_listed_plan lives in csrc/sweep_listed.hip and cannot be compiled on the host from a header.  The literals are
held against the Python restatement of the GPU file (c_lds / c_passes / m_lds / m_passes); what binds that restatement to the product
is the GPU diagnostic — the launch count of last_filters_exact_plan on the forced listed route, asserted there at every shape."""
import json
import os
import shutil
import subprocess

import pytest

import test_gpu_large_dim_filters_modes as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = 256
CLASSES = {False: (8, 4, 1), True: (16, 4, 1)}


def mode_cases():
    """(half, dim, k, nq, count) of every listed call of sections B and C: the one-filter batches, every group size of the per-query
    tables and what is left of a group behind each pass, with the list lengths of the filters (the negated 10 %, 65 rows, one row)"""
    out = []
    for half, table, shapes, sizes in ((False, g.SQ8_TABLE, g.B_SHAPES, (1, 4, 9, 7)), (True, g.HALF_TABLE, g.C_EUCLID, (1, 4, 17, 5, 3))):
        n_of = {dim: n for n, dim in shapes}
        assert set(n_of) == {dim for dim, _ in table}, "a table row without a shape, or a shape without a row"
        for (dim, k), row in table.items():
            n = n_of[dim]
            for nq in sizes:
                left = nq
                for B, took in g.table_passes(half, nq, row[3]):
                    for count in (n - n // 10, 65, 1):
                        out.append((half, dim, k, left, count))
                    left -= took
    return sorted(set(out))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("large_dim_plan_model") / "large_dim_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "large_dim_plan_model.cpp")])
    cases = mode_cases()
    args = ["%s:%d:%d:%d:%d:%d" % ("half" if half else "sq8", dim, k, nq, count, N_CUS) for half, dim, k, nq, count in cases]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(rows) == len(cases) > 100
    return rows


def test_mode_listed_plan_takes_the_class_of_the_tables(model):
    seen = set()
    for r in model:
        half = r["mode"] == "half"
        table = g.HALF_TABLE if half else g.SQ8_TABLE
        wide, f4, f1, cap = table[(r["dim"], r["k"])]
        what = (r["mode"], r["dim"], r["k"], r["nq"], r["count"])
        # the footprint of every class is the table's, byte for byte, and the class taken is the widest that fits the budget
        assert (r["lds_wide"], r["lds_4"], r["lds_1"]) == (wide, f4, f1), what
        assert r["budget"] == g.FM_BUDGET
        foot = dict(zip(CLASSES[half], (wide, f4, f1)))
        assert cap == next(B for B in CLASSES[half] if foot[B] <= g.FM_BUDGET), what
        # the pass: the class the batch asks for, held down to the table's; its queries; its LDS
        B, took = g.table_passes(half, r["nq"], cap)[0]
        assert (r["B"], r["nq_pass"], r["lds"]) == (B, took, foot[B]), what
        # the blocks: contiguous chunks of row groups, at most n_cus x resident blocks (the GPU file asserts nothing about them;
        # a launch of zero blocks or one past the list would be the kernel's fault to find)
        rpg = 64 // B if half else 64
        ngroups = (r["count"] + rpg - 1) // rpg
        per_cu = min(g.FM_BUDGET // foot[B], 3 if half else 4)
        want = max(1, min((ngroups + 3) // 4, N_CUS * per_cu))
        per_block = (ngroups + want - 1) // want
        assert (r["per_block"], r["blocks"]) == (per_block, (ngroups + per_block - 1) // per_block), what
        assert r["blocks"] >= 1 and (r["blocks"] - 1) * r["per_block"] < ngroups <= r["blocks"] * r["per_block"], what
        seen.add((half, B, foot[B] > g.OPT_IN))
    # every class of both modes was planned, and the classes 8 / 4 (SQ8) and 16 / 4 (half) on both sides of the 64 KiB opt-in
    assert {(h, B) for h, B, _ in seen} == {(False, 8), (False, 4), (False, 1), (True, 16), (True, 4), (True, 1)}
    assert {(False, 8, True), (False, 4, True), (True, 16, True), (True, 4, True)} <= seen
    assert not any(over for _, B, over in seen if B == 1)


def test_the_edges_the_shapes_were_chosen_for():
    s, h = g.SQ8_TABLE, g.HALF_TABLE
    assert s[(1536, 10)][0] == 70400 > g.OPT_IN and g.FM_BUDGET // 70400 == 2                 # past the opt-in, two blocks per CU
    assert s[(4096, 10)][0] == 152320 and g.FM_BUDGET // 152320 == 1 and 8 * 4096 * 4 > g.OPT_IN   # one block per CU, query tile past 64 KiB
    assert s[(4096, 200)][:2] == (164480, 92480) and s[(4096, 200)][3] == 4                   # 640 B over: nine queries = 4 + 4 + 1
    assert g.table_passes(False, 9, 4) == [(4, 4), (4, 4), (1, 1)]
    assert s[(4099, 10)][0] == 152448 == 4 * 8 * 4100 + 20480 + 8 * 8 * 10 + 16 * 8           # dpad 4 100
    assert s[(9000, 10)][1] > g.FM_BUDGET and s[(9000, 10)][3] == 1
    assert h[(2536, 10)][0] == 163712 == g.FM_BUDGET - 128 and h[(2536, 10)][3] == 16          # the exact-fit launch
    assert h[(2544, 10)][0] == 164224 and h[(2544, 10)][3] == 4
    assert h[(4096, 10)][1] == 65888 > g.OPT_IN and h[(4096, 10)][3] == 4                      # the first B 4 instance past the opt-in
    assert h[(4095, 10)] == h[(4096, 10)]                                                      # stride 4 096
    assert h[(10240, 10)][1] > g.FM_BUDGET and h[(10240, 10)][3] == 1
    assert g.table_passes(True, 17, 4) == [(4, 4)] * 4 + [(1, 1)] and g.table_passes(True, 17, 16) == [(16, 16), (1, 1)]


def test_f32_literals_against_the_restated_sweep_listed_plan():
    """section A: the footprints, the class and the passes of the groups of 9 and 17 (g.a_expected_launches asserts them against
    c_lds / c_passes / m_lds / m_passes) — and that the shapes cover every class"""
    assert {dim for dim, _ in g.C_TABLE} == {dim for _, dim in g.A_SHAPES} and {k for _, k in g.C_TABLE} == set(g.A_KS)
    launches = {key: g.a_expected_launches("C", key[1], key[0]) for key in g.C_TABLE}
    assert {g.C_TABLE[key][3]: n for key, n in launches.items()} == {8: 3, 4: 2, 1: 1}
    assert g.C_TABLE[(1536, 10)][0] == 49856 <= g.C_WINDOW < 62016 == g.C_TABLE[(1536, 200)][0]
    assert g.C_TABLE[(2047, 10)][0] >= 65536 and g.C_TABLE[(2047, 10)][1] == 32768 + 352
    assert g.C_TABLE[(4096, 10)][1] >= 65536 and g.C_TABLE[(4096, 10)][2] == 16384 + 96
    assert g.c_passes(9, 10, 4096) == [(1, 1)] * 9 and g.c_passes(9, 10, 2047) == [(4, 4), (4, 4), (1, 1)]
    for key in g.M_TABLE:
        assert g.a_expected_launches("M", key[1], key[0]) == 1
    assert {row[3] for row in g.M_TABLE.values()} == {16, 8}
    assert g.M_TABLE[(2048, 10)][0] == 167616 > g.M_BUDGET >= g.M_TABLE[(1536, 200)][0]
    assert g.c_lds(1, 10, 16384) == 65632 > g.C_WINDOW      # past every plan
    # the modes the GPU file expects at each (metric, dim, k) have a table row
    for _, dim in g.A_SHAPES:
        for k in g.A_KS:
            for metric in g.FLOATS:
                mode = g.ldf.expected_mode(metric, dim, k)
                assert (dim, k) in (g.M_TABLE if mode == "M" else g.C_TABLE), (str(metric), dim, k, mode)


def test_rescore_shapes_are_generic_dims_with_the_query_scratch():
    assert g.D_SHAPES == [(1200, 1536, 8, 60), (1000, 4096, 8, 40), (1000, 4099, 6, 40)]
    assert all(dim not in (256, 512, 768, 1024) and dim > 1024 for _, dim, _, _ in g.D_SHAPES)
    assert g.fr.lds_bytes(64, 64, 4099) - g.fr.lds_bytes(64, 64, 1024) == 16400


def test_tables_interleave_as_the_gpu_tests_expect():
    assert len(g.fms.interleave(g.B_SIZES, 5)) == 23 and len(g.fms.interleave(g.fms.HALF_SIZES, 9)) == 30
    assert len(g.fms.interleave(g.C_DOT_SIZES, 9)) == 19
