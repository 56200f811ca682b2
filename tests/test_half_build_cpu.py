"""CPU-side checks for graph construction over the half-precision rows (tests/test_gpu_half_build.py is the GPU side):

  * the oracle recipes of tests/half_build_ref.py mean what the GPU tests take them to mean — every case's graph over the rounded rows
    differs from the graph over the f32 rows (else a build that ignored the graph precision would pass), the switch recipe prunes
    lists that were full at the switch and lands the level stream where a live graph's stands;
  * what the compiler made of hnsw_insert_half_kernel / hnsw_ndist_half_kernel, read from the built library like
    tests/test_hnsw_half_resources_cpu.py.
"""
import os
import subprocess
import sys
import tempfile

import pytest

import build_shapes as bs
import half_build_ref as hb
import half_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


# ---- 1. the precondition of every GPU case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hb.SHAPES, ids=lambda s: f"n{s[0]}_d{s[1]}")
@pytest.mark.parametrize("metric", hb.METRICS)
def test_rounded_rows_build_another_graph(metric, shape):
    n = shape[0]
    for mode in hb.MODES:
        g32 = hb.case_oracle(metric, shape, hr.F32, mode)
        for precision in hb.PRECISIONS:
            g = hb.case_oracle(metric, shape, precision, mode)
            d = hb.differing_lists(g, g32, n)
            print(f"{metric} {shape} {mode} {hb.PNAME[precision]}: {d} of {n} layer-0 lists differ from the f32 graph's")
            assert d >= 1, (metric, shape, mode, precision)


# ---- 2. the switch recipe -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", [True, False], ids=["live", "loaded"])
@pytest.mark.parametrize("case", hb.SWITCH_CASES, ids=lambda c: f"{c[0]}_{hb.PNAME[c[1]]}_to_{hb.PNAME[c[2]]}")
def test_switch_recipe_prunes_full_lists_and_differs_from_both_plain_builds(case, live, tmp_path):
    metric, before, after = case
    g, pruned, _ = hb.switch_oracle(metric, before, after, tmp_path, live)
    n = hb.SWITCH_N + hb.SWITCH_MORE
    assert len(g) == n
    full_at_switch = sum(len(x) == 2 * hb.SWITCH_M for x in bs.layer0_lists(hb.build_oracle(
        hb.rounded(hb.switch_data(metric)[0], before), metric, hb.SWITCH_M, hb.SWITCH_EFC, "sequential"), hb.SWITCH_N))
    print(f"{case} live {live}: {full_at_switch} lists full at the switch, {pruned} of them pruned afterwards")
    assert pruned >= 1                                   # (load_case_oracle's condition: a prune ranks by the refilled cache)
    if live:
        # neither a build that kept the old precision nor one that had the new precision from the start
        for p in (before, after):
            assert hb.differing_lists(g, hb.unswitched_oracle(metric, p), n) >= 1, hb.PNAME[p]


def test_advancing_the_level_stream_is_one_step_per_call():
    from oracle import pyoracle as po
    metric = "euclidean"
    rows, _ = hb.switch_data(metric)
    g = hb.build_oracle(rows[:40], metric, hb.SWITCH_M, hb.SWITCH_EFC, "sequential")
    s0 = g.rng_state()
    hb.advance_level_stream(g, 7, rows[0])
    assert g.rng_state() == int(po.xorshift_stream(7, s0)[-1])


# ---- 3. what the compiler made of the new kernels -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels():
    pytest.importorskip("msgpack")
    assert os.path.exists(kr.LIB), "libvelesdb_hip.so is not built (python -m velesdb_amd.build)"
    return {k["name"]: k for k in kr.kernels()}


def name(family, metric, cpl, f16):
    return f"vdb::{family}<{metric}, {cpl}, {'true' if f16 else 'false'}>"


@pytest.mark.parametrize("family", ["hnsw_insert_half_kernel", "hnsw_ndist_half_kernel"])
def test_exactly_the_thirty_instances_exist_without_scratch(kernels, family):
    fam = [n for n in kernels if kr.family(n) == family]
    want = {name(family, m, cpl, f16) for m in (0, 1, 2) for cpl in (0, 1, 2, 3, 4) for f16 in (True, False)}
    assert len(want) == 30 and set(fam) == want, sorted(set(fam) ^ want)
    for n in fam:
        k = kernels[n]
        assert k["block"] == 256, k
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k


@pytest.mark.parametrize("f16", [True, False])
def test_headline_insert_instance_keeps_its_f32_twins_occupancy(kernels, f16):
    h = kernels[name("hnsw_insert_half_kernel", 0, 3, f16)]
    t = kernels["vdb::hnsw_insert_kernel<0, 3>"]
    print(f"hnsw_insert_half_kernel<0, 3, {f16}>: {h['vgpr']} registers, {h['waves_per_simd']} waves per SIMD; f32 twin {t['vgpr']}, {t['waves_per_simd']}")
    assert h["waves_per_simd"] >= t["waves_per_simd"], (h, t)


@pytest.mark.skipif(not os.path.exists(kr.OBJDUMP), reason="llvm-objdump is not installed")
def test_no_flat_instruction_in_the_new_symbols(kernels):
    new = [k for k in kernels.values() if kr.family(k["name"]) in ("hnsw_insert_half_kernel", "hnsw_ndist_half_kernel")]
    assert len(new) == 60
    objs = kr.code_objects()
    assert len({k["obj"] for k in new}) == 1
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(objs[new[0]["obj"]])
        f.flush()
        txt = subprocess.run([kr.OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
    sym, flat = None, {}
    for line in txt.split("\n"):
        if line.endswith(">:") and "<" in line:
            sym = line[line.index("<") + 1:-2]
        elif sym is not None and line.split("//")[0].strip().startswith("flat_"):
            flat[sym] = flat.get(sym, 0) + 1
    bad = {k["name"]: flat[k["symbol"]] for k in new if k["symbol"] in flat}
    assert not bad, bad
