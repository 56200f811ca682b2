"""The metric x chunks-per-lane dispatch of the graph-walk launches (velesdb_amd/csrc/vdb_walk_dispatch.hpp), the part that needs no
GPU: the header compiles with a plain host compiler, and for every metric and every dimension class the callable receives exactly the
constants the hand-written ladders selected, exactly once (tests/walk_dispatch_model.cpp has the table)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_dispatch_selects_what_the_ladders_selected(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "walk_dispatch_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "walk_dispatch_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)  # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    # 9 dims x (7 metric values x (3 families + the metric alone) + the chunks alone) + the two-way helper
    assert line["ok"] and line["violations"] == 0 and line["cases"] == 9 * (7 * 4 + 1) + 2
