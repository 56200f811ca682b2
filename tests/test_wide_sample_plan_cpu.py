"""The WIDE selection's sample plan, checked on the CPU (`velesdb_amd/csrc/vdb_wide_sample.hpp`: host arithmetic, the text the library
compiles).  `tests/wide_sample_model.cpp` walks nq in {16, 96, 256, 1000, 1024} x n in {65 536, 66 001, 10^6, 6.25 * 10^6} x several k,
sample tiles per block and group sizes on a 256-CU chip: the sample range is whole 256-row tiles <= n, keys per query <= kWideSeedGroups
(and >= k), the sample launch's block map reaches every sample tile of every query tile once, and the selection launches behind it
cover every row tile from row 0 exactly once (built with ASan + UBSan)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_sample_plan_and_the_launches_behind_it(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "wide_sample_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "wide_sample_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)   # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["ok"] and line["violations"] == 0 and line["cases"] == 5 * 4 * 7 * 2 * 2
