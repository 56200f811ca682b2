"""The selection stage's park-after-failure rule, run on the CPU.

`velesdb_amd/csrc/vdb_select_hold.hpp` (host arithmetic, the text the library compiles) holds the rule the four `select_level_*`
selectors share: a verdict of the selector's own level with more than 1/16 of the batch unproven parks it for 64 batches.
`tests/select_hold_model.cpp` asks the selectors in `brute_dev`'s order over synthetic verdict streams (built with ASan + UBSan)
and prints the level traces of four configurations on data that defeats every selection; they must be the traces of
`tests/select_hold_traces.py`, the ones `tests/test_gpu_dev_sequences.py::test_hold_trace_with_a_sync_per_call` holds the library
to on the GPU.  With one seen-sequence shared by the four selectors (the state before this header existed) WIDE, asked first,
consumed every verdict: levels 2 / 5 / 3 never parked and the traces read 4, then 64 x 2 / 2 / 3.
"""
import json
import os
import shutil
import subprocess

import pytest

from select_hold_traces import CALLS, TRACES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_hold_traces_and_rules_of_the_model(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "select_hold_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "velesdb_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "select_hold_model.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)   # the binary links its own sanitizer runtime
    r = subprocess.run([exe], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line.pop("failed_checks") == 0
    assert set(line) == set(TRACES)
    for name, want in TRACES.items():
        assert len(line[name]) == CALLS
        assert line[name] == want, (name, line[name])
