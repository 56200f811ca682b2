"""bench.py --dump-outputs on the GPU: a plain (headline-only) run at a small size writes what its last timed step returned, and that is
what a caller of the same path gets for the same queries — ids, score bits and counts of search_batch_brute_force over the same seeded
corpus, regenerated here the way bench.py generates it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, K, Q = 70_000, 768, 10, 256


def test_plain_run_dumps_the_last_timed_step(tmp_path, gpu_required):
    import torch
    import velesdb_amd as va
    out = tmp_path / "dump"
    steps, warmup = 3, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--settle-steps", "0",
                        "--rows", str(N), "--batch", str(Q), "--hnsw-batch", str(Q), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["legs"] == {} and line["legs_file"] is None          # the headline alone
    assert sorted(os.listdir(out)) == ["counts.npy", "ids.npy", "scores.npy"]
    ids, sc, cnt = (np.load(out / f) for f in ("ids.npy", "scores.npy", "counts.npy"))
    assert ids.dtype == np.float64 and sc.dtype == np.float32 and ids.shape == sc.shape == (Q, K) and cnt.shape == (Q,)

    # bench.py's inputs: corpus from seed 42, a query pool of max(4 Q, 256, --hnsw-batch) rows from seed 43; step i searches the Q
    # queries at (i * Q) % (pool - Q + 1), and the last timed step is i = warmup + steps - 1
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    rows = torch.randn((N, D), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
    g.manual_seed(43)
    pool = max(4 * Q, 256, Q)
    queries = torch.randn((pool, D), generator=g, device=dev, dtype=torch.float32).cpu().numpy()
    off = ((warmup + steps - 1) * Q) % (pool - Q + 1)
    ix = va.HnswIndex(D, va.DistanceMetric.Cosine, va.HnswParams(32, 400, N))
    try:
        ix.upload(np.arange(N, dtype=np.uint64), rows)
        eid, esc, ecnt = ix.search_batch_brute_force(queries[off:off + Q], K)
    finally:
        ix.close()
    assert np.array_equal(ids, eid)
    assert np.array_equal(sc.view(np.uint32), np.ascontiguousarray(esc, dtype=np.float32).view(np.uint32))
    assert np.array_equal(cnt, ecnt)
