"""bench.py without --full on the GPU, at a toy size: a fresh process that builds the index, warms up, times its steps, writes
--dump-outputs and prints ONE line that carries the headline and no other leg."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(400)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    n, nq, k, steps, warmup = 20_000, 1000, 10, 3, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--n", str(n), "--nq", str(nq), "--dump-outputs", str(tmp_path / "dump")]
    env = {k_: v_ for k_, v_ in os.environ.items() if k_ != "BENCH_BATCHES"}       # the default rotation of 8 batches
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(nq / (out["ms_per_step"] * 1e-3), rel=1e-2)
    assert out["config"]["n"] == n and out["config"]["queries_per_gpu"] == nq
    for leg in ("roofline", "cpu_baseline", "checks", "recall_at_10", "device_resident", "float32_rows", "bandwidth_point",
                "harder_set_at_recall_gate", "others", "bench_dist", "functor_api"):
        assert out[leg] is None, leg
    # the last timed step's results: valid ids, ascending finite distances, and the neighbours of that step's batch
    ids = np.load(tmp_path / "dump" / "ids.npy")
    dist = np.load(tmp_path / "dump" / "distances.npy")
    assert ids.shape == dist.shape == (nq, k) and ids.dtype == np.float64 and dist.dtype == np.float32
    assert ((ids >= 0) & (ids < n)).all() and np.isfinite(dist).all() and (np.diff(dist, axis=1) >= 0).all()
    assert all(len(set(row)) == k for row in ids.tolist())
    dev = torch.device("cuda", 0)
    X = bench.make_sift_like(n, 128, seed=1, device=dev)
    Q = bench.make_sift_like(nq, 128, seed=2 + (warmup + steps - 1) % 8, device=dev)
    assert bench.recall_ids(ids.astype(np.int64), bench.brute_force_topk(X, Q, k)) >= 0.95
