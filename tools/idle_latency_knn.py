#!/usr/bin/env python3
"""Single-query latency of the host-buffer call (Ohnsw.knn: one query per call, test/test.ml:122) on the C2 index: median of
200 calls at ef = k = 10 and at ef 128, with 1 and with 64 queries per call from ordinary memory (the small-call path: a
page-locked block of the handle's).  (GPU box)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ocaml_hnsw_amd as H  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
X = bench.make_sift_like(1000000, 128, 1, dev).cpu().numpy()
hg = H.Ohnsw.build_batch_bigarray(X, 16, 200, seed=1)
Q = bench.make_sift_like(256, 128, 2, dev).cpu().numpy()
for ef, k in ((10, 10), (128, 10)):
    for nq in (1, 64):
        ts = []
        for i in range(220):
            q = Q[i % 190:i % 190 + nq]
            t = time.perf_counter()
            H.Ohnsw.knn_batch_bigarray(hg, k, q, ef=ef)
            ts.append(time.perf_counter() - t)
        ts = sorted(ts[20:])
        print("  ef %3d, %2d queries per call: median %.1f us (min %.1f)" % (ef, nq, 1e6 * ts[len(ts) // 2], 1e6 * ts[0]), flush=True)
