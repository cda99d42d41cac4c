#!/usr/bin/env python3
"""What shrinking an index costs (hnsw_index_remove) next to the only alternative, hnsw_build of the surviving vectors.  C2 data:
1 M x 128 SIFT-like integers (byte-valued), M 16, efC 200.  For 0.1 %, 1 %, 10 % and 50 % removed (a random set): wall time of the
one hnsw_index_remove call on a freshly built index, wall time of hnsw_build over X[live] on the same machine, and recall@10 at
ef 128 of both against the exact scan.  No ratio is promised: the table goes into profiles/remove_rate.txt.
--quality adds the numbers of tests/test_gpu_remove.py's recall gate (uniform, n 3000, d 16, M 8, efC 64, 20 % removed, ef 32).
Usage: python tools/remove_rate.py [--n 1000000] [--quality]"""
import argparse
import os
import sys
import time

try:   # one HIP runtime per process: torch's bundled copy first
    import torch  # noqa: F401
except ImportError:
    pass
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ocaml_hnsw_amd as H  # noqa: E402


def sift_like(n, d, seed, centres):
    rng = np.random.default_rng(seed)
    out = np.empty((n, d), np.float32)
    step = 1 << 17
    for s in range(0, n, step):
        m = min(step, n - s)
        out[s:s + m] = np.clip(np.rint(centres[rng.integers(0, len(centres), m)] + rng.normal(0, 25, size=(m, d))), 0, 218)
    return out


def recall(hg, Q, k, ef):
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]
    ids = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, truth)]))


def quality():
    n, d, nq, M, efc = 3000, 16, 300, 8, 64
    rng = np.random.default_rng(60)
    X = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    Q = rng.uniform(-1, 1, size=(nq, d)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1)
    new_id = H.Ohnsw.remove_batch(hg, rng.choice(n, size=n // 5, replace=False))
    ref = [recall(H.Ohnsw.build_batch_bigarray(X[new_id >= 0], M, efc, seed=s), Q, 10, 32) for s in (1, 2, 3, 4, 5)]
    print("quality gate (uniform, n 3000, d 16, M 8, efC 64, 20 %% removed, recall@10 at ef 32, 300 queries): repaired %.4f; "
          "rebuilt with seeds 1..5: %s" % (recall(hg, Q, 10, 32), " ".join("%.4f" % r for r in ref)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    H.load()
    if a.quality:
        quality()
    d, M, efc, seed, n = 128, 16, 200, 1, a.n
    centres = np.random.default_rng(1234).integers(20, 200, size=(4096, d)).astype(np.float32)
    X = sift_like(n, d, 1, centres)
    Q = sift_like(a.nq, d, 2, centres)
    print("C2 data: n %d, d %d, M %d, efC %d, SIFT-like integers; recall@10 at ef 128 over %d queries against the exact scan" % (n, d, M, efc, a.nq))
    print("%8s %10s | %14s %8s %9s | %14s %8s" % ("removed", "nodes", "remove ms", "recall", "mean deg", "rebuild ms", "recall"), flush=True)
    for pct in (0.1, 1.0, 10.0, 50.0):
        m = int(round(n * pct / 100))
        dead = np.random.default_rng(7).choice(n, size=m, replace=False)
        hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=seed)
        hg.vectors = None                                                # (no host copy to shrink: the call alone is timed)
        t = time.perf_counter()
        new_id = H.Ohnsw.remove_batch(hg, dead)
        t_remove = time.perf_counter() - t
        r_remove = recall(hg, Q, 10, 128)
        deg = hg.stats()["layer_connectivity"][0]["mean"]
        hg.release()
        Xl = np.ascontiguousarray(X[new_id >= 0])
        t = time.perf_counter()
        fresh = H.Ohnsw.build_batch_bigarray(Xl, M, efc, seed=seed)
        t_build = time.perf_counter() - t
        r_build = recall(fresh, Q, 10, 128)
        fresh.release()
        print("%7.1f%% %10d | %14.1f %8.4f %9.2f | %14.1f %8.4f" % (pct, m, 1e3 * t_remove, r_remove, deg, 1e3 * t_build, r_build), flush=True)


if __name__ == "__main__":
    main()
