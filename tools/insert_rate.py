#!/usr/bin/env python3
"""What growing an index costs (hnsw_index_insert) next to building it (hnsw_build), C2 shape: SIFT-like integers, d 128,
M 16, efC 200.  hnsw_build of 1 M vectors; build(900 k) followed by inserts of the last 100 k in calls of 100 k / 10 k / 1 k,
and 100 calls of one vector each.  Prints ms per call, nodes/s and recall@10 at ef 128 of the grown index next to the fully
built one (exact ground truth on the device).  Usage: python tools/insert_rate.py [--n 1000000]"""
import argparse
import os
import sys
import time

try:   # one HIP runtime per process: torch's bundled copy first
    import torch
except ImportError:
    torch = None
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


def ground_truth(X, Q, k):
    """the exact neighbours' ids: the library's own scan over a flat index (hnsw_brute_force_batch)"""
    flat = H.Hgraph.flat(X)
    try:
        return H.Ohnsw.brute_force_knn(flat, k, Q)[0]
    finally:
        flat.release()


def recall(hg, Q, gt, ef=128, k=10):
    ids, _ = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, gt)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--tail", type=int, default=100_000)
    ap.add_argument("--nq", type=int, default=1000)
    a = ap.parse_args()
    d, M, efc, seed = 128, 16, 200, 1
    n, n0 = a.n, a.n - a.tail
    centres = np.random.default_rng(1234).integers(20, 200, size=(4096, d)).astype(np.float32)
    X = sift_like(n, d, 1, centres)
    Q = sift_like(a.nq, d, 2, centres)
    gt = ground_truth(X, Q, 10)
    H.load()

    def build(rows):
        t = time.perf_counter()
        hg = H.Ohnsw.build_batch_bigarray(X[:rows], M, efc, seed=seed)
        return hg, time.perf_counter() - t

    full, t_full = build(n)
    print("C2 shape: d %d, M %d, efC %d, SIFT-like integers; recall@10 at ef 128 over %d queries" % (d, M, efc, a.nq))
    print("hnsw_build of %d: %.1f ms (%.2f M nodes/s), recall %.4f" % (n, 1e3 * t_full, n / t_full / 1e6, recall(full, Q, gt)))
    del full
    _, t_base = build(n0)
    print("hnsw_build of %d: %.1f ms" % (n0, 1e3 * t_base))
    for call, calls in ((a.tail, 1), (a.tail // 10, 10), (a.tail // 100, 100), (1, 100)):
        hg, _ = build(n0)
        ts = []
        for c in range(calls):
            s = n0 + c * call
            t = time.perf_counter()
            H.Ohnsw.insert_batch(hg, X[s:s + call], M, efc, seed=seed)
            ts.append(time.perf_counter() - t)
        ts = np.array(ts)
        grown = n0 + calls * call
        line = ("insert into %d in calls of %6d x %3d: %8.2f ms per call (median %.2f, first %.2f), %.3f M nodes/s, "
                "one call = %.2f %% of the %d build" % (n0, call, calls, 1e3 * ts.mean(), 1e3 * np.median(ts), 1e3 * ts[0],
                                                        call / ts.mean() / 1e6, 100 * ts.mean() / t_full, n))
        if grown == n:
            line += ", recall %.4f" % recall(hg, Q, gt)
        print(line, flush=True)
        del hg


if __name__ == "__main__":
    main()
