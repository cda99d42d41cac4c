#!/usr/bin/env python3
"""What the diversified search costs.  Shapes: c2 (1 M x 128 SIFT-like integers = byte rows, L2) and c3 (1 M x 100 float32 rows, inner
product), M 16, efC 200, ef 128, k 10, lambda 0.5, 10 k queries.  On ONE handle, the calls of a leg taking turns:
  (a) hnsw_search_batch_diverse at pool 32, 64, 128 against hnsw_search_batch at k = pool -- the inner call alone, so the difference
      is the selection;
  (b) the same call against the host round trip it replaces: hnsw_search_batch at k = pool, hnsw_index_get_rows of the p rows per
      query, then the greedy loop in numpy (pair distances from one batched Gram product, the loop vectorised over the queries);
      the numpy loop is float32 but not bit-identical to the device's (another summation order): how many rows agree is printed.
Host clock around the synchronous host calls, medians and ranges of --steps rounds after a warm round; a comparison is between calls
of the same run on the same handle, never against a recorded number.
--kernels-only: hnsw_diversify_batch beside hnsw_rerank_batch on the same device-resident pools, --steps calls each per pool -- run
it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (hnsw_diversify_kernel against hnsw_rerank_kernel), in a run
of its own.
Informational: nothing gates on it.  The table printed here is what profiles/diverse.txt holds.
Usage: python tools/diverse_rate.py [--shape c2|c3] [--n 1000000] [--nq 10000] [--steps 7] [--host-steps 2] [--kernels-only]
       [--out profiles/diverse.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:   # one HIP runtime per process: torch's bundled copy first, if there is one
    import torch  # noqa: F401
except ImportError:
    pass
import ocaml_hnsw_amd as H  # noqa: E402

POOLS = (32, 64, 128)


def timed(calls, steps):
    """the calls take turns; per call the times of `steps` rounds after a warm one (ms)"""
    times = [[] for _ in calls]
    for r in range(steps + 1):
        for j, call in enumerate(calls):
            t0 = time.perf_counter()
            call()
            if r:
                times[j].append((time.perf_counter() - t0) * 1e3)
    return times


def fmt(t):
    return "%9.3f ms (min %.3f, max %.3f, %d runs)" % (float(np.median(t)), min(t), max(t), len(t))


def overlap(a, b):
    return "the ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "the ranges do not overlap"


def host_round_trip(hg, Q, pool, k, lam, ef, ip):
    """what a caller does today: the search at k = pool, the rows up the link, the greedy loop in numpy"""
    ids, r = H.Ohnsw.knn_batch_bigarray(hg, pool, Q, ef=ef)
    nq = len(Q)
    pad = ids < hg.id_base                                      # (a walk that found fewer than pool nodes: never picked)
    R = hg.rows(np.where(pad, hg.id_base, ids).reshape(-1)).reshape(nq, pool, -1)
    G = np.matmul(R, R.transpose(0, 2, 1))                      # [nq][p][p]
    if ip:
        D = np.float32(1.0) - G
    else:
        sq = np.einsum("qpd,qpd->qp", R, R)
        D = np.sqrt(np.maximum(sq[:, :, None] + sq[:, None, :] - 2.0 * G, 0.0))
    lam32, mu32 = np.float32(lam), np.float32(1.0) - np.float32(lam)
    rows = np.arange(nq)
    pick = np.zeros((nq, k), np.int64)
    m = np.full((nq, pool), np.inf, np.float32)
    taken = pad.copy()
    taken[:, 0] = True
    for j in range(1, k):
        m = np.minimum(m, D[rows, pick[:, j - 1]])
        g = lam32 * r - mu32 * m
        g[taken] = np.inf
        pick[:, j] = np.argmin(g, axis=1)
        taken[rows, pick[:, j]] = True
    return np.take_along_axis(ids, pick, axis=1)        # (a row with fewer than k real candidates repeats its first pick: such rows disagree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2", choices=("c2", "c3"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("diverse_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    M, efc, ef, k, lam = 16, 200, 128, 10, 0.5
    rng = np.random.default_rng(7)
    ip = a.shape == "c3"
    if ip:
        d = 100
        X = rng.normal(size=(a.n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rng.normal(size=(a.nq, d)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    else:
        d = 128
        centres = rng.integers(20, 200, size=(256, d))
        X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
        Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef, metric=H.METRIC_IP if ip else H.METRIC_L2)
    say("diversified search: %s shape, n %d, d %d, %s, M %d, efC %d, ef %d, k %d, lambda %g, %d queries; build %.1f s; rows: %d B"
        % (a.shape.upper(), a.n, d, "inner product" if ip else "L2", M, efc, ef, k, lam, a.nq, time.time() - t0, hg.row_bytes()))

    if a.kernels_only:
        say("the operator beside the re-rank on the same pools, %d calls each per pool (kernel times: the trace of this run)" % a.steps)
        for pool in POOLS:
            cand = H.Ohnsw.knn_batch_bigarray(hg, pool, Q, ef=ef)[0]
            t = timed([lambda: H.Ohnsw.rerank(hg, k, Q, cand), lambda: H.Ohnsw.diversify(hg, k, Q, cand, lam)], a.steps)
            say("pool %3d: hnsw_rerank_batch %s; hnsw_diversify_batch %s (host calls, candidates uploaded)" % (pool, fmt(t[0]), fmt(t[1])))
    else:
        say("the calls of a leg take turns on one handle, medians of %d rounds after a warm round (the host round trip: %d rounds)" % (a.steps, a.host_steps))
        for pool in POOLS:
            inner = lambda: H.Ohnsw.knn_batch_bigarray(hg, pool, Q, ef=ef)                     # noqa: E731
            diverse = lambda: H.Ohnsw.knn_batch_diverse(hg, k, Q, pool, lam, ef=ef)            # noqa: E731
            got = diverse()
            want = H.Ohnsw.diversify(hg, k, Q, inner()[0], lam)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            moved = int((got[0] != H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]).any(axis=1).sum())
            t = timed([inner, diverse], a.steps)
            say("(a) pool %3d: hnsw_search_batch k = pool %s; hnsw_search_batch_diverse %s: +%.3f ms = %.2fx, %s; %d of %d rows differ from the plain k nearest"
                % (pool, fmt(t[0]), fmt(t[1]), float(np.median(t[1])) - float(np.median(t[0])), float(np.median(t[1])) / float(np.median(t[0])),
                   overlap(t[0], t[1]), moved, a.nq))
            host_ids = host_round_trip(hg, Q, pool, k, lam, ef, ip)
            th = timed([lambda: host_round_trip(hg, Q, pool, k, lam, ef, ip), diverse], a.host_steps)
            say("(b) pool %3d: search + hnsw_index_get_rows + numpy greedy loop %s; hnsw_search_batch_diverse %s: %.1fx faster, %s; %d of %d rows agree with the numpy loop"
                % (pool, fmt(th[0]), fmt(th[1]), float(np.median(th[0])) / float(np.median(th[1])), overlap(th[0], th[1]),
                   int((host_ids == got[0]).all(axis=1).sum()), a.nq))
    hg.release()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
