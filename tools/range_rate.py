#!/usr/bin/env python3
"""What range search costs on the C2 shape (1 M x 128 SIFT-like integers, L2), 10 k queries, through the host calls (pageable
matrices, host clock, median of --steps calls after a warm call).  Two parts, run as separate commands:
  --part scan    hnsw_range_brute_force_batch at radii where a query has about 10, 1 000 and 100 000 hits, beside
                 hnsw_brute_force_batch (k = 10) of the same handle in the same process, alternating.  That call is the yardstick:
                 the range scan reads the table twice and sorts only its hits.  (The 100 000-hit radius runs on fewer queries, so
                 that the call's total stays near 10^8 results; its yardstick is timed on the same queries.)
  --part search  hnsw_range_search_batch (M 16, efC 200, ef 128) at radii where most queries are served at stage 0, beside
                 hnsw_search_batch of (ef, ef) on the same batch, with the share of queries per stage and the range recall against
                 hnsw_range_brute_force_batch: hits found / hits true, summed over the queries.
Informational: nothing gates on it.  The table printed here is what profiles/range_search.txt holds.
Usage: python tools/range_rate.py --part scan|search [--n 1000000] [--nq 10000] [--steps 5] [--out FILE (appended to)]"""
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


def alternating_ms(fa, fb, steps):
    """medians of two calls timed in turn, after one warm call each"""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(steps):
        for fn, out in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ta)), float(np.median(tb))


def radius_for(X, Q, hits, sample=32):
    """the radius at which a query has about `hits` hits: the median over a few queries of their hits-th smallest distance (numpy)"""
    x2 = (X.astype(np.float64) ** 2).sum(1)
    out = []
    for q in Q[:sample].astype(np.float64):
        d2 = x2 - 2.0 * (X @ q.astype(np.float32)).astype(np.float64) + (q ** 2).sum()
        out.append(np.sqrt(max(0.0, np.partition(d2, hits - 1)[hits - 1])))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("scan", "search"), required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("range_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef = 128, 16, 200, 128
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    if a.part == "scan":
        hg = H.Hgraph.flat(X)
        say("hnsw_range_brute_force_batch: C2 shape, n %d, d %d, L2, %d queries; beside hnsw_brute_force_batch (k = 10)" % (a.n, d, a.nq))
        for hits in (10, 1000, 100000):
            if hits >= a.n:
                continue
            nq = max(1, min(a.nq, 100_000_000 // hits))
            radius = radius_for(X, Q, hits)
            Qs = Q[:nq]
            rms, kms = alternating_ms(lambda: H.Ohnsw.brute_force_range(hg, radius, Qs), lambda: H.Ohnsw.brute_force_knn(hg, 10, Qs), a.steps)
            lims = H.Ohnsw.brute_force_range(hg, radius, Qs)[0]
            say("radius %9.3f (about %6d hits; measured mean %9.1f, total %10d; %5d queries): range scan %9.3f ms, k-scan %9.3f ms, "
                "ratio %.2f; %.3f M q/s" % (radius, hits, float(np.diff(lims).mean()), int(lims[-1]), nq, rms, kms, rms / kms, nq / rms / 1e3))
    else:
        t0 = time.time()
        hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
        say("hnsw_range_search_batch: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, %d queries; build %.1f s; rows: %d B; beside "
            "hnsw_search_batch (ef, ef)" % (a.n, d, M, efc, ef, a.nq, time.time() - t0, hg.row_bytes()))
        for hits in (10, 50, 200):
            radius = radius_for(X, Q, hits)
            rms, kms = alternating_ms(lambda: H.Ohnsw.range_search(hg, radius, Q, ef=ef), lambda: H.Ohnsw.knn_batch_bigarray(hg, ef, Q, ef=ef), a.steps)
            lims, _, _, _, _, stage = H.Ohnsw.range_search(hg, radius, Q, ef=ef, counters=True)
            true = H.Ohnsw.brute_force_range(hg, radius, Q)[0]
            values, counts = np.unique(stage, return_counts=True)
            shares = ", ".join("%s %.1f %%" % ("exact" if v == H.STAGE_EXACT else "stage %d" % v, 100.0 * c / a.nq) for v, c in zip(values, counts))
            say("radius %9.3f (about %4d hits; true mean %7.1f): range search %8.3f ms, %7.3f M q/s; search (ef, ef) %8.3f ms; ratio %.2f; %s; "
                "range recall %.4f" % (radius, hits, float(np.diff(true).mean()), rms, a.nq / rms / 1e3, kms, rms / kms, shares,
                                       float(lims[-1]) / max(1.0, float(true[-1]))))
    hg.release()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
