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
  --part matrix  hnsw_range_brute_force_batch with option "scan_matrix" off and on, alternating within one handle, --steps (7)
                 timings per leg after two warm rounds, reported as ranges: 1 M x 128 Gaussian float rows, L2, at the radius of the
                 median 10th-neighbour distance (1 000 and 10 000 queries), at a wide radius with about 1 % of the table per query,
                 and on the rows and queries + 100 (norms far above the distances).  The call takes host queries: they are
                 page-locked and read in place, the result stays on the device (keep), the host clock spans the call, which ends in
                 a synchronisation.  Every on/off pair is compared: lims, ids and distance bits must be equal.  --kernels: a few
                 calls per option at 1 000 queries and nothing else, to be run under a kernel trace, in a run of its own.
                 The table of profiles/range_matrix.txt.
  --part bytes   the same measurement for option "scan_bytes" 0 against 2 (the range scan's 8-bit matrix kernels): 1 M x 128
                 byte-valued rows of the C2 shape, L2 and IP, 1 000 and 10 000 queries at the radius of the median 10th-neighbour
                 distance and 1 000 queries at a wide radius (the median distance of the n / 100-th neighbour); hits per query and
                 their share of the table are printed.  --kernels: as above (L2 only).  The table of profiles/range_bytes.txt.
Informational: nothing gates on it.  The table printed by the first two parts is what profiles/range_search.txt holds.
Usage: python tools/range_rate.py --part scan|search|matrix|bytes [--n 1000000] [--nq 10000] [--steps 5] [--kernels] [--out FILE (appended to)]"""
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


def matrix_part(a, say):
    """option "scan_matrix" off / on over the exact range scan (see the module's docstring)"""
    d, steps = 128, max(5, a.steps)
    say('hnsw_range_brute_force_batch, option "scan_matrix" off / on, one handle, alternating: n %d, d %d, L2, %d timings per leg' % (a.n, d, steps))
    for leg, shift in (("gauss", 0.0),) if a.kernels else (("gauss", 0.0), ("shifted", 100.0)):
        rng = np.random.default_rng(11)
        X = rng.standard_normal((a.n, d), dtype=np.float32) + np.float32(shift)
        Qall = rng.standard_normal((a.nq, d), dtype=np.float32) + np.float32(shift)
        hg = H.Hgraph.flat(X)
        cases = [(10, min(1000, a.nq))]
        if not a.kernels and leg == "gauss":
            cases += [(10, a.nq), (max(10, a.n // 100), min(1000, a.nq))]
        for hits, nq in cases:
            radius = radius_for(X, Qall, hits)
            Q = H.host_empty((nq, d))          # page-locked: read in place
            Q[:] = Qall[:nq]
            t, got = {0: [], 1: []}, {}
            for r in range((2 if a.kernels else steps) + 2):        # (two warm rounds)
                for v in (0, 1):
                    hg.set_option("scan_matrix", v)
                    t0 = time.perf_counter()
                    res = H.Ohnsw.brute_force_range(hg, radius, Q, keep=True)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert hg.scan_path() == (H.SCAN_PATH_MATRIX if v else H.SCAN_PATH_FLOAT)
                    if r >= 2:
                        t[v].append(dt)
                    if r == 0:
                        got[v] = res.fetch()
                    res.release()
            for x, y in zip(got[0], got[1]):
                assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
            disjoint = max(t[1]) < min(t[0]) or max(t[0]) < min(t[1])
            say("%-7s nq %5d radius %8.3f (mean %9.1f hits per query, %9d in all): off %8.3f .. %8.3f ms, on %8.3f .. %8.3f ms; ranges %s; "
                "off/on of the medians %.2f; on: %.3f ms per 1 000 queries"
                % (leg, nq, radius, float(np.diff(got[1][0]).mean()), int(got[1][0][-1]), min(t[0]), max(t[0]), min(t[1]), max(t[1]),
                   "disjoint" if disjoint else "overlap", np.median(t[0]) / np.median(t[1]), np.median(t[1]) * 1000.0 / nq))
        hg.release()


def bytes_part(a, say):
    """option "scan_bytes" 0 / 2 over the exact range scan (see the module's docstring)"""
    d, steps = 128, max(5, a.steps)
    say('hnsw_range_brute_force_batch, option "scan_bytes" 0 / 2, one handle, alternating: n %d, d %d, byte-valued rows, %d timings per leg' % (a.n, d, steps))
    rng = np.random.default_rng(7)          # (the C2 shape of the other parts: clustered SIFT-like integers in 0..218)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Qall = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    for metric, name in ((H.METRIC_L2, "L2"),) if a.kernels else ((H.METRIC_L2, "L2"), (H.METRIC_IP, "IP")):
        hg = H.Hgraph.flat(X, metric=metric)
        cases = [(10, min(1000, a.nq))]
        if not a.kernels:
            cases += [(10, a.nq), (max(10, a.n // 100), min(1000, a.nq))]
        for hits, nq in cases:
            if metric == H.METRIC_L2:
                radius = radius_for(X, Qall, hits)
            else:       # the distance is 1 - product: the median over a few queries of their hits-th smallest
                radius = float(np.median([np.partition(1.0 - (X @ q).astype(np.float64), hits - 1)[hits - 1] for q in Qall[:32]]))
            Q = H.host_empty((nq, d))          # page-locked: read in place
            Q[:] = Qall[:nq]
            t, got = {0: [], 2: []}, {}
            for r in range((2 if a.kernels else steps) + 2):        # (two warm rounds)
                for v in (0, 2):
                    hg.set_option("scan_bytes", v)
                    t0 = time.perf_counter()
                    res = H.Ohnsw.brute_force_range(hg, radius, Q, keep=True)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert hg.scan_path() == (2 if v else 1)
                    if r >= 2:
                        t[v].append(dt)
                    if r == 0:
                        got[v] = res.fetch()
                    res.release()
            for x, y in zip(got[0], got[2]):
                assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
            mean = float(np.diff(got[2][0]).mean())
            disjoint = max(t[2]) < min(t[0]) or max(t[0]) < min(t[2])
            say("%s nq %5d radius %14.3f (mean %9.1f hits per query = %.4f %% of the table, %9d in all): off %8.3f .. %8.3f ms, on %8.3f .. %8.3f ms; "
                "ranges %s; off/on of the medians %.2f; on: %.3f ms per 1 000 queries"
                % (name, nq, radius, mean, 100.0 * mean / a.n, int(got[2][0][-1]), min(t[0]), max(t[0]), min(t[2]), max(t[2]),
                   "disjoint" if disjoint else "overlap", np.median(t[0]) / np.median(t[2]), np.median(t[2]) * 1000.0 / nq))
        hg.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("scan", "search", "matrix", "bytes"), required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("range_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.part in ("matrix", "bytes"):
        (matrix_part if a.part == "matrix" else bytes_part)(a, say)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return

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
