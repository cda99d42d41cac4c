#!/usr/bin/env python3
"""What grouped search (hnsw_search_batch_grouped) costs: the C2 shape (1 M x 128 SIFT-like integers, L2, M 16, efC 200, ef 128,
k 10), 10 k queries, three labelings of the nodes -- all distinct (every node its own group), uniform random groups of 10 nodes,
and the generator's own clusters (256 groups of ~3900 nodes) -- each set against two baselines on the same handle in the same run,
the three calls alternating: hnsw_search_batch with (ef, k), and hnsw_search_batch_filtered under an all-ones mask (the same ladder
with the filtered select rule; the all-distinct labeling is that walk plus one select of its own).  Per labeling: ms per batch
through the host call (pageable matrices, host clock, median of --steps rounds after a warm round) and the share of queries per
stage.  Then the exact stage alone (hnsw_brute_force_batch_grouped, --exact-queries queries): ms per query for uniform random
labels over n_labels = 10^3, 10^5 and 10^6.  Informational: nothing gates on it.  The table printed here is what
profiles/grouped.txt holds.
Usage: python tools/group_rate.py [--n 1000000] [--nq 10000] [--steps 7] [--exact-queries 64] [--out profiles/grouped.txt]"""
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


def stage_shares(stage, nq):
    values, counts = np.unique(stage, return_counts=True)
    return ", ".join("%s %.1f %%" % ("exact" if v == H.STAGE_EXACT else "stage %d" % v, 100.0 * c / nq) for v, c in zip(values, counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--exact-queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("group_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef, k = 128, 16, 200, 128, 10
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    cluster = rng.integers(0, 256, a.n)
    X = np.clip(np.rint(centres[cluster] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
    say("hnsw_search_batch_grouped: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s; rows: %d B"
        % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
    ones = hg.filter(np.ones(a.n, bool))
    labelings = (("all distinct", np.arange(a.n), a.n),
                 ("random groups of 10", np.random.default_rng(8).integers(0, a.n // 10, a.n), a.n // 10),
                 ("the generator's clusters", cluster, 256))
    say("per labeling the three calls alternate, medians of %d rounds after a warm round" % a.steps)
    for name, lab, n_labels in labelings:
        t0 = time.perf_counter()
        L = hg.labels(lab, n_labels)
        made = (time.perf_counter() - t0) * 1e3
        calls = (lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef),
                 lambda: H.Ohnsw.knn_batch_filtered(hg, k, Q, ones, ef=ef),
                 lambda: H.Ohnsw.knn_batch_grouped(hg, k, Q, L, ef=ef))
        times = [[], [], []]
        for r in range(a.steps + 1):
            for j, call in enumerate(calls):
                t0 = time.perf_counter()
                call()
                if r:
                    times[j].append((time.perf_counter() - t0) * 1e3)
        plain, filt, grp = (float(np.median(t)) for t in times)
        stage = H.Ohnsw.knn_batch_grouped(hg, k, Q, L, ef=ef, counters=True)[5]
        info = L.info()
        say("%-24s (%7d groups, labels made in %.1f ms): grouped %8.3f ms per batch (min %.3f); hnsw_search_batch %8.3f ms (%.2fx); "
            "hnsw_search_batch_filtered under an all-ones mask %8.3f ms (%.2fx); %s"
            % (name, info[2], made, grp, min(times[2]), plain, grp / plain, filt, grp / filt, stage_shares(stage, a.nq)))
        L.release()
    ones.release()
    nx = min(a.exact_queries, a.nq)
    say("the exact stage alone (hnsw_brute_force_batch_grouped, k %d, %d queries, uniform random labels), beside hnsw_brute_force_batch" % (k, nx))
    t_scan = []
    for r in range(a.steps + 1):
        t0 = time.perf_counter()
        H.Ohnsw.brute_force_knn(hg, k, Q[:nx])
        if r:
            t_scan.append((time.perf_counter() - t0) * 1e3)
    say("hnsw_brute_force_batch: %.3f ms per query" % (float(np.median(t_scan)) / nx))
    for n_labels in (1000, 100000, 1000000):
        L = hg.labels(np.random.default_rng(n_labels).integers(0, n_labels, a.n), n_labels)
        t = []
        for r in range(a.steps + 1):
            t0 = time.perf_counter()
            H.Ohnsw.brute_force_grouped(hg, k, Q[:nx], L)
            if r:
                t.append((time.perf_counter() - t0) * 1e3)
        say("n_labels %7d (%7d in use): %8.3f ms per query (min %.3f)" % (n_labels, L.info()[2], float(np.median(t)) / nx, min(t) / nx))
        L.release()
    hg.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
