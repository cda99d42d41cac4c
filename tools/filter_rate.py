#!/usr/bin/env python3
"""What filtered search (hnsw_search_batch_filtered) costs: the C2 shape (1 M x 128 SIFT-like integers, L2, M 16, efC 200, ef 128,
k 10), 10 k queries, a uniform random allow-mask of selectivity 1.0 / 0.5 / 0.1 / 0.01 / 0.001.  Per selectivity: queries/s through
the host call (pageable matrices, host clock, median of --steps calls after a warm call), the share of queries served per stage
(0, 1, ... = how often W doubled; exact = the masked scan), and recall@10 of the first --recall-queries queries against the
exact scan over the allowed vectors alone (a flat index of X[mask]: the same order, ids mapped back).  Beside them the unfiltered
hnsw_search_batch rate of the same handle.  Informational: nothing gates on it.  The table printed here is what
profiles/filtered_search.txt holds.
Usage: python tools/filter_rate.py [--n 1000000] [--nq 10000] [--steps 5] [--out profiles/filtered_search.txt]"""
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


def median_ms(fn, steps):
    fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("filter_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef, k = 128, 16, 200, 128, 10
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
    say("hnsw_search_batch_filtered: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s; rows: %d B"
        % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
    plain = median_ms(lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef), a.steps)
    say("unfiltered hnsw_search_batch: %.3f ms per batch, %.3f M q/s" % (plain, a.nq / plain / 1e3))
    nr = min(a.recall_queries, a.nq)
    for sel in (1.0, 0.5, 0.1, 0.01, 0.001):
        mask = np.ones(a.n, bool) if sel >= 1.0 else np.random.default_rng(int(sel * 1e6)).random(a.n) < sel
        flt = hg.filter(mask)
        ms = median_ms(lambda: H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef), a.steps)
        ids, _, _, _, stage = H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef, counters=True)
        allowed = np.flatnonzero(mask)
        sub = H.Hgraph.flat(X[mask])
        truth = allowed[H.Ohnsw.brute_force_knn(sub, k, Q[:nr])[0]]
        sub.release()
        hits = np.mean([len(set(x) & set(y)) for x, y in zip(ids[:nr], truth)]) / k
        values, counts = np.unique(stage, return_counts=True)
        shares = ", ".join("%s %.1f %%" % ("exact" if v == H.STAGE_EXACT else "stage %d" % v, 100.0 * c / a.nq) for v, c in zip(values, counts))
        say("selectivity %-5g (%7d allowed): %8.3f ms per batch, %7.3f M q/s (%.2fx the unfiltered call); %s; recall@%d %.4f"
            % (sel, flt.count(), ms, a.nq / ms / 1e3, plain / ms, shares, k, hits))
        flt.release()
    hg.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
