#!/usr/bin/env python3
"""What the paged searches cost: the C2 shape (1 M x 128 SIFT-like integers = byte rows, L2, M 16, efC 200, ef 128, k 10, 10 k
queries).  On ONE handle, the calls of a leg taking turns:
  (a) page 0 -- hnsw_search_batch_after with the start cursor -- against hnsw_search_batch: the price of the ladder's host round trip;
  (b) pages 1 ... 9 fed by out_next against what they replace: ONE hnsw_search_batch at k = 10 (p + 1), ef = max(128, k), sliced;
      and which stage served them;
  (c) a page at rank 2000 (--deep-nq queries): the graph form (the whole ladder, then the exact stage) and the exact form, beside
      hnsw_brute_force_batch with k = 1024 -- which cannot reach rank 2000: its time is printed for scale, not as a comparison.
Host clock around the synchronous host calls, medians of --steps rounds after a warm round; a comparison is between calls of the same
run on the same handle, never against a recorded number.
--scan-only: the exact form alone (start cursor, then a cursor at rank 2000) beside hnsw_brute_force_batch at the same k, --steps
calls each -- run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (hnsw_after_scan_kernel against
hnsw_scan_kernel), in a run of its own.
Informational: nothing gates on it.  The table printed here is what profiles/after.txt holds.
Usage: python tools/after_rate.py [--n 1000000] [--nq 10000] [--deep-nq 1000] [--steps 7] [--scan-only] [--out profiles/after.txt]"""
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
    return "%8.3f ms (min %.3f, max %.3f)" % (float(np.median(t)), min(t), max(t))


def overlap(a, b):
    return "the ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "the ranges do not overlap"


def deep_cursor(hg, Q, rank):
    """the cursor a caller holds after `rank` results, by the exact form (pages of at most 1024)"""
    cur = None
    left = rank
    while left:
        step = min(left, 1024)
        cur = H.Ohnsw.brute_force_after(hg, step, Q, cur)[2]
        left -= step
    return cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--deep-nq", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--scan-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("after_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef, k = 128, 16, 200, 128, 10
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    Qd = Q[:min(a.deep_nq, a.nq)]

    if a.scan_only:
        hg = H.Hgraph.flat(X)
        deep = deep_cursor(hg, Qd, min(2000, a.n // 2))
        say("paged search, the exact form alone: n %d, d %d, L2, k %d, %d queries, %d calls each" % (a.n, d, k, len(Qd), a.steps))
        calls = [lambda: H.Ohnsw.brute_force_knn(hg, k, Qd), lambda: H.Ohnsw.brute_force_after(hg, k, Qd),
                 lambda: H.Ohnsw.brute_force_after(hg, k, Qd, deep)]
        first = calls[0](), calls[1]()
        # (the two orders agree wherever a row's distances are distinct)
        same = np.array_equal(first[0][0], first[1][0])
        t = timed(calls, a.steps)
        for name, x in zip(("hnsw_brute_force_batch", "hnsw_brute_force_batch_after, start cursor", "hnsw_brute_force_batch_after, rank 2000"), t):
            say("%-46s %s per call" % (name, fmt(x)))
        say("start cursor: the same ids as hnsw_brute_force_batch: %s" % ("yes" if same else "no (rows with tied distances)"))
        hg.release()
    else:
        t0 = time.time()
        hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
        say("paged search: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s; rows: %d B"
            % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
        say("the calls of a leg take turns on one handle, medians of %d rounds after a warm round" % a.steps)
        # (a) page 0
        plain = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
        page0 = H.Ohnsw.knn_batch_after(hg, k, Q, ef=ef, counters=True)
        rows_same = int((plain[0] == page0[0]).all(axis=1).sum())
        t = timed([lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef), lambda: H.Ohnsw.knn_batch_after(hg, k, Q, ef=ef)], a.steps)
        say("(a) page 0: hnsw_search_batch %s; hnsw_search_batch_after, start cursor %s: %.2fx, %s; %d of %d rows equal, stages %s"
            % (fmt(t[0]), fmt(t[1]), float(np.median(t[1])) / float(np.median(t[0])), overlap(t[0], t[1]), rows_same, a.nq,
               dict(zip(*[x.tolist() for x in np.unique(page0[5], return_counts=True)]))))
        # (b) pages 1 .. 9
        cur = page0[2]
        for p in range(1, 10):
            kk = k * (p + 1)
            e = max(ef, kk)
            page = H.Ohnsw.knn_batch_after(hg, k, Q, cur, ef=ef, counters=True)
            big = H.Ohnsw.knn_batch_bigarray(hg, kk, Q, ef=e)
            rows_same = int((big[0][:, kk - k:] == page[0]).all(axis=1).sum())
            held = cur
            t = timed([lambda: H.Ohnsw.knn_batch_bigarray(hg, kk, Q, ef=e), lambda: H.Ohnsw.knn_batch_after(hg, k, Q, held, ef=ef)], a.steps)
            stages = dict(zip(*[x.tolist() for x in np.unique(page[5], return_counts=True)]))
            say("(b) page %d: hnsw_search_batch k %3d ef %3d, sliced %s; hnsw_search_batch_after %s: %.2fx, %s; %d of %d rows equal; stages %s"
                % (p, kk, e, fmt(t[0]), fmt(t[1]), float(np.median(t[1])) / float(np.median(t[0])), overlap(t[0], t[1]), rows_same, a.nq, stages))
            cur = page[2]
        # (c) a page at rank 2000
        deep = deep_cursor(hg, Qd, min(2000, a.n // 2))
        got = H.Ohnsw.knn_batch_after(hg, k, Qd, deep, ef=ef, counters=True)
        want = H.Ohnsw.brute_force_after(hg, k, Qd, deep)
        # (W_1024 is a walk's W: where it holds k nodes beyond rank 2000 the ladder serves the query; the others are the exact stage's)
        ex = got[5] == H.STAGE_EXACT
        assert np.array_equal(got[0][ex], want[0][ex]) and np.array_equal(got[1][ex].view(np.uint32), want[1][ex].view(np.uint32))
        stages = dict(zip(*[x.tolist() for x in np.unique(got[5], return_counts=True)]))
        t = timed([lambda: H.Ohnsw.knn_batch_after(hg, k, Qd, deep, ef=ef), lambda: H.Ohnsw.brute_force_after(hg, k, Qd, deep),
                   lambda: H.Ohnsw.brute_force_knn(hg, min(1024, a.n), Qd)], max(2, a.steps // 2))
        say("(c) a page at rank 2000, %d queries: hnsw_search_batch_after (the ladder 128 ... 1024, then the exact stage) %s; "
            "hnsw_brute_force_batch_after %s; for scale, hnsw_brute_force_batch at k = 1024 %s -- it cannot reach rank 2000, so there is no call to compare with; "
            "stages %s, %d of %d rows equal to the exact form's"
            % (len(Qd), fmt(t[0]), fmt(t[1]), fmt(t[2]), stages, int((got[0] == want[0]).all(axis=1).sum()), len(Qd)))
        hg.release()
    if a.out:
        with open(a.out, "a" if a.scan_only else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
