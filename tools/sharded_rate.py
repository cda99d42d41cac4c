#!/usr/bin/env python3
"""What partitioning costs when it is not needed: the C2 shape (1 M x 128 SIFT-like integers, L2, M 16, efC 200, ef 128, k 10),
10 k queries, ONE device.  First hnsw_search_batch on the unsharded index (the single-device path every other tool times), then for
G = 1, 2, 4, 8 shards, all on that device (hnsw_sharded_build with the device listed G times): the build's wall time, the time of
hnsw_sharded_search_batch per batch and its factor over the unsharded call, and beside it where that time goes -- the G searches
alone (hnsw_search_batch on each borrowed shard handle, one after another, summed) and the merge alone (hnsw_merge_lists on those
rows: a host call, so upload, kernel and download of 8 * nq * k bytes per shard).  Recall@k of both answers against the exact scan
is printed too: G graphs of n / G nodes searched with the same ef find more than one graph of n nodes.  Pageable matrices, host
clock, median of --steps calls after a warm one.  Peer copies between DISTINCT devices are not measured here.  Informational:
nothing gates on it.  The table printed here is what profiles/sharded.txt holds.
Usage: python tools/sharded_rate.py [--n 1000000] [--nq 10000] [--steps 5] [--out profiles/sharded.txt]"""
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


def recall(ids, truth):
    return float(np.mean([len(np.intersect1d(a, b)) / len(b) for a, b in zip(ids, truth)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("sharded_rate: no HIP device (there is no CPU path to time)")
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
    t_build = time.time() - t0
    truth, _ = H.Ohnsw.brute_force_knn(hg, k, Q)
    plain = median_ms(lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef), a.steps)
    ids, _ = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
    say("sharded index on ONE device: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries" % (a.n, d, M, efc, ef, k, a.nq))
    say("unsharded: build %5.1f s; hnsw_search_batch %8.3f ms per batch, %7.3f M q/s; recall@%d %.4f"
        % (t_build, plain, a.nq / plain / 1e3, k, recall(ids, truth)))
    hg.release()
    for G in (1, 2, 4, 8):
        t0 = time.time()
        s = H.ShardedHgraph.build(X, M, efc, [0] * G, seed=1, expected_ef=ef)
        t_build = time.time() - t0
        ms = median_ms(lambda: s.knn_batch(Q, ef, k), a.steps)
        shards = [s.shard(g) for g in range(G)]
        searches = sum(median_ms(lambda h=h: H.Ohnsw.knn_batch_bigarray(h, k, Q, ef=ef), a.steps) for h, _ in shards)
        rows = [H.Ohnsw.knn_batch_bigarray(h, k, Q, ef=ef) for h, _ in shards]
        li, ld, first = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), [lo for _, lo in shards]
        merge = median_ms(lambda: H.merge_lists(li, ld, first, k), a.steps)
        got = s.knn_batch(Q, ef, k)
        want = H.merge_lists(li, ld, first, k)
        same = np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        bf, _ = s.brute_force_knn(k, Q)
        say("G %d: build %5.1f s; hnsw_sharded_search_batch %8.3f ms per batch, %7.3f M q/s (%5.2fx the unsharded call's time); the %d "
            "searches alone %8.3f ms, hnsw_merge_lists alone %6.3f ms; recall@%d %.4f; rows equal to the merge of the shards' rows: %s; "
            "exact scan equal to the unsharded one: %s"
            % (G, t_build, ms, a.nq / ms / 1e3, ms / plain, G, searches, merge, k, recall(got[0], truth), "yes" if same else "NO",
               "yes" if np.array_equal(bf, truth.astype(np.int64)) else "NO"))
        s.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
