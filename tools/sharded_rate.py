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
--legs adds the query calls of a sharded index, same shape, same one device (default: knn, the table above):
  filtered  hnsw_sharded_search_batch_filtered at selectivity 1 / 0.1 / 0.01 for G = 1, 2, 4, 8 against hnsw_search_batch_filtered on
            one index of all rows
  range     hnsw_sharded_range_search_batch at a radius that gives about 10 hits per query, same G, against hnsw_range_search_batch
  merge     hnsw_merge_segments alone on 8 lists at about 10 and about 10 000 hits per query: the host call with the result kept on
            the device (upload and kernels, no download) and the bytes it reads and writes; the kernels' own time is what
            `rocprofv3 --kernel-trace --stats -- python tools/sharded_rate.py --legs merge` prints for hnsw_merge_segments_*
Usage: python tools/sharded_rate.py [--n 1000000] [--nq 10000] [--steps 5] [--legs knn,filtered,range,merge] [--out profiles/sharded.txt]"""
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


def merge_leg(say, steps):
    """hnsw_merge_segments alone: 8 lists, segments of equal length, distinct random distances"""
    rng = np.random.default_rng(3)
    for nq, per_list in ((10000, 1), (100, 1250)):             # about 10 and about 10 000 hits per query
        n_lists = 8
        lims = [np.arange(nq + 1, dtype=np.int64) * per_list for _ in range(n_lists)]
        dist = [np.sort(rng.random((nq, per_list), dtype=np.float32), axis=1).reshape(-1) for _ in range(n_lists)]
        ids = [np.tile(np.arange(per_list, dtype=np.int32), nq) for _ in range(n_lists)]
        first = np.arange(n_lists, dtype=np.int64) * per_list
        total = n_lists * nq * per_list
        moved = total * 8 + n_lists * (nq + 1) * 8 + total * 12 + (nq + 1) * 8       # inputs read once, outputs written once

        def call():
            H.merge_segments(lims, ids, dist, first, keep=True).release()
        ms = median_ms(call, steps)
        say("hnsw_merge_segments alone: %d lists, %d queries, %d hits per query: host call (upload, kernels; result kept on the device) "
            "%8.3f ms; %.1f MB read and written by the kernels" % (n_lists, nq, n_lists * per_list, ms, moved / 1e6))


def query_legs(say, a, legs, X, Q, hg, ef, k, M, efc):
    """the filtered and range legs: the unsharded calls on hg, then the sharded ones for G = 1, 2, 4, 8"""
    rng = np.random.default_rng(11)
    masks = [(sel, rng.random(a.n) < sel) for sel in (1.0, 0.1, 0.01)]
    _, d10 = H.Ohnsw.brute_force_knn(hg, 10, Q[:1000])
    radius = float(np.median(d10[:, 9]))                        # about 10 hits per query
    plain_f, plain_r = {}, None
    if "filtered" in legs:
        for sel, m in masks:
            f = hg.filter(m)
            plain_f[sel] = median_ms(lambda: H.Ohnsw.knn_batch_filtered(hg, k, Q, f, ef=ef), a.steps)
            f.release()
            say("unsharded: hnsw_search_batch_filtered at selectivity %.2f %8.3f ms per batch" % (sel, plain_f[sel]))
    if "range" in legs:
        plain_r = median_ms(lambda: H.Ohnsw.range_search(hg, radius, Q, ef=ef), a.steps)
        lims = H.Ohnsw.range_search(hg, radius, Q, ef=ef)[0]
        say("unsharded: hnsw_range_search_batch at radius %.4f (%.1f hits per query) %8.3f ms per batch" % (radius, lims[-1] / a.nq, plain_r))
    for G in (1, 2, 4, 8):
        s = H.ShardedHgraph.build(X, M, efc, [0] * G, seed=1, expected_ef=ef)
        if "filtered" in legs:
            for sel, m in masks:
                f = s.filter(m)
                ms = median_ms(lambda: s.knn_batch_filtered(Q, ef, k, f), a.steps)
                f.release()
                say("G %d: hnsw_sharded_search_batch_filtered at selectivity %.2f %8.3f ms per batch (%5.2fx the unsharded call's time)"
                    % (G, sel, ms, ms / plain_f[sel]))
        if "range" in legs:
            ms = median_ms(lambda: s.range_search(Q, radius, ef=ef), a.steps)
            lims = s.range_search(Q, radius, ef=ef)[0]
            say("G %d: hnsw_sharded_range_search_batch %8.3f ms per batch (%5.2fx the unsharded call's time), %.1f hits per query"
                % (G, ms, ms / plain_r, lims[-1] / a.nq))
        s.release()
    say("all shards on one device; distinct devices: not measured")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="knn")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    if H.device_count() < 1:
        raise SystemExit("sharded_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if "merge" in legs:
        merge_leg(say, a.steps)
    if not legs & {"knn", "filtered", "range"}:
        return finish(a, lines)
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
    if legs & {"filtered", "range"}:
        query_legs(say, a, legs, X, Q, hg, ef, k, M, efc)
    hg.release()
    for G in (1, 2, 4, 8) if "knn" in legs else ():
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
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, "a" if a.legs != "knn" else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
