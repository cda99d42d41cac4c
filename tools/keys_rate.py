#!/usr/bin/env python3
"""What the keys an index owns cost: the C2 shape (1 M x 128 SIFT-like integers = byte rows, L2, M 16, efC 200, ef 128, k 10), 10 k
queries.  hnsw_search_batch_keyed against hnsw_search_batch on ONE handle, the two calls alternating (the keyed call is the plain
one plus one translate launch over nq * k ids -- nq * k * 12 bytes -- and a download of 8-byte instead of 4-byte rows); then
hnsw_index_set_keys for n keys, hnsw_index_find_keys for 10 k and for n keys, and hnsw_index_remove_keys of 1000 keys against
hnsw_index_remove of the same nodes on a twin handle.  Host clock around the synchronous host calls, pageable arrays, medians of
--steps rounds after a warm round (the removals: one run each, they change the index).  Informational: nothing gates on it.  The
table printed here is what profiles/keys.txt holds.
Usage: python tools/keys_rate.py [--n 1000000] [--nq 10000] [--steps 7] [--out profiles/keys.txt]"""
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


def median_ms(call, steps):
    t = []
    for r in range(steps + 1):
        t0 = time.perf_counter()
        call()
        if r:
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("keys_rate: no HIP device (there is no CPU path to time)")
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
    say("keys: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s; rows: %d B"
        % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
    keys = rng.permutation(a.n).astype(np.int64) * 7919 - (a.n * 7919) // 2          # distinct, both signs, in no order

    ms, lo = median_ms(lambda: hg.set_keys(keys), a.steps)
    say("hnsw_index_set_keys, %d keys (upload, radix sort of the pairs, duplicate check): %8.3f ms (min %.3f); tables: %d bytes"
        % (a.n, ms, lo, hg.keys_info()[1]))

    calls = (lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef), lambda: H.Ohnsw.knn_batch_keyed(hg, k, Q, ef=ef))
    times = [[], []]
    for r in range(a.steps + 1):
        for j, call in enumerate(calls):
            t0 = time.perf_counter()
            call()
            if r:
                times[j].append((time.perf_counter() - t0) * 1e3)
    plain, keyed = float(np.median(times[0])), float(np.median(times[1]))
    say("the two calls alternate on one handle, medians of %d rounds after a warm round" % a.steps)
    say("hnsw_search_batch       %8.3f ms per batch (min %.3f, max %.3f)" % (plain, min(times[0]), max(times[0])))
    say("hnsw_search_batch_keyed %8.3f ms per batch (min %.3f, max %.3f): %.3fx, %+.3f ms" % (keyed, min(times[1]), max(times[1]), keyed / plain, keyed - plain))
    ids = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
    ms, lo = median_ms(lambda: hg.keys(ids), a.steps)
    say("hnsw_index_keys_of for those %d ids from host memory (upload, translate, download): %8.3f ms (min %.3f)" % (ids.size, ms, lo))

    for m in (min(10000, a.n), a.n):
        look = keys[np.random.default_rng(m).integers(0, a.n, m)]
        ms, lo = median_ms(lambda: hg.find_keys(look), a.steps)
        say("hnsw_index_find_keys, %7d keys: %8.3f ms (min %.3f)" % (m, ms, lo))

    gone = np.sort(np.random.default_rng(9).choice(a.n, size=min(1000, a.n // 2), replace=False))
    twin = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
    t0 = time.perf_counter()
    H.Ohnsw.remove_batch(twin, gone)
    by_id = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hg.remove_keys(keys[gone])
    by_key = (time.perf_counter() - t0) * 1e3
    same = np.array_equal(hg.keys(), np.delete(keys, gone))
    say("hnsw_index_remove of %d nodes on a twin without keys: %8.1f ms; hnsw_index_remove_keys of their keys: %8.1f ms (one run each; keys moved: %s)"
        % (len(gone), by_id, by_key, "yes" if same else "NO"))
    twin.release()
    hg.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
