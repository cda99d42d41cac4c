#!/usr/bin/env python3
"""What soft deletion (hnsw_index_mark_deleted ... hnsw_index_compact) costs: the C2 shape (1 M x 128 SIFT-like integers, L2, M 16,
efC 200, ef 128, k 10), 10 k queries.  With 0 %, 0.1 %, 1 % and 10 % of the nodes marked (a uniform random set, grown from one
level to the next): queries/s of hnsw_search_batch on the marked handle (pageable matrices, host clock, median of --steps calls
after a warm call) and, beside it, of the explicit hnsw_search_batch_filtered under a host-built mask of the live nodes on a twin
handle that is never marked -- the two run the same code, and their rows are compared once.  Then the same search after
hnsw_index_compact, and the wall time of mark_deleted for 1 and for 10 000 ids and of compact.  Informational: nothing gates on it.
The table printed here is what profiles/soft_delete.txt holds.
Usage: python tools/soft_delete_rate.py [--n 1000000] [--nq 10000] [--steps 5] [--out profiles/soft_delete.txt]"""
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


def once_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("soft_delete_rate: no HIP device (there is no CPU path to time)")
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
    twin = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
    say("soft deletion: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; two builds %.1f s; rows: %d B"
        % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
    search = lambda h: H.Ohnsw.knn_batch_bigarray(h, k, Q, ef=ef)
    plain = median_ms(lambda: search(hg), a.steps)
    say("marked  0     %% (      0 nodes): hnsw_search_batch %8.3f ms per batch, %7.3f M q/s (the plain path)" % (plain, a.nq / plain / 1e3))
    order = np.random.default_rng(11).permutation(a.n)
    t_one = once_ms(lambda: hg.mark_deleted(order[:1]))
    say("mark_deleted of 1 id: %.3f ms (the first mark: the live mask is allocated)" % t_one)
    t_one = once_ms(lambda: hg.mark_deleted(order[1:2]))
    say("mark_deleted of 1 id: %.3f ms" % t_one)
    t_many = once_ms(lambda: hg.mark_deleted(order[2:10002]))
    say("mark_deleted of 10000 ids: %.3f ms" % t_many)
    hg.unmark_deleted(order[:10002])
    assert hg.deleted_count() == 0
    back = median_ms(lambda: search(hg), a.steps)
    say("all unmarked again: hnsw_search_batch %8.3f ms per batch (the plain path again)" % back)
    marked = 0
    for share in (0.001, 0.01, 0.1):
        m = int(round(share * a.n))
        hg.mark_deleted(order[marked:m])
        marked = m
        live = np.ones(a.n, bool)
        live[order[:m]] = False
        flt = twin.filter(live)
        ms = median_ms(lambda: search(hg), a.steps)
        mf = median_ms(lambda: H.Ohnsw.knn_batch_filtered(twin, k, Q, flt, ef=ef), a.steps)
        got, want = search(hg), H.Ohnsw.knn_batch_filtered(twin, k, Q, flt, ef=ef)
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want))
        say("marked %-5g %% (%7d nodes): hnsw_search_batch %8.3f ms per batch, %7.3f M q/s (%.2fx the plain call's time); "
            "hnsw_search_batch_filtered under a host-built live mask %8.3f ms; rows of the two %s"
            % (100 * share, m, ms, a.nq / ms / 1e3, ms / plain, mf, "equal" if same else "DIFFER"))
        flt.release()
    t_compact = once_ms(hg.compact)
    after = median_ms(lambda: search(hg), a.steps)
    say("compact of %d marked nodes: %.1f ms; n %d afterwards" % (marked, t_compact, hg.info().n))
    say("after compact: hnsw_search_batch %8.3f ms per batch, %7.3f M q/s (%.2fx the time before any mark)" % (after, a.nq / after / 1e3, after / plain))
    hg.release()
    twin.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
