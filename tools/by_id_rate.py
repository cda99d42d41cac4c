#!/usr/bin/env python3
"""What the searches by stored item cost: the C2 shape (1 M x 128 SIFT-like integers = byte rows, L2, M 16, efC 200, ef 128, k 10),
10 k stored nodes as the queries.  On ONE handle, alternating: hnsw_search_batch_by_id with exclude_self 0 and 1 (40 KB of ids up),
hnsw_search_batch over the same rows from a page-locked matrix and from a pageable one (5 MB up), and the full round trip a caller
wrote before: hnsw_index_get_rows, hnsw_search_batch with k + 1, the strip of the own id in numpy.  Then hnsw_knn_graph of the whole
index against a Python loop of by-id calls over the same chunks.  Host clock around the synchronous host calls, medians of --steps
rounds after a warm round.  The comparison is between calls of the same run on the same handle, never against a recorded number.
--gather-only: the gather kernel alone (hnsw_index_get_rows_device, 10 k rows) against a device-to-device copy of the same bytes,
--steps launches each between two events -- run it under `rocprofv3 --kernel-trace --stats` for the kernel's own time.
Informational: nothing gates on it.  The table printed here is what profiles/by_id.txt holds.
Usage: python tools/by_id_rate.py [--n 1000000] [--nq 10000] [--steps 7] [--gather-only] [--out profiles/by_id.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:   # one HIP runtime per process: torch's bundled copy first, if there is one
    import torch
except ImportError:
    torch = None
import ocaml_hnsw_amd as H  # noqa: E402


def strip_self(ids, dist, own, k):
    """the host side of the round trip: per row the first entry equal to the query's own id (else the last one) removed"""
    hit = ids == own[:, None]
    p = np.where(hit.any(axis=1), hit.argmax(axis=1), k)
    keep = np.arange(k + 1)[None, :] != p[:, None]
    return ids[keep].reshape(-1, k), dist[keep].reshape(-1, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("by_id_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef, k = 128, 16, 200, 128, 10
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    ids = rng.choice(a.n, size=min(a.nq, a.n), replace=False).astype(np.int32)
    nq = len(ids)

    if a.gather_only:
        if torch is None:
            raise SystemExit("by_id_rate --gather-only needs torch for the device buffers")
        hg = H.Hgraph.flat(X)
        dev = torch.device("cuda", 0)
        d_ids = torch.from_numpy(ids).to(dev)
        out = torch.empty((nq, d), dtype=torch.float32, device=dev)
        src = torch.empty((nq, d), dtype=torch.float32, device=dev)
        say("by id, the gather alone: %d rows of %d floats (%d bytes) out of a table of %d rows, %d launches between two events" % (nq, d, nq * d * 4, a.n, a.steps))
        for name, call in (("hnsw_index_get_rows_device", lambda: H.rows_device(hg, d_ids.data_ptr(), nq, out.data_ptr(), d)),
                           ("device-to-device copy of the same bytes", lambda: out.copy_(src))):
            call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                call()
            e1.record()
            torch.cuda.synchronize()
            say("%-42s %8.4f ms per launch" % (name, e0.elapsed_time(e1) / a.steps))
        assert np.array_equal(out.copy_(src).cpu().numpy(), src.cpu().numpy())
        H.rows_device(hg, d_ids.data_ptr(), nq, out.data_ptr(), d)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), X[ids])
        hg.release()
    else:
        t0 = time.time()
        hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
        say("by id: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d stored nodes as the queries; build %.1f s; rows: %d B"
            % (a.n, d, M, efc, ef, k, nq, time.time() - t0, hg.row_bytes()))
        Qp = H.host_empty((nq, d), np.float32)
        Qp[:] = hg.rows(ids)
        Q = np.array(Qp)

        def round_trip():
            R = H.Ohnsw.knn_batch_bigarray(hg, k + 1, hg.rows(ids), ef=ef)
            return strip_self(R[0], R[1], ids, k)

        calls = [("hnsw_search_batch_by_id, exclude_self 0", lambda: H.Ohnsw.knn_batch_by_id(hg, k, ids, ef=ef, exclude_self=False)),
                 ("hnsw_search_batch_by_id, exclude_self 1", lambda: H.Ohnsw.knn_batch_by_id(hg, k, ids, ef=ef)),
                 ("hnsw_search_batch, page-locked matrix", lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Qp, ef=ef)),
                 ("hnsw_search_batch, pageable matrix", lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)),
                 ("get_rows + search k + 1 + strip in numpy", round_trip)]
        # the calls agree before they are timed
        want = calls[2][1]()
        got = calls[0][1]()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        want = round_trip()
        got = calls[1][1]()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        times = [[] for _ in calls]
        for r in range(a.steps + 1):
            for j, (_, call) in enumerate(calls):
                t0 = time.perf_counter()
                call()
                if r:
                    times[j].append((time.perf_counter() - t0) * 1e3)
        say("the calls alternate on one handle, medians of %d rounds after a warm round" % a.steps)
        base = float(np.median(times[2]))
        for (name, _), t in zip(calls, times):
            say("%-42s %8.3f ms per batch (min %.3f, max %.3f): %.3fx the page-locked host call" % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / base))

        chunk = 65536
        t0 = time.perf_counter()
        g = hg.knn_graph(k, ef=ef)
        graph_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        parts = [H.Ohnsw.knn_batch_by_id(hg, k, np.arange(v0, min(v0 + chunk, a.n), dtype=np.int32), ef=ef) for v0 in range(0, a.n, chunk)]
        loop_ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(g[0], np.concatenate([p[0] for p in parts])) and np.array_equal(g[1].view(np.uint32), np.concatenate([p[1] for p in parts]).view(np.uint32))
        say("hnsw_knn_graph of all %d nodes (chunks of %d): %9.1f ms; a Python loop of by-id calls over the same chunks: %9.1f ms (one run each; same rows: %s)"
            % (a.n, chunk, graph_ms, loop_ms, "yes" if same else "NO"))
        hg.release()
    if a.out:
        with open(a.out, "a" if a.gather_only else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
