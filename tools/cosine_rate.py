#!/usr/bin/env python3
"""What HNSW_METRIC_COSINE costs on top of its IP twin: the normaliser in front of the data and of every query batch
(ocaml-hnsw_amd/csrc/hnsw_cosine.hip).  Two tables, recorded and not gated; what is printed here is what profiles/cosine.txt holds.

 (a) the normalise kernel alone: bytes per second (rows read + rows written) over --rows x 128 device-resident float32 rows
     (default 1 M), from the caller's matrix into the handle's scratch as every device-form call runs it.  The kernel has no entry
     point of its own that takes device memory, so it is reached through hnsw_distance_batch_device on a flat COSINE index of one
     row, whose query batch IS the matrix (nq = rows, m = 1); the same call on a flat IP index is the distance launch alone and is
     subtracted.  Events around --reps calls each; beside a device-to-device hipMemcpy of the same bytes timed in the same run;
 (b) the COSINE host call (hnsw_search_batch, 10 k queries) against the IP twin's call on pre-normalised queries, on one data
     set of d = 100 (default 200 k rows, M 16, ef 64, k 10), ALTERNATED call by call in one process: medians of --steps pairs and
     the spread (min .. max) of each side; pageable and page-locked query matrices.

Method: every shape is called once before it is timed; a call ends in the library's own stream synchronisation, so the host clock
brackets finished work; nothing else runs on the device.
The figure of (a) is a difference of two timings whose distance launches read different buffers: an estimate.  The kernel's own
time comes from a kernel trace of table (a) in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cosine_rate.py --only a
(the line of cosine_normalise_kernel in <dir>/**/*kernel_stats.csv).
Usage: python tools/cosine_rate.py [--only a,b] [--rows 1000000] [--n 200000] [--nq 10000] [--steps 15] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocaml_hnsw_amd as H  # noqa: E402

DEV = torch.device("cuda", 0)


def event_ms(fn, reps):
    """ms per call of fn(), `reps` calls between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_rate(rows, reps):
    d = 128
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    X = torch.randn((rows, d), generator=g, device=DEV)
    Y = torch.empty_like(X)
    ids = torch.zeros(rows, dtype=torch.int32, device=DEV)
    out = torch.empty(rows, dtype=torch.float32, device=DEV)
    one = np.ones((1, d), np.float32)
    flat = {m: H.Hgraph.flat(one, metric=m).to_device(0) for m in (H.METRIC_COSINE, H.METRIC_IP)}
    L = H.load()
    st = torch.cuda.current_stream().cuda_stream

    def dist(metric):
        H._check(L.hnsw_distance_batch_device(flat[metric].handle, X.data_ptr(), rows, d, ids.data_ptr(), 1, out.data_ptr(), st or None))

    for m in flat:
        dist(m)                                   # code objects, the handle's scratch
    Y.copy_(X)
    ms_cos = event_ms(lambda: dist(H.METRIC_COSINE), reps)       # normalise (X -> scratch) + the distance launch over the scratch
    ms_ip = event_ms(lambda: dist(H.METRIC_IP), reps)            # the distance launch alone
    ms_copy = event_ms(lambda: Y.copy_(X), reps)                 # hipMemcpy device to device
    nbytes = 2.0 * rows * d * 4
    ms_norm = ms_cos - ms_ip
    print("(a) normalise kernel, %d x %d float32 rows device-resident (%.1f MB read + %.1f MB written), %d launches each:" %
          (rows, d, nbytes / 2e6, nbytes / 2e6, reps))
    print("    normalise + distance launch %.4f ms, distance launch alone %.4f ms -> normalise %.4f ms = %.1f GB/s" %
          (ms_cos, ms_ip, ms_norm, nbytes / ms_norm / 1e6 if ms_norm > 0 else float("nan")))
    print("    device-to-device copy of the same bytes %.4f ms = %.1f GB/s" % (ms_copy, nbytes / ms_copy / 1e6))
    for h in flat.values():
        h.release()


def host_call(n, nq, steps):
    d, M, efc, ef, k = 100, 16, 100, 64, 10
    rng = np.random.default_rng(9)
    centres = rng.normal(size=(256, d)).astype(np.float32)
    X = (centres[rng.integers(0, 256, n)] + 0.35 * rng.normal(size=(n, d)).astype(np.float32)) * rng.uniform(0.5, 20.0, size=(n, 1)).astype(np.float32)
    Q = (centres[rng.integers(0, 256, nq)] + 0.35 * rng.normal(size=(nq, d)).astype(np.float32)) * np.float32(3.0)
    NX, NQ = H.normalise(X), H.normalise(Q)
    t0 = time.time()
    hc = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, metric=H.METRIC_COSINE, expected_ef=ef)
    hi = H.Ohnsw.build_batch_bigarray(NX, M, efc, seed=1, metric=H.METRIC_IP, expected_ef=ef)
    print("(b) host call, n %d, d %d, M %d, efC %d, ef %d, k %d, %d queries per call; both builds %.1f s" % (n, d, M, efc, ef, k, nq, time.time() - t0))
    for where in ("pageable", "page-locked"):
        if where == "page-locked":
            Qc, Qi = H.host_empty((nq, d)), H.host_empty((nq, d))
            Qc[...] = Q
            Qi[...] = NQ
        else:
            Qc, Qi = Q, NQ
        out_c = (np.empty((nq, k), np.int32), np.empty((nq, k), np.float32))
        out_i = (np.empty((nq, k), np.int32), np.empty((nq, k), np.float32))
        for _ in range(3):
            H.Ohnsw.knn_batch_bigarray(hc, k, Qc, ef=ef, out=out_c)
            H.Ohnsw.knn_batch_bigarray(hi, k, Qi, ef=ef, out=out_i)
        same = np.array_equal(out_c[0], out_i[0]) and np.array_equal(out_c[1].view(np.uint32), out_i[1].view(np.uint32))
        tc, ti = [], []
        for _ in range(steps):                     # alternated: other people's work shares the host
            t = time.perf_counter()
            H.Ohnsw.knn_batch_bigarray(hc, k, Qc, ef=ef, out=out_c)
            tc.append(time.perf_counter() - t)
            t = time.perf_counter()
            H.Ohnsw.knn_batch_bigarray(hi, k, Qi, ef=ef, out=out_i)
            ti.append(time.perf_counter() - t)
        tc, ti = np.array(tc) * 1e3, np.array(ti) * 1e3
        print("    %-11s queries: COSINE %.3f ms (%.3f .. %.3f), IP twin on N(Q) %.3f ms (%.3f .. %.3f), ratio %.3f, %d pairs; results %s" %
              (where, np.median(tc), tc.min(), tc.max(), np.median(ti), ti.min(), ti.max(), np.median(tc) / np.median(ti), steps,
               "bit-equal" if same else "DIFFER"))
    hc.release()
    hi.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="a,b", help="which tables; `--only a` under `rocprofv3 --kernel-trace --stats` gives the kernel's own time")
    a = ap.parse_args()
    H.load()
    if H.device_count() < 1:
        raise SystemExit("cosine_rate.py measures on a device: none found")
    print("library: %s" % H.LIB_PATH, flush=True)
    if "a" in a.only.split(","):
        kernel_rate(a.rows, a.reps)
    if "b" in a.only.split(","):
        host_call(a.n, a.nq, a.steps)


if __name__ == "__main__":
    main()
