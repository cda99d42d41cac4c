#!/usr/bin/env python3
"""What option "refine" costs: the half-row searches with their candidates re-ranked over the float32 rows, against the
unrefined half rows and the rows each shape reads by default, on C2 with byte_rows 0 (1 M x 128, L2, ef 128, k 10) and C3's
shape (1.18 M x 100 clustered unit vectors, inner product, ef 256, k 100) -- tools/half_rows_rate.py's data, calls and
recall.  Per row: q/s through the host call and device-resident, the launches' ms under option time_kernels (search + re-rank),
recall@k over X for the first 1000 queries.  A library without the option (HNSW_LIB_PATH = an older build: the baseline
figures) prints the first two rows only.  Then the re-rank kernel alone: 10 k queries x 128 candidates of the C2 index
(hnsw_rerank_batch_device), its time against the row bytes it gathers.
Usage: python tools/refine_rate.py [--only C2,C3] [--steps 7]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_rows_rate as R  # noqa: E402

H = R.H


def has_refine(hg):
    try:
        hg.set_option("refine", 0)
        return True
    except H.InvalidArgument:
        return False


def rerank_alone(hg, Q, c, steps):
    """the kernel's own time for the candidates a search of ef = c finds, and the rows' bytes over it"""
    nq, d = Q.shape
    hg.set_option("half_rows", 0)
    cand = H.Ohnsw.knn_batch_bigarray(hg, c, Q, ef=c)[0]
    Qd, Cd = torch.from_numpy(Q).to(R.DEV), torch.from_numpy(cand).to(R.DEV)
    ids = torch.empty((nq, c), dtype=torch.int32, device=R.DEV)
    dd = torch.empty((nq, c), dtype=torch.float32, device=R.DEV)
    st = torch.cuda.current_stream()
    ms = []
    for i in range(steps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        H.rerank_device(hg, Qd.data_ptr(), nq, d, Cd.data_ptr(), c, c, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
        b.record(st)
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    t = float(np.median(ms))
    gathered = nq * c * hg.info().row_stride_bytes
    print("  re-rank kernel alone: %d queries x %d candidates, k %d: %.3f ms; %d-byte rows: %.1f MB gathered = %.2f TB/s "
          "(%.0f %% of 8 TB/s HBM peak)" % (nq, c, c, t, hg.info().row_stride_bytes, gathered / 1e6, gathered / t / 1e9,
                                           100 * gathered / t / 1e9 / 8), flush=True)


def run(tag, X, Q, metric, M, efc, ef, k, steps, setup=(), alone=False):
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, metric=metric)
    for name, v in setup:
        hg.set_option(name, v)
    Qd = torch.from_numpy(Q).to(R.DEV)
    gt = R.exact_topk(X, Qd[:1000], k, metric)
    print("%s: n %d, d %d, %s, M %d, efC %d, ef %d, k %d, %d queries" %
          (tag, X.shape[0], X.shape[1], "IP" if metric else "L2", M, efc, ef, k, Q.shape[0]), flush=True)
    rows = [(0, 0), (1, 0)] + ([(1, 2 * k), (1, 4 * k), (1, -1)] if has_refine(hg) else [])
    for half, refine in rows:
        hg.set_option("half_rows", half)
        if refine:
            hg.set_option("refine", refine)
        r = R.measure(hg, Q, Qd, ef, k, steps, gt)
        c = ef if refine < 0 else min(ef, max(k, refine))
        print("  %-8s rows, %-22s host %7.3f M q/s, device-resident %7.3f M q/s, launches %.3f ms (+ pre-pass %.3f ms), recall@%d %.4f"
              % (R.ROW_NAMES[hg.info().row_format], ("refine %d (%d candidates):" % (refine, c)) if refine else "refine off:",
                 r["host_qps"] / 1e6, r["dev_qps"] / 1e6, r["kernel_ms"], r["prepass_ms"], k, r["recall"]), flush=True)
    if alone and has_refine(hg):
        rerank_alone(hg, Q, 128, steps)
    hg.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="C2,C3")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    H.load()
    print("library: %s" % H.LIB_PATH, flush=True)
    only = a.only.split(",")
    if "C2" in only:
        run("C2 (SIFT-like integers, byte rows off)", R.sift_like(1_000_000, 128, 1), R.sift_like(a.nq, 128, 2), 0, 16, 200, 128, 10,
            a.steps, setup=(("byte_rows", 0),), alone=True)
    if "C3" in only:
        run("C3 shape (clustered unit vectors)", R.clustered_unit(1_183_514, 100, 12), R.clustered_unit(a.nq, 100, 112), 1, 32, 200, 256,
            100, a.steps)


if __name__ == "__main__":
    main()
