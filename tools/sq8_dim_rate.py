#!/usr/bin/env python3
"""What option "sq8_dim_rows" buys and costs against "sq8_rows" and the float32 rows, side by side, on two 1 M x 128 L2 sets:
the benchmark's float shape (C2: SIFT-like integers searched with byte_rows 0, tools/half_rows_rate.py's generator) and the
outlier set of tests/test_gpu_sq8_dim.py scaled up (standard normal, 8 rows multiplied by 400 in dimension 0: one map for the
whole table is blind there).  Per set the rows
    float32 rows,  sq8 rows + refine R,  per-dimension sq8 rows + refine R        for R = 0 and 64
at ef 128, k 10, with queries/s through the host call (hnsw_search_batch) and device-resident (hnsw_search_batch_device on torch
buffers), the launches' ms under option time_kernels (walk + re-rank + query transform; the pre-pass apart) and recall@10 over X
for the first 1000 queries against hnsw_brute_force_batch.  The comparison that matters is the L2 walk over the per-dimension
codes against the walk over the sq8 codes ON THE SAME HANDLE: the same bytes gathered, through the byte-row kernels (hand-scheduled
loop, integer path when the query is byte-valued) there and through the C++ hop loop with one more multiply per dimension here.
Method: tools/half_rows_rate.py's measure() -- a first call per configuration is not timed, medians of --steps calls of a 10 k
batch, one process, nothing else on the device.  The table printed here is what profiles/sq8_dim_rows.txt holds.
Usage: python tools/sq8_dim_rate.py [--only C2,outliers] [--n 1000000] [--steps 7]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_rows_rate as R  # noqa: E402

H = R.H
ROW_NAMES = dict(R.ROW_NAMES)
ROW_NAMES[H.ROWS_SQ8] = "sq8"
ROW_NAMES[H.ROWS_SQ8_DIM] = "sq8_dim"


def normal(n, d, seed):
    g = torch.Generator(device=R.DEV)
    g.manual_seed(seed)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        m = min(1 << 20, n - s)
        out[s:s + m] = torch.randn((m, d), generator=g, device=R.DEV).cpu().numpy()
    return out


def run(tag, X, Q, M, efc, ef, k, steps, setup=()):
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1)
    build_s = time.time() - t0
    for name, v in setup:
        hg.set_option(name, v)
    Qd = torch.from_numpy(Q).to(R.DEV)
    gt = H.Ohnsw.brute_force_knn(hg, k, Q[:1000])[0]
    print("%s: n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s%s" %
          (tag, X.shape[0], X.shape[1], M, efc, ef, k, Q.shape[0], build_s, "".join(", %s %d" % s for s in setup)), flush=True)
    base, walk_ms = None, {}
    for option, refines in ((None, (0,)), ("sq8_rows", (0, 64)), ("sq8_dim_rows", (0, 64))):
        if option:
            t0 = time.time()
            hg.set_option(option, 1)
            print("  %s 1: %.2f s, device_bytes %.3f GB" % (option, time.time() - t0, hg.info().device_bytes / 1e9), flush=True)
        for refine in refines:
            hg.set_option("refine", refine)
            r = R.measure(hg, Q, Qd, ef, k, steps, gt)
            base = base or r
            walk_ms[(option, refine)] = r["kernel_ms"]
            print("  %-8s rows (%4d B/row), refine %3d (%4d re-ranked): host %7.3f M q/s (%.2fx), device-resident %7.3f M q/s (%.2fx), "
                  "launches %.3f ms (+ pre-pass %.3f ms), recall@%d %.4f"
                  % (ROW_NAMES[hg.info().row_format], hg.row_bytes(), refine, min(ef, max(k, refine)) if option else 0,
                     r["host_qps"] / 1e6, r["host_qps"] / base["host_qps"], r["dev_qps"] / 1e6, r["dev_qps"] / base["dev_qps"],
                     r["kernel_ms"], r["prepass_ms"], k, r["recall"]), flush=True)
        if option:
            hg.set_option(option, -1)
    for refine in (0, 64):
        print("  L2 walk over the per-dimension codes / over the sq8 codes, refine %d: launches %.2fx the time"
              % (refine, walk_ms[("sq8_dim_rows", refine)] / walk_ms[("sq8_rows", refine)]), flush=True)
    hg.set_option("refine", 0)
    hg.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="C2,outliers")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    H.load()
    only = a.only.split(",")
    if "C2" in only:
        run("C2 (SIFT-like integers, byte rows off)", R.sift_like(a.n, 128, 1), R.sift_like(a.nq, 128, 2), 16, 200, 128, 10, a.steps,
            setup=(("byte_rows", 0),))
    if "outliers" in only:
        X = normal(a.n, 128, 31)
        X[np.random.default_rng(32).choice(a.n, 8, replace=False), 0] *= np.float32(400)
        run("outliers (standard normal, 8 rows x 400 in dimension 0)", X, normal(a.nq, 128, 33), 16, 200, 128, 10, a.steps)


if __name__ == "__main__":
    main()
