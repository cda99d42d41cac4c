#!/usr/bin/env python3
"""What option "sq8_rows" buys and costs: float vectors walked as 8-bit codes by the byte-row kernels and re-ranked over the
float32 rows, against the rows each shape reads by default and against half rows with the same re-rank.  Shapes (tools/
half_rows_rate.py's generators): C3's shape with structureless unit vectors (1.18 M x 100, inner product, M 32, ef 256, k 100),
the clustered C3 set (the same shape, 256 directions) and C5's shape (10 M x 96 clustered unit vectors, L2, M 32, ef 512, k 10).
Per shape the rows
    float32 / split rows (the default),  half rows + refine R,  sq8 rows + refine R        for R = 0, 4 k and -1
with queries/s through the host call (hnsw_search_batch) and device-resident (hnsw_search_batch_device on torch buffers), the
launches' ms under option time_kernels (walk + re-rank, and the query transform when no pre-pass runs; the pre-pass -- with the
transform in front of it when it runs -- apart) and recall@k over X for the first 1000
queries against hnsw_brute_force_batch.  (Half rows at R = 0 return the half-row search unrefined.)
Method: one index per shape, every row format on that index; a first call per configuration pays the shape's one-time
decisions and is not timed; medians of --steps calls of a 10 k batch; the device-resident figure is bracketed by events on the
stream the calls run on.  One process, nothing else on the device.  The table printed here is what profiles/sq8_rows.txt holds.
Usage: python tools/sq8_rate.py [--only C3,C3c,C5] [--c5-n 10000000] [--steps 7]"""
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


def random_unit(n, d, seed):
    g = torch.Generator(device=R.DEV)
    g.manual_seed(seed)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        m = min(1 << 20, n - s)
        x = torch.randn((m, d), generator=g, device=R.DEV)
        out[s:s + m] = (x / x.norm(dim=1, keepdim=True)).cpu().numpy()
    return out


def run(tag, X, Q, metric, M, efc, ef, k, steps):
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, metric=metric)
    build_s = time.time() - t0
    Qd = torch.from_numpy(Q).to(R.DEV)
    gt = H.Ohnsw.brute_force_knn(hg, k, Q[:1000])[0]
    print("%s: n %d, d %d, %s, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s" %
          (tag, X.shape[0], X.shape[1], "IP" if metric else "L2", M, efc, ef, k, Q.shape[0], build_s), flush=True)
    base = None
    for option, refines in ((None, (0,)), ("half_rows", (0, 4 * k, -1)), ("sq8_rows", (0, 4 * k, -1))):
        if option:
            t0 = time.time()
            hg.set_option(option, 1)
            print("  %s 1: %.2f s, device_bytes %.3f GB" % (option, time.time() - t0, hg.info().device_bytes / 1e9), flush=True)
        for refine in refines:
            hg.set_option("refine", refine)
            r = R.measure(hg, Q, Qd, ef, k, steps, gt)
            base = base or r
            c = ef if refine < 0 else min(ef, max(k, refine))
            print("  %-8s rows (%4d B/row), refine %3d (%4d re-ranked): host %7.3f M q/s (%.2fx), device-resident %7.3f M q/s (%.2fx), "
                  "launches %.3f ms (+ pre-pass %.3f ms), recall@%d %.4f"
                  % (ROW_NAMES[hg.info().row_format], hg.row_bytes(), refine, c if option else 0, r["host_qps"] / 1e6,
                     r["host_qps"] / base["host_qps"], r["dev_qps"] / 1e6, r["dev_qps"] / base["dev_qps"], r["kernel_ms"], r["prepass_ms"],
                     k, r["recall"]), flush=True)
        if option:
            hg.set_option(option, -1)
    hg.set_option("refine", 0)
    hg.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="C3,C3c,C5")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--c3-n", type=int, default=1_183_514)
    ap.add_argument("--c5-n", type=int, default=10_000_000)
    a = ap.parse_args()
    H.load()
    print("library: %s" % H.LIB_PATH, flush=True)
    only = a.only.split(",")
    if "C3" in only:
        run("C3 shape (structureless unit vectors)", random_unit(a.c3_n, 100, 21), random_unit(a.nq, 100, 121), 1, 32, 200, 256, 100, a.steps)
    if "C3c" in only:
        run("C3 set (clustered unit vectors)", R.clustered_unit(a.c3_n, 100, 12), R.clustered_unit(a.nq, 100, 112), 1, 32, 200, 256, 100,
            a.steps)
    if "C5" in only:
        run("C5 shape (clustered unit vectors)", R.clustered_unit(a.c5_n, 96, 13), R.clustered_unit(a.nq, 96, 113), 0, 32, 200, 512, 10,
            a.steps)


if __name__ == "__main__":
    main()
