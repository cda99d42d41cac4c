#!/usr/bin/env python3
"""What the three exact scans cost at the row widths the other yardsticks do not reach: d 32 (NCH 1), 300 (NCH 8), 600 (NCH 16)
beside tools/brute_force_rate.py and tools/range_rate.py (d 100, 128, 784), both metrics.  n Gaussian rows, nq queries; per (d,
metric) the host-call median, least and greatest of --steps calls after two warm ones: the k-scan (hnsw_brute_force_batch, k 10),
the range scan (hnsw_range_brute_force_batch at a radius with about 100 hits per query) and the masked scan
(hnsw_search_batch_filtered over 5 allowed rows: fewer than k, so the exact stage at once -- the call is the walk over the mask's
words).  Informational: nothing gates on it.  Runs only with a device.
Usage: python tools/scan_family_rate.py [--tag NAME] [--n 200000] [--nq 2000] [--d 32,300,600] [--steps 9] [--out FILE (appended to)]"""
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


def spread(fn, steps):
    fn()
    fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    out = np.sort(out)
    return "median %8.3f ms (min %8.3f, max %8.3f)" % (np.median(out), out[0], out[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--d", default="32,300,600")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("scan_family_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for d in (int(x) for x in a.d.split(",")):
        rng = np.random.default_rng(d)
        X = rng.standard_normal((a.n, d), dtype=np.float32)
        Q = rng.standard_normal((a.nq, d), dtype=np.float32)
        mask = np.zeros(a.n, bool)
        mask[[0, 31, 32, a.n // 2, a.n - 1]] = True
        for metric, name in ((H.METRIC_L2, "L2"), (H.METRIC_IP, "IP")):
            hg = H.Hgraph.flat(X, metric=metric)
            radius = float(np.median(H.Ohnsw.brute_force_knn(hg, 100, Q[:64])[1][:, 99]))
            flt = hg.filter(mask)
            head = "%s d %3d %s n %d nq %d" % (a.tag, d, name, a.n, a.nq)
            say("%s k-scan      %s" % (head, spread(lambda: H.Ohnsw.brute_force_knn(hg, 10, Q), a.steps)))
            say("%s range scan  %s" % (head, spread(lambda: H.Ohnsw.brute_force_range(hg, radius, Q), a.steps)))
            say("%s masked scan %s" % (head, spread(lambda: H.Ohnsw.knn_batch_filtered(hg, 10, Q, flt, ef=16), a.steps)))
            flt.release()
            hg.release()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
