#!/usr/bin/env python3
"""What option "scan_matrix" (the exact scan of float rows screened by fp32 matrix instructions, hnsw_scan_matrix.hip) buys: the
table of profiles/scan_matrix.txt.  Generated data from a seed; runs only with a device.

One handle per leg; option off (the float scan: the code path without the option) and on alternate within the process, each
timing is one hnsw_brute_force_batch_device call between HIP events, REPS (>= 5) timings per leg, reported as ranges.
  gauss    1 M x 128 Gaussian float rows, L2
  shifted  the same rows and queries + 100: norms far above the distances, where the margin must bite
  ip       1.18 M x 100 Gaussian rows, inner product (the C3 shape)
each at 10 / 1 000 / 10 000 queries with k 10 and 1 000 queries with k 100.
  --kernels: a few calls per option at 1 000 queries and nothing else, to be run under a kernel trace, in a run of its own.
Every on/off pair is also compared: ids and distance bits must be equal.
Usage: python tools/scan_matrix_rate.py [--reps 7] [--out profiles/scan_matrix.txt] [--kernels] [--legs gauss,shifted,ip]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ocaml_hnsw_amd as H  # noqa: E402

LEGS = {"gauss": (1_000_000, 128, H.METRIC_L2, 0.0), "shifted": (1_000_000, 128, H.METRIC_L2, 100.0), "ip": (1_180_000, 100, H.METRIC_IP, 0.0)}


def rng_range(ms):
    return "%8.3f .. %8.3f ms" % (min(ms), max(ms))


def overlap(a, b):
    return "ranges overlap" if min(a) <= max(b) and min(b) <= max(a) else "ranges disjoint"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--legs", default="gauss,shifted,ip")
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("scan_matrix_rate: no HIP device (there is no CPU path to time)")
    reps = max(5, a.reps)
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('option "scan_matrix" off / on, one handle, alternating: %s, %d timings per leg' % (torch.cuda.get_device_name(0), reps))
    for leg in a.legs.split(","):
        n, d, metric, shift = LEGS[leg]
        rng = np.random.default_rng(11)
        X = rng.standard_normal((n, d), dtype=np.float32) + np.float32(shift)
        Qall = rng.standard_normal((10000, d), dtype=np.float32) + np.float32(shift)
        hg = H.Hgraph.flat(X, metric=metric).to_device(0)
        del X
        for nq, k in ((1000, 10),) if a.kernels else ((10, 10), (1000, 10), (10000, 10), (1000, 100)):
            Qd = torch.from_numpy(np.ascontiguousarray(Qall[:nq])).to(dev)
            out = {v: (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)) for v in (0, 1)}
            t = {0: [], 1: []}
            for r in range(reps + 2):           # (two warm-up rounds)
                for v in (0, 1):
                    hg.set_option("scan_matrix", v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    H.brute_force_device(hg, Qd.data_ptr(), nq, d, k, out[v][0].data_ptr(), out[v][1].data_ptr())
                    e1.record()
                    e1.synchronize()
                    assert hg.scan_path() == (H.SCAN_PATH_MATRIX if v else H.SCAN_PATH_FLOAT)
                    if r >= 2:
                        t[v].append(e0.elapsed_time(e1))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
            say("%-7s %d x %d %s nq %5d k %3d: off %s, on %s; %s; off/on of the medians %.2f"
                % (leg, n, d, "L2" if metric == H.METRIC_L2 else "IP", nq, k, rng_range(t[0]), rng_range(t[1]), overlap(t[0], t[1]), np.median(t[0]) / np.median(t[1])))
        hg.release()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
