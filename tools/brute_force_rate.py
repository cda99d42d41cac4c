#!/usr/bin/env python3
"""What the exact scan (hnsw_brute_force_batch) costs: generated data from a seed, runs only with a device.

  (a) C2 shape, 1 M x 128, L2, k 10, at nq = 10, 1 000 and 10 000;   (b) C3 shape, 1.18 M x 100, IP, k 100, nq = 1 000;
  (c) the bench_dist shape, 60 000 x 784, L2, k 10, nq = 10 000.
For each: the host call (pageable matrices, host clock) and the device-resident call (HIP events), warmed, >= 20 repetitions with
their spread; pairs/s; and the share of the fp32 vector peak (157.3 TFLOPS): the least time is nq * n * d * (2 lane operations
for L2, 1 for IP) over that rate -- the scan is bound by arithmetic, not by bytes (each row chunk is used for a tile of queries).
At C2 / nq 1 000 also, alternating with the scan: the one other route to the same bits, hnsw_distance_batch over all n ids per
query followed by torch.topk, in its device form (its host form moves 2 * 4 * nq * n bytes = 8 GB over PCIe: 150 ms at 54 GB/s);
and torch's matmul + topk (bench.brute_force_topk; other bits: for information).
Usage: python tools/brute_force_rate.py [--reps 20] [--out profiles/brute_force_rate.txt]"""
import argparse
import os
import sys
import time

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ocaml_hnsw_amd as H  # noqa: E402

PEAK = 157.3e12
PCIE_FLOOR_MS = 2 * 4 * 1000 * 1_000_000 / 54e9 * 1e3


def spread(ms):
    ms = np.sort(np.asarray(ms))
    return "median %.3f ms (min %.3f, max %.3f, n %d)" % (np.median(ms), ms[0], ms[-1], len(ms))


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("brute_force_rate: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("hnsw_brute_force_batch: %s, fp32 vector peak %.1f TFLOPS" % (torch.cuda.get_device_name(0), PEAK / 1e12))
    shapes = [("C2", 1_000_000, 128, H.METRIC_L2, 10, (10, 1000, 10000)), ("C3", 1_180_000, 100, H.METRIC_IP, 100, (1000,)),
              ("bench_dist", 60_000, 784, H.METRIC_L2, 10, (10000,))]
    for name, n, d, metric, k, nqs in shapes:
        rng = np.random.default_rng(7)
        if metric == H.METRIC_L2:
            X = rng.integers(0, 219, size=(n, d), dtype=np.uint8).astype(np.float32)
            Qall = rng.integers(0, 219, size=(max(nqs), d), dtype=np.uint8).astype(np.float32)
        else:
            X = rng.standard_normal((n, d), dtype=np.float32)
            X /= np.linalg.norm(X, axis=1, keepdims=True)
            Qall = rng.standard_normal((max(nqs), d), dtype=np.float32)
            Qall /= np.linalg.norm(Qall, axis=1, keepdims=True)
        hg = H.Hgraph.flat(X, metric=metric).to_device(0)
        for nq in nqs:
            Q = np.ascontiguousarray(Qall[:nq])
            Qd = torch.from_numpy(Q).to(dev)
            ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
            dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
            scan = lambda: H.brute_force_device(hg, Qd.data_ptr(), nq, d, k, ids.data_ptr(), dd.data_ptr())
            for _ in range(3):
                scan()
                H.Ohnsw.brute_force_knn(hg, k, Q)
            torch.cuda.synchronize()
            t_dev = events(scan, a.reps)
            t_host = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                hi, hd = H.Ohnsw.brute_force_knn(hg, k, Q)
                t_host.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(hi, ids.cpu().numpy()) and np.array_equal(hd.view(np.uint32), dd.cpu().numpy().view(np.uint32))
            ops = nq * n * d * (2 if metric == H.METRIC_L2 else 1)
            med = float(np.median(t_dev))
            say("%s n %d d %d %s k %d nq %d" % (name, n, d, "L2" if metric == H.METRIC_L2 else "IP", k, nq))
            say("  device-resident call: %s; %.3g pairs/s; least time %.3f ms = %.1f %% of the fp32 vector peak (arithmetic-bound)"
                % (spread(t_dev), nq * n / (med * 1e-3), ops / PEAK * 1e3, 100 * ops / PEAK / (med * 1e-3)))
            say("  host call:            %s" % spread(t_host))
            if name == "C2" and nq == 1000:
                # the other route to the same bits: every distance through hnsw_distance_batch, then topk -- 64 queries at a time
                # (nq * n floats at once are 4 GB), alternating with the scan
                all_ids = torch.arange(n, dtype=torch.int32, device=dev).repeat(64, 1).contiguous()
                dist = torch.empty((64, n), dtype=torch.float32, device=dev)
                L = H.load()

                def gather_topk():
                    for s in range(0, nq, 64):
                        m = min(64, nq - s)
                        H._check(L.hnsw_distance_batch_device(hg.handle, Qd.data_ptr() + 4 * d * s, m, d, all_ids.data_ptr(), n, dist.data_ptr(), None))
                        torch.topk(dist[:m], k, dim=1, largest=False)
                sys.path.insert(0, ROOT)
                import bench
                Xd = torch.from_numpy(X).to(dev)
                matmul = lambda: bench.brute_force_topk(Xd, Qd, k)
                gather_topk(); matmul()
                torch.cuda.synchronize()
                t_scan, t_gather, t_mm = [], [], []
                for _ in range(max(5, a.reps // 4)):
                    t_scan += events(scan, 1)
                    t_gather += events(gather_topk, 1)
                    t_mm += events(matmul, 1)
                say("  alternating: scan %s" % spread(t_scan))
                say("               hnsw_distance_batch_device over all n + torch.topk %s" % spread(t_gather))
                say("               torch matmul + topk (other bits, for information) %s" % spread(t_mm))
                say("  PCIe floor of that route's host form (8 GB at 54 GB/s): %.0f ms; the scan's host call: %.3f ms" % (PCIE_FLOOR_MS, float(np.median(t_host))))
                assert float(np.median(t_host)) < PCIE_FLOOR_MS, "the host call is not below the other route's transfer floor"
                assert float(np.median(t_scan)) < float(np.median(t_gather)), "the scan is not faster than distance_batch + topk"
                del Xd, all_ids, dist
        hg.release()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
