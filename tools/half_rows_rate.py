#!/usr/bin/env python3
"""Half rows (option "half_rows") against the rows each shape reads by default, on the float shapes of the benchmark:
C2 with byte_rows 0 (SIFT-like, 1 M x 128, L2, M 16, ef 128, k 10: float32 rows), C3's shape (1.18 M x 100 clustered unit
vectors, inner product, M 32, ef 256, k 100: split rows) and C5's (10 M x 96 clustered unit vectors, L2, M 32, ef 512, k 10:
float32 rows).  Per shape and row format: q/s through the host call (hnsw_search_batch) and device-resident
(hnsw_search_batch_device on torch buffers), the search kernel's ms under option time_kernels (pre-pass apart), and
recall@k over the first 1000 queries against exact ground truth computed with torch on the device -- recall of the search
over X, so the half rows' loss of precision shows.  Medians of --steps calls of a 10 k batch.
Usage: python tools/half_rows_rate.py [--only C2,C3,C5] [--c5-n 10000000] [--steps 7]"""
import argparse
import os
import sys
import time

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ocaml_hnsw_amd as H  # noqa: E402

DEV = torch.device("cuda", 0)
ROW_NAMES = {H.ROWS_F32: "float32", H.ROWS_BYTES: "bytes", H.ROWS_SPLIT: "split", H.ROWS_HALF: "half"}


def sift_like(n, d, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(1234)
    cen = torch.randint(20, 200, (4096, d), generator=g, device=DEV).float()
    g.manual_seed(seed)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        m = min(1 << 20, n - s)
        x = cen[torch.randint(0, 4096, (m,), generator=g, device=DEV)] + 25 * torch.randn((m, d), generator=g, device=DEV)
        out[s:s + m] = torch.clamp(torch.round(x), 0, 218).cpu().numpy()
    return out


def clustered_unit(n, d, seed, centres=256, spread=1.5):
    g = torch.Generator(device=DEV)
    g.manual_seed(4321)
    cen = torch.randn((centres, d), generator=g, device=DEV)
    cen = cen / cen.norm(dim=1, keepdim=True)
    g.manual_seed(seed)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        m = min(1 << 20, n - s)
        x = cen[torch.randint(0, centres, (m,), generator=g, device=DEV)] + spread * torch.randn((m, d), generator=g, device=DEV) / d ** 0.5
        out[s:s + m] = (x / x.norm(dim=1, keepdim=True)).cpu().numpy()
    return out


def exact_topk(X, Qd, k, metric):
    best_v = best_i = None
    for s in range(0, X.shape[0], 1 << 20):
        xb = torch.from_numpy(X[s:s + (1 << 20)]).to(DEV)
        sc = Qd @ xb.T if metric else -((xb * xb).sum(1)[None, :] - 2.0 * (Qd @ xb.T))
        v, i = torch.topk(sc, min(k, xb.shape[0]), dim=1)
        i = i + s
        if best_v is not None:
            v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            o = torch.topk(v, k, dim=1).indices
            v, i = torch.gather(v, 1, o), torch.gather(i, 1, o)
        best_v, best_i = v, i
        del xb, sc
    return best_i.cpu().numpy()


def recall(ids, gt, k):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, gt)]))


def measure(hg, Q, Qd, ef, k, steps, gt):
    nq, d = Q.shape
    ids_t = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    dist_t = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream()

    def dev_call():
        H.search_batch_device(hg, Qd.data_ptr(), nq, d, ef, k, ids_t.data_ptr(), dist_t.data_ptr(), stream=st.cuda_stream)
    ids, _ = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)          # (first call: one-time decisions of the shape)
    host = []
    for _ in range(steps):
        t = time.perf_counter()
        H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
        host.append(time.perf_counter() - t)
    dev_call()
    torch.cuda.synchronize()
    hg.set_option("time_kernels", 1)
    hg.kernel_times()
    devt = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        dev_call()
        b.record(st)
        torch.cuda.synchronize()
        devt.append(a.elapsed_time(b) * 1e-3)
    kern_ms, pre_ms, _ = hg.kernel_times()
    hg.set_option("time_kernels", 0)
    return {"host_qps": nq / float(np.median(host)), "dev_qps": nq / float(np.median(devt)), "kernel_ms": kern_ms,
            "prepass_ms": pre_ms, "recall": recall(ids[:len(gt)], gt, k), "ids": ids}


def run(tag, X, Q, metric, M, efc, ef, k, steps, setup=()):
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, metric=metric)
    build_s = time.time() - t0
    for name, v in setup:
        hg.set_option(name, v)
    Qd = torch.from_numpy(Q).to(DEV)
    gt = exact_topk(X, Qd[:1000], k, metric)
    print("%s: n %d, d %d, %s, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s%s" %
          (tag, X.shape[0], X.shape[1], "IP" if metric else "L2", M, efc, ef, k, Q.shape[0], build_s,
           "".join(", %s %d" % s for s in setup)), flush=True)
    res = {}
    for half in (0, 1):
        hg.set_option("half_rows", half)
        fmt = ROW_NAMES[hg.info().row_format]
        r = measure(hg, Q, Qd, ef, k, steps, gt)
        res[half] = r
        print("  %-8s rows (%4d B/row): host %7.3f M q/s, device-resident %7.3f M q/s, kernel %.3f ms (+ pre-pass %.3f ms), recall@%d %.4f"
              % (fmt, hg.row_bytes(), r["host_qps"] / 1e6, r["dev_qps"] / 1e6, r["kernel_ms"], r["prepass_ms"], k, r["recall"]), flush=True)
    same = float(np.mean(res[0]["ids"] == res[1]["ids"]))
    print("  half / current: host %.3fx, device-resident %.3fx, kernel %.3fx; recall %+.4f; ids equal to the current rows' %.4f"
          % (res[1]["host_qps"] / res[0]["host_qps"], res[1]["dev_qps"] / res[0]["dev_qps"], res[0]["kernel_ms"] / res[1]["kernel_ms"],
             res[1]["recall"] - res[0]["recall"], same), flush=True)
    hg.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="C2,C3,C5")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--c5-n", type=int, default=10_000_000)
    a = ap.parse_args()
    H.load()
    only = a.only.split(",")
    if "C2" in only:
        run("C2 (SIFT-like integers, byte rows off)", sift_like(1_000_000, 128, 1), sift_like(a.nq, 128, 2), 0, 16, 200, 128, 10,
            a.steps, setup=(("byte_rows", 0),))
    if "C3" in only:
        run("C3 shape (clustered unit vectors)", clustered_unit(1_183_514, 100, 12), clustered_unit(a.nq, 100, 112), 1, 32, 200, 256,
            100, a.steps)
    if "C5" in only:
        run("C5 shape (clustered unit vectors)", clustered_unit(a.c5_n, 96, 13), clustered_unit(a.nq, 96, 113), 0, 32, 200, 512, 10,
            a.steps)


if __name__ == "__main__":
    main()
