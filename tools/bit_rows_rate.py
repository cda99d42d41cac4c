#!/usr/bin/env python3
"""What option "bit_rows" buys and costs on WIDE rows, where a float32 row is 16 or 32 128-byte lines, its per-dimension sq8 codes
4 or 8, and its bits half a line or one: the repository's clustered generator (tools/half_rows_rate.py: unit vectors around 256
directions) at d = 1024 and d = 512, n = 200 000, inner product, M 16, 10 k queries.  ONE handle per set; the row formats
    float32 rows,  sq8_dim_rows + refine R,  bit_rows 1 (means) + refine R,  bit_rows 2 (signs) + refine R
are switched on that handle, at ef in {128, 256, 512} and R in {0, 4 k, -1}, k 10.  Per configuration:
  * call: ms per 10 k batch of the whole device-resident call (hnsw_search_batch_device on torch buffers, device events around it,
    the stream synchronised): query transform + pre-pass + walk + re-rank;
  * launches: ms of the search launches alone under option time_kernels (the walk and the re-rank of c behind it; at R = 0 the re-rank
    reads k rows per query, so that figure is the walk's; the ordering pre-pass is listed apart);
  * recall@10 over the first 1000 queries against hnsw_brute_force_batch.
Method: every configuration is warmed by one untimed call; the configurations are visited in --rounds rounds, alternating the formats
inside each round, --steps timed calls per visit; the figure is the median over all of a configuration's calls and the spread its
min .. max.  One process, nothing else of ours on the device.  The table printed here is what profiles/bit_rows.txt holds.
--query-bits: the leg of option "bit_query_bits" instead (profiles/bit_query_bits.txt): the formats are sq8_dim_rows, bit_rows 1 with
the query at one bit (the Hamming walk) and bit_rows 1 with bit_query_bits 4 (the same rows against the 4-bit query), alternated
on the one handle, at refine -1 and 40.  The pre-pass column holds the query transform as well (it is queued behind the first event),
so its difference between the two bit formats bounds what the 4-bit transform and the descent against the planes cost.
Usage: python tools/bit_rows_rate.py [--dims 1024,512] [--n 200000] [--rounds 3] [--steps 5] [--query-bits]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_rows_rate as R  # noqa: E402

H = R.H
K = 10
FORMATS = (("float32", None, 0, 0), ("sq8_dim", "sq8_dim_rows", 1, 0), ("bits/mean", "bit_rows", 1, 0), ("bits/sign", "bit_rows", 2, 0))
# (name, option, value, bit_query_bits) of the --query-bits leg
QUERY_BITS_FORMATS = (("float32", None, 0, 0), ("sq8_dim", "sq8_dim_rows", 1, 0), ("bits/q1", "bit_rows", 1, 0), ("bits/q4", "bit_rows", 1, 4))


def switch(hg, option, value, query_bits=0):
    for other in ("sq8_dim_rows", "bit_rows"):
        hg.set_option(other, -1 if other == "sq8_dim_rows" else 0)
    hg.set_option("bit_query_bits", query_bits)
    if option:
        hg.set_option(option, value)


def timed(hg, Qd, ef, ids_t, dist_t, steps):
    """(ms per device-resident call, ms of its search launches, ms of its pre-pass), `steps` calls each"""
    nq, d = Qd.shape
    st = torch.cuda.current_stream()
    # (a switch of the row format makes the handle forget its per-shape decisions: one untimed call takes them again)
    H.search_batch_device(hg, Qd.data_ptr(), nq, d, ef, K, ids_t.data_ptr(), dist_t.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    hg.set_option("time_kernels", 1)
    hg.kernel_times()
    calls, kern, pre = [], [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        H.search_batch_device(hg, Qd.data_ptr(), nq, d, ef, K, ids_t.data_ptr(), dist_t.data_ptr(), stream=st.cuda_stream)
        b.record(st)
        torch.cuda.synchronize()
        calls.append(a.elapsed_time(b))
        k_ms, p_ms, _ = hg.kernel_times()
        kern.append(k_ms)
        pre.append(p_ms)
    hg.set_option("time_kernels", 0)
    return calls, kern, pre


def run(d, n, nq, rounds, steps, query_bits=False):
    X, Q = R.clustered_unit(n, d, 1), R.clustered_unit(nq, d, 2)
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, 16, 200, seed=1, metric=H.METRIC_IP)
    print("clustered unit vectors: n %d, d %d, inner product, M 16, efC 200, k %d, %d queries; build %.1f s; device_bytes %.3f GB"
          % (n, d, K, nq, time.time() - t0, hg.info().device_bytes / 1e9), flush=True)
    Qd = torch.from_numpy(Q).to(R.DEV)
    ids_t = torch.empty((nq, K), dtype=torch.int32, device=R.DEV)
    dist_t = torch.empty((nq, K), dtype=torch.float32, device=R.DEV)
    gt = H.Ohnsw.brute_force_knn(hg, K, Q[:1000])[0]
    formats, refines = (QUERY_BITS_FORMATS, (4 * K, -1)) if query_bits else (FORMATS, (0, 4 * K, -1))
    configs = [(f, ef, r) for ef in (128, 256, 512) for f in formats for r in ((0,) if f[1] is None else refines)]
    acc = {c: ([], [], []) for c in configs}
    rec, row_bytes = {}, {}
    for rnd in range(rounds + 1):                    # round 0 warms every configuration and takes its recall: not timed
        for cfg in configs:
            (name, option, value, qbits), ef, refine = cfg
            switch(hg, option, value, qbits)
            hg.set_option("refine", refine)
            if rnd == 0:
                ids = H.Ohnsw.knn_batch_bigarray(hg, K, Q[:1000], ef=ef)[0]
                rec[cfg], row_bytes[cfg] = R.recall(ids, gt, K), hg.row_bytes()
                timed(hg, Qd, ef, ids_t, dist_t, 1)
                continue
            for into, got in zip(acc[cfg], timed(hg, Qd, ef, ids_t, dist_t, steps)):
                into.extend(got)
    base = {}
    for cfg in configs:
        (name, option, value, qbits), ef, refine = cfg
        calls, kern, pre = (np.array(a) for a in acc[cfg])
        if option is None:
            base[ef] = (np.median(calls), np.median(kern))
        c = 0 if option is None else ef if refine < 0 else min(ef, max(K, refine))
        print("  ef %3d %-9s rows (%4d B/row) refine %3d (%3d re-ranked): call %7.3f ms (%.3f .. %.3f; %.2fx float32), launches %7.3f ms "
              "(%.3f .. %.3f; %.2fx float32), pre-pass %.3f ms, recall@%d %.4f"
              % (ef, name, row_bytes[cfg], refine, c, np.median(calls), calls.min(), calls.max(), base[ef][0] / np.median(calls),
                 np.median(kern), kern.min(), kern.max(), base[ef][1] / np.median(kern), np.median(pre), K, rec[cfg]), flush=True)
    switch(hg, None, 0)
    hg.set_option("refine", 0)
    hg.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="1024,512")
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--query-bits", action="store_true", help="the leg of option bit_query_bits: the bit rows against a 1-bit and a 4-bit query")
    a = ap.parse_args()
    H.load()
    for d in (int(x) for x in a.dims.split(",")):
        run(d, a.n, a.nq, a.rounds, a.steps, a.query_bits)


if __name__ == "__main__":
    main()
