#!/usr/bin/env python3
"""What an upsert costs against the two calls it replaces: the C2 shape (1 M x 128 SIFT-like integers = byte rows, L2, M 16, efC 200),
upserts of 1000 keys, half of them stored and half new.  Two twin handles are built with the same seed and given the same keys; in
every round handle A gets hnsw_index_upsert_keyed and handle B gets hnsw_index_remove_keys of the stored half followed by
hnsw_index_insert_keyed of all 1000, the two alternating and taking turns to go first, so both see the same index in the same state (afterwards their keys are
compared).  Once with the handles as built and once with option sq8_rows on (byte_rows 0 first: the data is byte-valued), where each table swap quantises the whole table again.
Host clock around the synchronous calls, medians of --steps rounds after a warm round.  Device memory: a second thread samples
hipMemGetInfo while the call runs (the call releases the interpreter lock); the figure is the largest amount in use above the level
before the call, so it is a lower bound of the true peak at the sampling interval.  Informational: nothing gates on it.  The table
printed here is what profiles/upsert.txt holds.
Usage: python tools/upsert_rate.py [--n 1000000] [--m 1000] [--steps 6] [--out profiles/upsert.txt]"""
import argparse
import ctypes
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:   # one HIP runtime per process: torch's bundled copy first, if there is one
    import torch  # noqa: F401
except ImportError:
    pass
import ocaml_hnsw_amd as H  # noqa: E402


def hip_runtime():
    """the HIP runtime this process has loaded already (never a second one)"""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64" in os.path.basename(path):
                return ctypes.CDLL(path)
    raise SystemExit("upsert_rate: no HIP runtime loaded")


class MemoryPeak:
    """bytes in use on the current device above the level at the start, sampled by a thread of its own"""

    def __init__(self, hip):
        self.hip, self.stop, self.peak = hip, False, 0
        self.base = self.used()

    def used(self):
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if self.hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
            return 0
        return total.value - free.value

    def run(self):
        while not self.stop:
            self.peak = max(self.peak, self.used() - self.base)
            time.sleep(0.0001)

    def __enter__(self):
        self.thread = threading.Thread(target=self.run)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()


def timed(hip, call):
    with MemoryPeak(hip) as mp:
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
    return ms, mp.peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("upsert_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc = 128, 16, 200
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))

    def draw(count):
        return np.clip(np.rint(centres[rng.integers(0, 256, count)] + rng.normal(0, 25, size=(count, d))), 0, 218).astype(np.float32)

    X = draw(a.n)
    keys0 = rng.permutation(a.n).astype(np.int64) * 7919 - (a.n * 7919) // 2          # distinct, both signs, in no order
    say("upsert: C2 shape, n %d, d %d, L2, M %d, efC %d; calls of %d keys, half stored and half new; medians of %d rounds after a warm round"
        % (a.n, d, M, efc, a.m, a.steps))
    hip = None
    for sq8 in (0, 1):
        t0 = time.time()
        A = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1)
        B = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1)
        hip = hip or hip_runtime()
        for hg in (A, B):
            hg.set_keys(keys0)
            if sq8:
                hg.set_option("byte_rows", 0)                   # (byte-valued data: the exact byte rows stand in front of the codes)
                hg.set_option("sq8_rows", 1)
        say("sq8_rows %d: two twins built in %.1f s; rows: %d B; index: %.0f MB of device memory each"
            % (sq8, time.time() - t0, A.row_bytes(), A.info().device_bytes / 1e6))
        stored = keys0.copy()
        next_key = int(keys0.max()) + 1
        one, rem, ins, peak_one, peak_two = [], [], [], [], []
        for r in range(a.steps + 1):
            half = a.m // 2
            old = stored[rng.choice(len(stored), size=half, replace=False)]
            new = np.arange(next_key, next_key + a.m - half, dtype=np.int64)
            next_key += a.m - half
            call_keys = np.concatenate([old, new])[rng.permutation(a.m)]
            V = draw(a.m)
            gone = call_keys[np.isin(call_keys, old)]
            if r % 2:       # whoever goes first follows the host's work of this round on an idle device: take turns
                t_one, p_one = timed(hip, lambda: H.Ohnsw.upsert_batch_keyed(A, V, call_keys, M, efc, seed=1))
            t_rem, p_rem = timed(hip, lambda: B.remove_keys(gone))
            t_ins, p_ins = timed(hip, lambda: H.Ohnsw.insert_batch_keyed(B, V, call_keys, M, efc, seed=1))
            if not r % 2:
                t_one, p_one = timed(hip, lambda: H.Ohnsw.upsert_batch_keyed(A, V, call_keys, M, efc, seed=1))
            stored = np.concatenate([stored[~np.isin(stored, old)], call_keys])
            if r:
                one.append(t_one), rem.append(t_rem), ins.append(t_ins), peak_one.append(p_one), peak_two.append(max(p_rem, p_ins))
        same = np.array_equal(A.keys(), B.keys()) and A.info().n == B.info().n
        two = [x + y for x, y in zip(rem, ins)]
        say("  hnsw_index_upsert_keyed                           %8.1f ms per call (min %.1f, max %.1f); sampled peak above the index: %.0f MB"
            % (float(np.median(one)), min(one), max(one), max(peak_one) / 1e6))
        say("  hnsw_index_remove_keys + hnsw_index_insert_keyed  %8.1f ms per pair (min %.1f, max %.1f; remove %.1f + insert %.1f); sampled peak: %.0f MB"
            % (float(np.median(two)), min(two), max(two), float(np.median(rem)), float(np.median(ins)), max(peak_two) / 1e6))
        say("  one call / two calls: %.3fx; n afterwards %d; the twins' keys afterwards are equal: %s"
            % (float(np.median(one)) / float(np.median(two)), A.info().n, "yes" if same else "NO"))
        A.release()
        B.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
