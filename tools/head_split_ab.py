#!/usr/bin/env python3
"""Option "head_queries" measured on bench.py's headline workload (GPU box).

    python tools/head_split_ab.py sweep [nq:H/H/... ...]      one process, one index: per batch size the synchronous host call
                                                            (page-locked matrices, eight rotating batches) at each H, the
                                                            settings alternated round by round; H = -1 is the automatic rule
    python tools/head_split_ab.py bench PARENT.so [RUNS]    plain `bench.py --gpus 1 --steps 20 --warmup 5` runs, the parent's
                                                            library and the tree's alternated (HNSW_LIB_PATH), RUNS (5) each

A setting may carry environment words behind its H, as in 4000@HNSW_PRIO=750,4192 (read by the library at every call).
Prints mean / median / min / max of the call in ms and whether ids and distance bits equal those of H = 0."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    import numpy as np
    ts = np.asarray(ts, dtype=np.float64)
    return "mean %.4f  median %.4f  min %.4f  max %.4f" % (ts.mean(), np.median(ts), ts.min(), ts.max())


def sweep(specs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import ocaml_hnsw_amd as H
    from bench import make_sift_like
    dev = torch.device("cuda", 0)
    n, d, k, ef, NB, rounds = 1_000_000, 128, 10, 128, 8, int(os.environ.get("ROUNDS", 6))
    hg = H.Ohnsw.build_batch_bigarray(make_sift_like(n, d, 1, dev).cpu().numpy(), 16, 200, seed=1)
    for spec in specs or ["10000:0/64/1808/3000/4000/5000/-1"]:
        nq, heads = spec.split(":")
        nq = int(nq)
        settings = []
        for h in heads.split("/"):
            h, _, env = h.partition("@")
            settings.append((int(h), dict(w.split("=", 1) for w in env.split("@")) if env else {}))
        Qs = []
        for b in range(NB):
            q = H.host_empty((nq, d), np.float32)
            q[:] = make_sift_like(nq, d, 2 + b, dev).cpu().numpy()
            Qs.append(q)
        oi, od = H.host_empty((nq, k), np.int32), H.host_empty((nq, k), np.float32)
        times = [[] for _ in settings]
        same = [True] * len(settings)
        ref = None
        for r in range(rounds + 1):                                   # round 0: the results compared, nothing timed
            for s, (h, env) in enumerate(settings):
                hg.set_option("head_queries", h)
                os.environ.update(env)
                for b in range(NB):
                    t0 = time.perf_counter()
                    H.Ohnsw.knn_batch_bigarray(hg, k, Qs[b], ef=ef, out=(oi, od))
                    t1 = time.perf_counter()
                    if r:
                        times[s].append(1e3 * (t1 - t0))
                    elif b == 0:
                        got = (oi.copy(), od.view(np.uint32).copy())
                        ref = ref or got
                        same[s] = np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
                for w in env:
                    del os.environ[w]
        base = np.mean(times[0])
        for s, (h, env) in enumerate(settings):
            print("nq %6d  H %6d %-28s %s  (%+.1f %% against the first)  same results: %s" %
                  (nq, h, " ".join("%s=%s" % e for e in env.items()), stats(times[s]), 100 * (np.mean(times[s]) / base - 1), same[s]), flush=True)
    hg.release()


def bench(parent, runs):
    libs = [("parent", os.path.abspath(parent)), ("new", os.path.join(ROOT, "ocaml-hnsw_amd", "libhnsw_mi355x.so"))]
    ms = {name: [] for name, _ in libs}
    for r in range(runs):
        for name, lib in libs:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                                 env=dict(os.environ, HNSW_LIB_PATH=lib), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
            if out.returncode != 0:
                print("run %d %s FAILED rc=%d" % (r, name, out.returncode), flush=True)
                sys.exit(1)                                           # a failing variant: start no further GPU work
            line = json.loads(out.stdout.decode().strip().splitlines()[-1])
            ms[name].append(line["ms_per_step"])
            print("run %d %-6s ms_per_step %.4f  value %.0f" % (r, name, line["ms_per_step"], line["value"]), flush=True)
    for name, _ in libs:
        print("%-6s %s  spread %.4f" % (name, stats(ms[name]), max(ms[name]) - min(ms[name])), flush=True)
    import numpy as np
    gain = np.mean(ms["parent"]) - np.mean(ms["new"])
    print("new is %.4f ms (%.1f %%) below the parent; the bar, three times the parent's spread: %.4f ms" %
          (gain, 100 * gain / np.mean(ms["parent"]), 3 * (max(ms["parent"]) - min(ms["parent"]))), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "bench":
        bench(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        sweep(sys.argv[2:])
