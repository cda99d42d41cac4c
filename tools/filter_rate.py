#!/usr/bin/env python3
"""What filtered search (hnsw_search_batch_filtered) costs: the C2 shape (1 M x 128 SIFT-like integers, L2, M 16, efC 200, ef 128,
k 10), 10 k queries, a uniform random allow-mask of selectivity 1.0 / 0.5 / 0.1 / 0.01 / 0.001.  Per selectivity: queries/s through
the host call (pageable matrices, host clock, median of --steps calls after a warm call), the share of queries served per stage
(0, 1, ... = how often W doubled; exact = the masked scan), and recall@10 of the first --recall-queries queries against the
exact scan over the allowed vectors alone (a flat index of X[mask]: the same order, ids mapped back).  Beside them the unfiltered
hnsw_search_batch rate of the same handle.  Informational: nothing gates on it.  The table printed here is what
profiles/filtered_search.txt holds.

--tenants L[,L...]: the mixed batch of a multi-tenant caller instead.  Uniform random labels 0 .. L-1 over the nodes
(Hgraph.filters_by_label), a uniform random tenant per query.  Per L the time of the ONE hnsw_search_batch_filtered_each call over
all queries against the loop of single-filter calls over each tenant's queries (sorted by tenant before the clock starts), the two
alternating in one run, medians of --steps repetitions (20 at least) after a warm round of both, and the stage histogram.  The rows
of the two are compared once (they are the same bits).  --loop-only times the loop alone, with per-tenant masks built on the host:
what a build without the per-query call offers.

--collect: option "filter_collect" (the answer from every node the walk evaluates, not from the final W only) against the ladder
over W, on one handle in one run: per selectivity ms per batch, the share of queries per stage and recall@10 against the exact
scan under the mask (brute_force_knn over the allowed vectors), with the option off and on; then the plain hnsw_search_batch of a
MARKED index (0.1 % and 10 % of the nodes marked deleted: what tools/soft_delete_rate.py times) both ways.  The table printed
here is what profiles/filter_collect.txt holds.
Usage: python tools/filter_rate.py [--n 1000000] [--nq 10000] [--steps 5] [--tenants 1,10,100,1000] [--collect] [--out profiles/filtered_search.txt]"""
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


def median_ms(fn, steps):
    fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def stage_shares(stage, nq):
    values, counts = np.unique(stage, return_counts=True)
    return ", ".join("%s %.1f %%" % ("exact" if v == H.STAGE_EXACT else "stage %d" % v, 100.0 * c / nq) for v, c in zip(values, counts))


def tenants(hg, Q, n, ef, k, counts, steps, loop_only, say):
    nq = len(Q)
    steps = max(steps, 20)
    for L in counts:
        labels = np.random.default_rng(1000 + L).integers(0, L, n)
        which = np.random.default_rng(2000 + L).integers(0, L, nq).astype(np.int32)
        t0 = time.perf_counter()
        filters = [hg.filter(labels == t) for t in range(L)] if loop_only else hg.filters_by_label(labels, L)
        made = (time.perf_counter() - t0) * 1e3
        groups = [np.flatnonzero(which == t) for t in range(L)]
        groups = [(t, g, np.ascontiguousarray(Q[g])) for t, g in enumerate(groups) if len(g)]

        def loop(counters=False):
            return [H.Ohnsw.knn_batch_filtered(hg, k, Qt, filters[t], ef=ef, counters=counters) for t, _, Qt in groups]

        def one(counters=False):
            return H.Ohnsw.knn_batch_filtered_each(hg, k, Q, filters, which, ef=ef, counters=counters)

        parts = loop(True)
        stage = np.zeros(nq, np.uint32)
        for (t, g, _), r in zip(groups, parts):
            stage[g] = r[4]
        same = ""
        if not loop_only:
            whole = one(True)
            ok = all(np.array_equal(whole[j][g].view(np.uint32), r[j].view(np.uint32)) for (t, g, _), r in zip(groups, parts) for j in range(5))
            same = "; rows of the two %s" % ("equal" if ok else "DIFFER")
        t_loop, t_one = [], []
        for _ in range(steps):          # alternating: drift of the machine lands on both
            t0 = time.perf_counter()
            loop()
            t_loop.append((time.perf_counter() - t0) * 1e3)
            if not loop_only:
                t0 = time.perf_counter()
                one()
                t_one.append((time.perf_counter() - t0) * 1e3)
        ml = float(np.median(t_loop))
        line = "tenants %-4d (%d in use, filters made in %.1f ms): loop of single-filter calls %9.3f ms (min %.3f), %7.3f M q/s" % (
            L, len(groups), made, ml, min(t_loop), nq / ml / 1e3)
        if not loop_only:
            mo = float(np.median(t_one))
            line += "; ONE per-query call %9.3f ms (min %.3f), %7.3f M q/s; loop / one call %.2fx" % (mo, min(t_one), nq / mo / 1e3, ml / mo)
        say(line + "; " + stage_shares(stage, nq) + same)
        for f in filters:
            f.release()


def recall_at_k(ids, X, mask, Q, k):
    """the share of the exact masked k nearest (a flat index of X[mask]: the same order, ids mapped back) found in ids"""
    allowed = np.flatnonzero(mask)
    sub = H.Hgraph.flat(X[mask])
    truth = allowed[H.Ohnsw.brute_force_knn(sub, k, Q)[0]]
    sub.release()
    return float(np.mean([len(set(x) & set(y)) for x, y in zip(ids, truth)])) / k


def collect(hg, X, Q, ef, k, steps, nr, say):
    n, nq = len(X), len(Q)
    say('option "filter_collect" off / on, the same handle, the two timed one after the other per line; recall@%d of the first %d queries '
        "against the exact scan under the mask" % (k, nr))

    def both(call, mask, what):
        for v in (0, 1):
            hg.set_option("filter_collect", v)
            ms = median_ms(lambda: call(False), steps)
            ids, _, _, _, stage = call(True)
            say("%s, filter_collect %d: %9.3f ms per batch, %7.3f M q/s; %s; recall@%d %.4f"
                % (what, v, ms, nq / ms / 1e3, stage_shares(stage, nq), k, recall_at_k(ids[:nr], X, mask, Q[:nr], k)))
        hg.set_option("filter_collect", 0)

    for sel in (1.0, 0.5, 0.1, 0.01, 0.001):
        mask = np.ones(n, bool) if sel >= 1.0 else np.random.default_rng(int(sel * 1e6)).random(n) < sel
        flt = hg.filter(mask)
        both(lambda counters: H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef, counters=counters), mask,
             "selectivity %-5g (%7d allowed)" % (sel, flt.count()))
        flt.release()
    # the plain call of a marked index (it answers under the live mask): the stages come from the filtered call under that mask,
    # which the plain call is bit for bit
    order = np.random.default_rng(11).permutation(n)
    marked = 0
    for share in (0.001, 0.1):
        m = int(round(share * n))
        hg.mark_deleted(order[marked:m])
        marked = m
        live = ~hg.deleted_mask()

        def call(counters):
            if not counters:
                return H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
            return H.Ohnsw.knn_batch_filtered(hg, k, Q, live, ef=ef, counters=True)
        both(call, live, "marked %-5g %% (%7d nodes), hnsw_search_batch" % (100 * share, m))
    hg.unmark_deleted(order[:marked])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--tenants", default=None, help="comma-separated tenant counts: time the mixed batch instead of the selectivity table")
    ap.add_argument("--loop-only", action="store_true", help="with --tenants: the loop of single-filter calls alone")
    ap.add_argument("--collect", action="store_true", help='option "filter_collect" off and on: rate, stages and recall per selectivity, and the marked index')
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.device_count() < 1:
        raise SystemExit("filter_rate: no HIP device (there is no CPU path to time)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    d, M, efc, ef, k = 128, 16, 200, 128, 10
    rng = np.random.default_rng(7)
    centres = rng.integers(20, 200, size=(256, d))
    X = np.clip(np.rint(centres[rng.integers(0, 256, a.n)] + rng.normal(0, 25, size=(a.n, d))), 0, 218).astype(np.float32)
    Q = np.clip(np.rint(centres[rng.integers(0, 256, a.nq)] + rng.normal(0, 25, size=(a.nq, d))), 0, 218).astype(np.float32)
    t0 = time.time()
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=1, expected_ef=ef)
    say("hnsw_search_batch_filtered: C2 shape, n %d, d %d, L2, M %d, efC %d, ef %d, k %d, %d queries; build %.1f s; rows: %d B"
        % (a.n, d, M, efc, ef, k, a.nq, time.time() - t0, hg.row_bytes()))
    plain = median_ms(lambda: H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef), a.steps)
    say("unfiltered hnsw_search_batch: %.3f ms per batch, %.3f M q/s" % (plain, a.nq / plain / 1e3))
    nr = min(a.recall_queries, a.nq)
    if a.tenants:
        say("mixed batch of %d queries, uniform random labels over the nodes, a uniform random tenant per query; medians of %d alternating repetitions"
            % (a.nq, max(a.steps, 20)))
        tenants(hg, Q, a.n, ef, k, [int(x) for x in a.tenants.split(",")], a.steps, a.loop_only, say)
    if a.collect:
        collect(hg, X, Q, ef, k, a.steps, nr, say)
    for sel in (() if a.tenants or a.collect else (1.0, 0.5, 0.1, 0.01, 0.001)):
        mask = np.ones(a.n, bool) if sel >= 1.0 else np.random.default_rng(int(sel * 1e6)).random(a.n) < sel
        flt = hg.filter(mask)
        ms = median_ms(lambda: H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef), a.steps)
        ids, _, _, _, stage = H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef, counters=True)
        allowed = np.flatnonzero(mask)
        sub = H.Hgraph.flat(X[mask])
        truth = allowed[H.Ohnsw.brute_force_knn(sub, k, Q[:nr])[0]]
        sub.release()
        hits = np.mean([len(set(x) & set(y)) for x, y in zip(ids[:nr], truth)]) / k
        shares = stage_shares(stage, a.nq)
        say("selectivity %-5g (%7d allowed): %8.3f ms per batch, %7.3f M q/s (%.2fx the unfiltered call); %s; recall@%d %.4f"
            % (sel, flt.count(), ms, a.nq / ms / 1e3, plain / ms, shares, k, hits))
        flt.release()
    hg.release()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
