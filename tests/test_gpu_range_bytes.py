"""Option "scan_bytes" 2 on the exact range scan (ocaml-hnsw_amd/csrc/hnsw_range_bytes.hip): the lims, ids and distance BITS of the
float range scan and of a numpy int64 reference (every sum is an integer below 2^24); what it may not serve runs the float range
kernels, and Hgraph.scan_path() tells which ran.  All comparisons are equality; every radius comes from the reference."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALLOWED = [0, 31, 32, 258, 259, 484, 516]       # both sides of a mask word's edge, first and last row
N, NQ = 517, 33         # n: no multiple of the 32-row block; nq: one full tile of 32 queries plus one
FLOAT, BYTES = 1, 2     # scan_path()
DUPLICATES = [12, 77, 300, 516]


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


@functools.lru_cache(maxsize=None)
def _case(d, metric=0, seed=0, n=N):
    """X, Q, the float32 distances [nq][n] made from int64 sums, each query's rows in the order (sum, id); shared: never written to"""
    rng = np.random.default_rng(1000 * d + seed)
    X, Q = rng.integers(0, 256, size=(n, d)).astype(np.float32), rng.integers(0, 256, size=(NQ, d)).astype(np.float32)
    X[5], X[40] = 0, 255
    X[DUPLICATES[1:]] = X[DUPLICATES[0]]    # three exact duplicates of one row: ties break by id
    Q[0], Q[NQ - 1] = 0, 255                # against X[40] / X[5] at d 256: 256 * 255^2 = 16 646 400 < 2^24
    Q[7] = X[DUPLICATES[0]]                 # ... one of them also a query: a zero distance
    x, q = X.astype(np.int64), Q.astype(np.int64)
    s = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2) if metric == 0 else q @ x.T
    dist = np.sqrt(s.astype(np.float64)).astype(np.float32) if metric == 0 else np.float32(1) - s.astype(np.float32)
    return X, Q, dist, np.lexsort((np.broadcast_to(np.arange(n), s.shape), s if metric == 0 else -s), axis=1)


def _on_off(hg, paths, c, call, values=(2, 0)):
    """call() under the two values of the option -> the first result; both as (lims, ids, ..., path), equal in every bit, paths as given"""
    out = []
    for v in values:
        hg.set_option("scan_bytes", v)
        out.append(tuple(a.view(np.uint32) if a.dtype == np.float32 else a for a in call()) + (hg.scan_path(),))
    assert (out[0][-1], out[1][-1]) == paths, c
    for x, y in zip(out[0][:-1], out[1][:-1]):
        np.testing.assert_array_equal(x, y, err_msg=c + ", option %d against %d" % values)
    return out[0]


@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 128, 200, 256])     # 64-byte rows nearly all padding; ragged and full 128- and 256-byte rows
def test_byte_range_scan_returns_the_float_range_scans_bits(H, d, metric, slabs):
    X, Q, dist, order = _case(d, metric)
    r_hit = np.sort(dist[0])[9]                             # attained exactly: a pair on the interval's edge
    hg = H.Hgraph.flat(X, metric=metric)
    hg.set_option("scan_slabs", slabs)
    for r in [r_hit, np.nextafter(r_hit, np.float32(-np.inf)), np.float32(1e30)] + ([np.float32(0)] if metric == 0 else []):
        c = "d %d metric %d slabs %d radius %r" % (d, metric, slabs, r)
        lims, ids, bits, _ = _on_off(hg, (BYTES, FLOAT), c, lambda: H.Ohnsw.brute_force_range(hg, float(r), Q))
        want = [o[dist[q][o] <= r] for q, o in enumerate(order)]
        assert r != np.float32(1e30) or all(len(w) == N for w in want), c      # every count is N, every PASS-1 guard is exercised
        np.testing.assert_array_equal(np.diff(lims), [len(w) for w in want], err_msg=c + " lengths against int64")
        np.testing.assert_array_equal(ids, np.concatenate(want), err_msg=c + " ids against int64")
        np.testing.assert_array_equal(bits, np.concatenate([dist[q][w] for q, w in enumerate(want)]).view(np.uint32), err_msg=c)
        if r == 0:                                          # the query equal to a stored row: its zero-distance duplicates, in id order
            assert ids[lims[7]:lims[8]].tolist() == DUPLICATES, c
    hg.release()


@pytest.mark.parametrize("metric, slabs", [pytest.param(0, None, id="0"), pytest.param(1, None, id="1"),    # the plan's own slabs
                                           # three slabs: the edges at rows 173 and 346 fall inside mask words 5 and 10
                                           pytest.param(0, 3, id="0-slabs3"), pytest.param(1, 3, id="1-slabs3")])
def test_masked_byte_range_scan(H, metric, slabs):
    X, Q = _case(100, seed=1)[:2]
    hg = H.Hgraph.flat(X, metric=metric)
    if slabs:
        hg.set_option("scan_slabs", slabs)
    mask = np.isin(np.arange(N), ALLOWED)
    for how in ("filter", "marks"):                         # the call's allow-mask, then the same rows through the handle's live mask
        if how == "marks":
            hg.mark_deleted(np.flatnonzero(~mask))
        lims, ids, _, _ = _on_off(hg, (BYTES, FLOAT), how, lambda: H.Ohnsw.brute_force_range(hg, 1e30, Q, filter=mask if how == "filter" else None))
        assert all(sorted(ids[lims[q]:lims[q + 1]]) == ALLOWED for q in range(NQ)), how
    hg.release()


def test_ladder_exact_stage(H):
    X, Q = (a.copy() for a in _case(20, seed=3, n=2003)[:2])
    Q[::2] = np.rint(128 + (Q[::2] - 128) / 16)             # queries near the centre of the cube: most of the table within the radius
    Q[1::2] = np.rint(Q[1::2] / 255) * 255                  # queries in its corners: hardly any of it
    dist = np.sqrt(((Q[:, None, :].astype(np.int64) - X[None].astype(np.int64)) ** 2).sum(2).astype(np.float64)).astype(np.float32)
    radius = float(np.quantile(dist, 0.5))
    hits = (dist <= np.float32(radius)).sum(1)
    # a query with fewer than 1024 hits is never saturated at 1024; W_1024 of one with three quarters of the table in range is all in range
    many, few = hits >= 1500, hits < 1000
    assert many.any() and few.any() and (many | few).all(), hits
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    stage = _on_off(hg, (BYTES, FLOAT), "ladder", lambda: H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True))[5]
    assert (stage[many] == H.STAGE_EXACT).all() and (stage[few] != H.STAGE_EXACT).all()
    hg.release()


@pytest.mark.parametrize("case", ["query 0.5", "query 256", "query -1", "float data", "d 300", "the switch"])
def test_fallbacks_and_the_switch(H, case):
    X, Q = (a.copy() for a in _case(300 if case == "d 300" else 100, seed=2)[:2])
    if case.startswith("query"):
        Q[NQ - 2, 17] = float(case.split()[1])              # one value of one query of the batch
    if case == "float data":
        X[100, 3] = 0.5
    radius = float(np.sort(np.sqrt(((Q[0].astype(np.float64) - X) ** 2).sum(1)))[9]) + 1.0
    hg = H.Hgraph.flat(X)
    if case != "the switch":                                # under 2 as under 0: the float range kernels and their results
        assert _on_off(hg, (FLOAT, FLOAT), case, lambda: H.Ohnsw.brute_force_range(hg, radius, Q))[0][-1] >= 10
    else:                                                   # 2 is everything 1 is: the k-scan takes the byte kernels, same ids and bits
        _on_off(hg, (BYTES, BYTES), "k-scan", lambda: H.Ohnsw.brute_force_knn(hg, 10, Q), values=(2, 1))
        hg.set_option("scan_bytes", 2)
        for v in (3, -1):                                   # refused, and the value set before still holds
            with pytest.raises(H.InvalidArgument):
                hg.set_option("scan_bytes", v)
            assert H.Ohnsw.brute_force_range(hg, radius, Q)[0][-1] >= 10 and hg.scan_path() == BYTES, v
    hg.release()
