"""Option "scan_matrix" on the exact range scan (ocaml-hnsw_amd/csrc/hnsw_range_matrix.hip): same lims, ids and distance BITS as the
float range scan and, on data whose sums are exact in fp32, as a numpy float64 reference; what it may not serve runs what ran before,
and Hgraph.scan_path() tells which.  All comparisons are equality; every radius comes from the float64 reference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALLOWED = [0, 31, 32, 258, 259, 484, 516]       # both sides of a mask word's edge, first and last row
N, NQ = 517, 33         # n: no multiple of the 32-row block; nq: one full tile of 32 queries plus one
FLOAT, MATRIX = 1, 3    # scan_path()
DUPLICATES = [12, 77, 300, 516]


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _data(kind, d, seed=0, n=N):
    rng = np.random.default_rng(1000 * d + seed)
    if kind == "exact":         # multiples of 1/8 in [-1, 1]: every sum is a multiple of 2^-6 below 2^11 at d <= 512, exact in fp32
        X, Q = (rng.integers(-8, 9, size=(n, d)) / 8.0).astype(np.float32), (rng.integers(-8, 9, size=(NQ, d)) / 8.0).astype(np.float32)
        X[5], Q[3] = 0, 0
        X[DUPLICATES[1:]] = X[DUPLICATES[0]]    # three exact duplicates of one row: ties break by id
        Q[7] = X[DUPLICATES[0]]                 # ... one of them also a query: a zero distance
        return X, Q
    X, Q = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((NQ, d), dtype=np.float32)
    if kind == "shifted":       # norms far above the distances: nearly every pair survives the screen
        X, Q = X + np.float32(1000), Q + np.float32(1000)
    if kind == "extreme":       # a norm that overflows to +inf from finite values; squares that underflow
        X[40], X[41] = X[40] * np.float32(1e20), X[41] * np.float32(1e-25)
    return X, Q


def _reference(X, Q, metric):
    """float64 sums s [nq][n] and the float32 distances made from them"""
    x, q = X.astype(np.float64), Q.astype(np.float64)
    with np.errstate(over="ignore"):
        s = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2) if metric == 0 else q @ x.T
        return s, (np.sqrt(s.astype(np.float32)) if metric == 0 else np.float32(1) - s.astype(np.float32))


def _on_off(H, hg, paths, c, call):
    """call() with the option on and off -> the on result; both as (lims, ids, ..., path), equal in every bit, paths as given"""
    out = []
    for on in (1, 0):
        hg.set_option("scan_matrix", on)
        out.append(tuple(a.view(np.uint32) if a.dtype == np.float32 else a for a in call()) + (hg.scan_path(),))
    assert (out[0][-1], out[1][-1]) == paths, c         # (on the parent of the matrix range scan a range call never set the path)
    for x, y in zip(out[0][:-1], out[1][:-1]):
        np.testing.assert_array_equal(x, y, err_msg=c + ", on against off")
    return out[0]


@pytest.mark.parametrize("kind", ["gauss", "shifted", "exact", "extreme"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 260, 512])      # a row nearly all padding; ragged rows of 128 floats; 3 and 4 pipeline stages of 128
def test_matrix_range_scan_returns_the_float_range_scans_bits(H, d, metric, kind):
    X, Q = _data(kind, d)
    s, dist = _reference(X, Q, metric)
    order = np.lexsort((np.broadcast_to(np.arange(N), s.shape), s if metric == 0 else -s), axis=1)
    r_hit = np.sort(dist[0])[9]                         # attained exactly on `exact`: a pair on the interval's edge
    radii = [r_hit, np.nextafter(r_hit, np.float32(-np.inf)), np.float32(1e30)] + ([np.float32(0)] if (kind, metric) == ("exact", 0) else [])
    hg = H.Hgraph.flat(X, metric=metric)
    for slabs in (1, 3):
        hg.set_option("scan_slabs", slabs)
        for r in radii:
            c = "%s d %d metric %d slabs %d radius %r" % (kind, d, metric, slabs, r)
            lims, ids, bits, _ = _on_off(H, hg, (MATRIX, FLOAT), c, lambda: H.Ohnsw.brute_force_range(hg, float(r), Q))
            if r == np.float32(1e30) and kind != "extreme":        # every buffer overflows many times in both passes
                assert (np.diff(lims) == N).all(), c
            if kind == "exact":
                want = [o[dist[q][o] <= r] for q, o in enumerate(order)]
                np.testing.assert_array_equal(np.diff(lims), [len(w) for w in want], err_msg=c + " lengths against float64")
                np.testing.assert_array_equal(ids, np.concatenate(want), err_msg=c + " ids against float64")
                np.testing.assert_array_equal(bits, np.concatenate([dist[q][w] for q, w in enumerate(want)]).view(np.uint32), err_msg=c)
                if r == 0:                              # the query equal to a stored row: its zero-distance duplicates, in id order
                    seg = ids[lims[7]:lims[8]].tolist()
                    assert seg == sorted(seg) and set(DUPLICATES) <= set(seg), c
    hg.release()


@pytest.mark.parametrize("metric, slabs", [pytest.param(0, None, id="0"), pytest.param(1, None, id="1"),    # the plan's own slabs
                                           # three slabs: the edges at rows 173 and 346 fall inside mask words 5 and 10
                                           pytest.param(0, 3, id="0-slabs3"), pytest.param(1, 3, id="1-slabs3")])
def test_masked_matrix_range_scan(H, metric, slabs):
    X, Q = _data("gauss", 100, seed=1)
    hg = H.Hgraph.flat(X, metric=metric)
    if slabs:
        hg.set_option("scan_slabs", slabs)
    mask = np.isin(np.arange(N), ALLOWED)
    lims, ids, _, _ = _on_off(H, hg, (MATRIX, FLOAT), "masked", lambda: H.Ohnsw.brute_force_range(hg, 1e30, Q, filter=mask))
    assert all(sorted(ids[lims[q]:lims[q + 1]]) == ALLOWED for q in range(NQ))
    hg.release()


def test_ladder_exact_stage(H):
    X, Q = _data("gauss", 20, seed=3, n=2003)
    dist = _reference(X, Q, 0)[1]
    radius = float(np.quantile(dist, 0.6))
    hits = (dist <= np.float32(radius)).sum(1)
    # a query with fewer than 1024 hits is never saturated at 1024; W_1024 of one with three quarters of the table in range is all in
    # range (the margins: the device's fp32 sums may put a boundary pair on the other side)
    many, few = hits >= 1500, hits < 1000
    assert many.any() and few.any(), hits
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    stage = _on_off(H, hg, (MATRIX, FLOAT), "ladder", lambda: H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True))[5]
    assert (stage[many] == H.STAGE_EXACT).all() and (stage[few] != H.STAGE_EXACT).all()
    hg.release()


@pytest.mark.parametrize("case", ["query nan", "query inf", "d 516", "byte rows"])
def test_fallbacks_keep_the_float_range_scan(H, case):
    X, Q = _data("gauss", 516 if case == "d 516" else 100, seed=2)
    byte = case == "byte rows"                      # a handle the byte scan takes keeps the float range kernels
    if byte:
        X, Q = np.rint(X * 40 + 128).clip(0, 255), np.rint(Q * 40 + 128).clip(0, 255)
    radius = float(np.sort(_reference(X, Q, 0)[1][0])[9])
    if case.startswith("query"):
        Q[NQ - 2, 17] = float(case.split()[1])      # one value of one query of the batch
    hg = H.Hgraph.flat(X)
    hg.set_option("scan_bytes", int(byte))
    assert _on_off(H, hg, (FLOAT, FLOAT), case, lambda: H.Ohnsw.brute_force_range(hg, radius, Q))[0][-1] > 0
    hg.release()
