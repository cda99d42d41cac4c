"""Option "scan_matrix" (ocaml-hnsw_amd/csrc/hnsw_scan_matrix.hip): the exact scan screened by fp32 matrix instructions returns
the ids and the distance BITS of the float scan and, on data whose sums are exact in fp32, of a numpy float64 reference; what it
may not serve runs what ran before, and Hgraph.scan_path() tells which.  All comparisons are equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALLOWED = [0, 31, 32, 258, 259, 484, 516]       # 7 < k, both sides of a mask word's edge, first and last row
N, NQ = 517, 33         # n: no multiple of the 32-row block; nq: one full tile of 32 queries plus one
FLOAT, BYTES, MATRIX = 1, 2, 3      # scan_path()


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _data(kind, d, seed=0):
    rng = np.random.default_rng(1000 * d + seed)
    if kind == "exact":         # integers in -8..8 times 2^-3: every sum of the chain is a multiple of 2^-6 below 2^24 of them, exact in fp32
        X, Q = (rng.integers(-8, 9, size=(N, d)) / 8.0).astype(np.float32), (rng.integers(-8, 9, size=(NQ, d)) / 8.0).astype(np.float32)
        X[5], Q[3] = 0, 0
        X[[77, 300, 516]] = X[12]               # three exact duplicates of one row: ties break by id
        Q[7] = X[12]                            # ... one of them also a query: a zero distance
        return X, Q
    X, Q = rng.standard_normal((N, d), dtype=np.float32), rng.standard_normal((NQ, d), dtype=np.float32)
    if kind == "shifted":       # norms far above the distances: nearly every pair survives the screen
        X, Q = X + np.float32(1000), Q + np.float32(1000)
    if kind == "extreme":       # a norm that overflows to +inf from finite values; squares that underflow
        X[40], X[41] = X[40] * np.float32(1e20), X[41] * np.float32(1e-25)
    return X, Q


def _reference(X, Q, metric, k):
    x, q = X.astype(np.float64), Q.astype(np.float64)
    s = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2) if metric == 0 else q @ x.T
    dist = np.sqrt(s).astype(np.float32) if metric == 0 else np.float32(1) - s.astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(N), s.shape), s if metric == 0 else -s), axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(dist, order, 1)


def _scan(H, hg, on, k, Q):
    hg.set_option("scan_matrix", on)
    ids, dist = H.Ohnsw.brute_force_knn(hg, k, Q)
    return ids, dist.view(np.uint32), hg.scan_path()


@pytest.mark.parametrize("kind", ["gauss", "shifted", "exact", "extreme"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 128, 260, 512])     # a row nearly all padding; ragged and full rows of 128 floats; 3 and 4 pipeline stages of 128
def test_matrix_scan_returns_the_float_scans_bits(H, d, metric, kind):
    X, Q = _data(kind, d)
    hg = H.Hgraph.flat(X, metric=metric)
    for slabs in (1, 3):
        hg.set_option("scan_slabs", slabs)
        for k in (1, 10, N):
            c = "%s d %d metric %d slabs %d k %d" % (kind, d, metric, slabs, k)
            ids1, bits1, path1 = _scan(H, hg, 1, k, Q)
            ids0, bits0, path0 = _scan(H, hg, 0, k, Q)
            assert (path1, path0) == (MATRIX, FLOAT), c
            np.testing.assert_array_equal(ids1, ids0, err_msg=c + " ids, on against off")
            np.testing.assert_array_equal(bits1, bits0, err_msg=c + " distance bits, on against off")
            if kind == "exact":
                rids, rdist = _reference(X, Q, metric, k)
                np.testing.assert_array_equal(ids1, rids, err_msg=c + " ids against float64")
                np.testing.assert_array_equal(bits1, rdist.view(np.uint32), err_msg=c + " distance bits against float64")
    hg.release()


@pytest.mark.parametrize("metric, slabs", [pytest.param(0, None, id="0"), pytest.param(1, None, id="1"),    # the plan's own slabs
                                           # three slabs: the edges at rows 173 and 346 fall inside mask words 5 and 10
                                           pytest.param(0, 3, id="0-slabs3"), pytest.param(1, 3, id="1-slabs3")])
def test_masked_matrix_scan(H, metric, slabs):
    X, Q = _data("gauss", 100, seed=1)
    hg = H.Hgraph.flat(X, metric=metric)
    if slabs:
        hg.set_option("scan_slabs", slabs)
    mask = np.isin(np.arange(N), ALLOWED)   # 7 allowed nodes < k: the filtered search goes straight to the exact stage
    out = {}
    for on in (1, 0):
        hg.set_option("scan_matrix", on)
        ids, dist = H.Ohnsw.knn_batch_filtered(hg, 10, Q, mask, ef=16)
        out[on] = (ids, dist.view(np.uint32), hg.scan_path())
    assert (out[1][2], out[0][2]) == (MATRIX, FLOAT)
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(out[1][1], out[0][1])
    assert sorted(out[1][0][0, :7]) == ALLOWED and (out[1][0][:, 7:] == -1).all()
    hg.release()


@pytest.mark.parametrize("case", ["query nan", "query inf", "d 516", "byte rows"])
def test_fallbacks_keep_what_ran_before(H, case):
    X, Q = _data("gauss", 516 if case == "d 516" else 100, seed=2)
    if case.startswith("query"):
        Q[NQ - 2, 17] = float(case.split()[1])      # one value of one query of the batch
    byte = case == "byte rows"                      # a handle the byte scan takes: it has precedence
    if byte:
        X, Q = np.rint(X * 40 + 128).clip(0, 255), np.rint(Q * 40 + 128).clip(0, 255)
    hg = H.Hgraph.flat(X)
    hg.set_option("scan_bytes", int(byte))
    want = BYTES if byte else FLOAT
    for v in (2, -1):                               # the option is a switch: anything but 0 / 1 is refused
        with pytest.raises(Exception):
            hg.set_option("scan_matrix", v)
    ids1, bits1, path1 = _scan(H, hg, 1, 10, Q)
    ids0, bits0, path0 = _scan(H, hg, 0, 10, Q)
    assert (path1, path0) == (want, want), case
    np.testing.assert_array_equal(ids1, ids0)
    np.testing.assert_array_equal(bits1, bits0)
    hg.release()

