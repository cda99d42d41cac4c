"""Option "scan_bytes" (ocaml-hnsw_amd/csrc/hnsw_scan_bytes.hip): the exact scan of byte-valued data through 8-bit matrix
instructions returns the ids and the distance BITS of the float scan -- every sum is an integer below 2^24 -- and of a numpy int64
reference; anything it may not serve (a query value that is no byte, float data, d > 256) runs the float scan, and
Hgraph.scan_path() tells which ran.  All comparisons are equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALLOWED = [0, 31, 32, 258, 259, 484, 516]       # test_gpu_scan_family.py's: 7 < k, both sides of a mask word's edge, first and last row

N, NQ = 517, 33         # n: no multiple of the 32-row block; nq: one full tile of 32 queries plus one
FLOAT, BYTES = 1, 2     # scan_path()


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _bytes_data(d, seed=0):
    rng = np.random.default_rng(1000 * d + seed)
    X = rng.integers(0, 256, size=(N, d)).astype(np.float32)
    X[5], X[40] = 0, 255
    X[[77, 300, 516]] = X[12]               # three exact duplicates of one row: ties break by id
    Q = rng.integers(0, 256, size=(NQ, d)).astype(np.float32)
    Q[0], Q[NQ - 1] = 0, 255                # against X[40] / X[5] at d 256: 256 * 255^2 = 16 646 400 < 2^24
    Q[7] = X[12]
    return X, Q


def _reference(X, Q, metric, k):
    x, q = X.astype(np.int64), Q.astype(np.int64)
    s = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2) if metric == 0 else q @ x.T
    dist = np.sqrt(s.astype(np.float64)).astype(np.float32) if metric == 0 else np.float32(1) - s.astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(N), s.shape), s if metric == 0 else -s), axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(dist, order, 1)


def _scan(H, hg, on, k, Q):
    hg.set_option("scan_bytes", on)
    ids, dist = H.Ohnsw.brute_force_knn(hg, k, Q)
    return ids, dist.view(np.uint32), hg.scan_path()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 128, 200, 256])     # 64-byte rows nearly all padding; ragged and full 128- and 256-byte rows
def test_matrix_scan_returns_the_float_scans_bits(H, d, metric):
    X, Q = _bytes_data(d)
    hg = H.Hgraph.flat(X, metric=metric)
    assert hg.scan_path() == 0
    for slabs in (1, 3):
        hg.set_option("scan_slabs", slabs)
        for k in (1, 10, N):
            c = "d %d metric %d slabs %d k %d" % (d, metric, slabs, k)
            ids1, bits1, path1 = _scan(H, hg, 1, k, Q)
            ids0, bits0, path0 = _scan(H, hg, 0, k, Q)
            assert (path1, path0) == (BYTES, FLOAT), c
            np.testing.assert_array_equal(ids1, ids0, err_msg=c + " ids, on against off")
            np.testing.assert_array_equal(bits1, bits0, err_msg=c + " distance bits, on against off")
            rids, rdist = _reference(X, Q, metric, k)
            np.testing.assert_array_equal(ids1, rids, err_msg=c + " ids against int64")
            np.testing.assert_array_equal(bits1, rdist.view(np.uint32), err_msg=c + " distance bits against int64")
    hg.release()


@pytest.mark.parametrize("metric, slabs", [pytest.param(0, None, id="0"), pytest.param(1, None, id="1"),    # the plan's own slabs
                                           # three slabs: the edges at rows 173 and 346 fall inside mask words 5 and 10
                                           pytest.param(0, 3, id="0-slabs3"), pytest.param(1, 3, id="1-slabs3")])
def test_masked_matrix_scan(H, metric, slabs):
    X, Q = _bytes_data(100, seed=1)
    hg = H.Hgraph.flat(X, metric=metric)
    if slabs:
        hg.set_option("scan_slabs", slabs)
    mask = np.zeros(N, bool)
    mask[ALLOWED] = True                    # 7 allowed nodes < k: the filtered search goes straight to the exact stage
    out = {}
    for on in (1, 0):
        hg.set_option("scan_bytes", on)
        ids, dist = H.Ohnsw.knn_batch_filtered(hg, 10, Q, mask, ef=16)
        out[on] = (ids, dist.view(np.uint32), hg.scan_path())
    assert (out[1][2], out[0][2]) == (BYTES, FLOAT)
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(out[1][1], out[0][1])
    assert sorted(out[1][0][0, :7]) == ALLOWED and (out[1][0][:, 7:] == -1).all()
    hg.release()


@pytest.mark.parametrize("case", ["query 0.5", "query 256", "query -1", "float data", "d 300"])
def test_fallback_to_the_float_scan(H, case):
    X, Q = _bytes_data(300 if case == "d 300" else 100, seed=2)
    if case.startswith("query"):
        Q[NQ - 2, 17] = float(case.split()[1])      # one value of one query of the batch
    if case == "float data":
        X[100, 3] = 0.5
    hg = H.Hgraph.flat(X)
    ids1, bits1, path1 = _scan(H, hg, 1, 10, Q)
    ids0, bits0, path0 = _scan(H, hg, 0, 10, Q)
    assert (path1, path0) == (FLOAT, FLOAT), case
    np.testing.assert_array_equal(ids1, ids0)
    np.testing.assert_array_equal(bits1, bits0)
    hg.release()
