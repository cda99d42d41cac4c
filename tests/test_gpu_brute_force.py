"""hnsw_brute_force_batch on the device against the oracle's exact scan, bit for bit: ids by assert_array_equal, distances as
uint32 views, `oracle.brute_force_knn(Space.l2 / ip(X, arith=TREE16), Q, k)` the check.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    if H.device_count() < 1:
        pytest.skip("no HIP device")
    return H


def _space(oracle, metric, X):
    return (oracle.Space.ip if metric else oracle.Space.l2)(X, arith=oracle.TREE16)


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))


def _data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


# every d (each lane-grid class, ragged last chunks, the LDS query path from d = 257 on), k, n and nq of the axes occurs; the cross
# product is thinned so that the oracle's n * nq * d stays near 1.4e10 over both metrics
GRID = [  # (d, n, nq, k)
    (3, 1, 1, 1), (3, 63, 7, 10), (3, 20011, 300, 100),
    (16, 1000, 7, 100), (16, 20011, 300, 10), (16, 20011, 1, 1024),
    (64, 1000, 300, 1), (64, 63, 7, 100), (64, 20011, 7, 1024),
    (65, 20011, 7, 1024), (65, 1000, 1, 10), (65, 20011, 300, 1),
    (100, 20011, 300, 100), (100, 63, 1, 10), (100, 1000, 7, 1024),
    (128, 20011, 300, 10), (128, 1000, 7, 1024), (128, 1, 7, 1), (128, 20011, 1, 100),
    (257, 1000, 300, 10), (257, 20011, 7, 100), (257, 63, 1, 1024),
    (784, 1000, 7, 10), (784, 20011, 300, 1), (784, 20011, 7, 1024), (784, 63, 1, 100),
    (1024, 20011, 7, 10), (1024, 1000, 300, 100), (1024, 63, 1, 1), (1024, 1, 1, 1024),
]


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("d,n,nq,k", GRID)
def test_parity_grid(H, oracle, metric, d, n, nq, k):
    X, Q = _data(1000 * d + n + nq + k + metric, n, d, nq)
    hg = H.Hgraph.flat(X, metric=metric)
    _same(H.Ohnsw.brute_force_knn(hg, k, Q), oracle.brute_force_knn(_space(oracle, metric, X), Q, k))
    hg.release()


def _levels(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, size=(n, d)).astype(np.float32), rng.integers(0, 4, size=(nq, d)).astype(np.float32)


@pytest.mark.parametrize("metric,k", [(0, 100), (1, 10), (1, 100)], ids=["l2-100", "ip-10", "ip-100"])
def test_ties_lowest_ids_win(H, oracle, metric, k):
    """integer-valued "levels" data: many vectors are exactly as far as the k-th, so the lowest ids must win, in id order"""
    X, Q = _levels(11, 5000, 8, 40)
    sp = _space(oracle, metric, X)
    want = oracle.brute_force_knn(sp, Q, k)
    # the oracle alone: some query really has >= 64 vectors on its k-th distance
    every = oracle.brute_force_knn(sp, Q[:8], X.shape[0])[1]
    on_kth = (every == every[:, k - 1:k]).sum(1)
    print("vectors on the k-th distance, per query:", on_kth.tolist())
    assert on_kth.max() >= 64
    _same(H.Ohnsw.brute_force_knn(H.Hgraph.flat(X, metric=metric), k, Q), want)


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
def test_identical_vectors_come_in_id_order(H, oracle, metric):
    X = np.tile(np.random.default_rng(3).standard_normal((1, 20)).astype(np.float32), (3000, 1))
    Q = np.random.default_rng(4).standard_normal((5, 20)).astype(np.float32)
    ids, dist = H.Ohnsw.brute_force_knn(H.Hgraph.flat(X, metric=metric), 70, Q)
    np.testing.assert_array_equal(ids, np.tile(np.arange(70, dtype=np.int32), (5, 1)))
    _same((ids, dist), oracle.brute_force_knn(_space(oracle, metric, X), Q, 70))


def test_survivor_buffer_compacts_again_and_again(H, oracle):
    """rows stored in DESCENDING distance to the queries: every row beats the current threshold, k = 1024"""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((60000, 16)).astype(np.float32)
    X = np.ascontiguousarray(X[np.argsort(-(X.astype(np.float64) ** 2).sum(1), kind="stable")])
    Q = (0.001 * rng.standard_normal((9, 16))).astype(np.float32)
    want = oracle.brute_force_knn(_space(oracle, 0, X), Q, 1024)
    hg = H.Hgraph.flat(X)
    for slabs in (0, 1, 3):
        hg.set_option("scan_slabs", slabs)
        _same(H.Ohnsw.brute_force_knn(hg, 1024, Q), want)


def test_result_does_not_depend_on_the_cut(H, oracle):
    import torch
    X, Q = _data(31, 20011, 100, 300)
    k = 10
    want = oracle.brute_force_knn(_space(oracle, 0, X), Q, k)
    hg = H.Hgraph.flat(X)
    _same(H.Ohnsw.brute_force_knn(hg, k, Q), want)                       # inside a large batch
    for q in (0, 7, 299):                                                 # alone
        _same(H.Ohnsw.brute_force_knn(hg, k, Q[q:q + 1]), (want[0][q:q + 1], want[1][q:q + 1]))
    _same(H.Ohnsw.brute_force_knn(hg, k, Q[5:18]), (want[0][5:18], want[1][5:18]))
    for slabs in (1, 2, 37, 1024):                                        # the slab-count knob
        hg.set_option("scan_slabs", slabs)
        _same(H.Ohnsw.brute_force_knn(hg, k, Q), want)
    hg.set_option("scan_slabs", 0)
    dev = torch.device("cuda", 0)                                         # the device entry point on a stream of its own
    Qd = torch.from_numpy(Q).to(dev)
    ids = torch.empty((300, k), dtype=torch.int32, device=dev)
    dd = torch.empty((300, k), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    H.brute_force_device(hg, Qd.data_ptr(), 300, 100, k, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    _same((ids.cpu().numpy(), dd.cpu().numpy()), want)


def test_conventions(H, oracle):
    X, Q = _data(41, 50, 24, 6)
    sp = _space(oracle, 0, X)
    wi, wd = oracle.brute_force_knn(sp, Q, 10)
    _same(H.Ohnsw.brute_force_knn(H.Hgraph.flat(X, id_base=1), 10, Q), (wi + 1, wd))          # id_base 1 gives ids + 1
    hg = H.Hgraph.flat(X)
    # k > n under both fills: the oracle's -1 / NaN, and -1 / +inf
    wi, wd = oracle.brute_force_knn(sp, Q, 64)
    assert (wi[:, 50:] == -1).all() and np.isnan(wd[:, 50:]).all()
    _same(H.Ohnsw.brute_force_knn(hg, 64, Q), (wi, wd))
    ids, dist = H.Ohnsw.brute_force_knn(hg, 64, Q, fill=H.FILL_BA)
    _same((ids[:, :50], dist[:, :50]), (wi[:, :50], wd[:, :50]))
    assert (ids[:, 50:] == -1).all() and np.isposinf(dist[:, 50:]).all()
    # n = 0: all fill, HNSW_OK
    empty = H.Hgraph.flat(np.zeros((0, 24), np.float32))
    ids, dist = H.Ohnsw.brute_force_knn(empty, 5, Q)
    assert (ids == -1).all() and np.isnan(dist).all()
    ids, dist = H.Ohnsw.brute_force_knn(empty, 5, Q, fill=H.FILL_BA)
    assert (ids == -1).all() and np.isposinf(dist).all()
    # the limits
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.brute_force_knn(hg, 0, Q)
    with pytest.raises(H.Failure, match=r"\[-7\].*k=1025"):
        H.Ohnsw.brute_force_knn(hg, 1025, Q)
    with pytest.raises(H.InvalidArgument, match="fill"):
        H.Ohnsw.brute_force_knn(hg, 5, Q, fill=7)
    # q_stride and null pointers, as hnsw_search_batch refuses them
    L = H.load()
    ids = np.empty((6, 5), np.int32)
    dist = np.empty((6, 5), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.hnsw_brute_force_batch(hg.handle, p(Q), 6, 23, 5, 0, p(ids), p(dist)) == H.ERR_BAD_ARG
    assert b"q_stride" in L.hnsw_last_error()
    for args in ((None, 6, 24, 5, 0, p(ids), p(dist)), (p(Q), 6, 24, 5, 0, None, p(dist)), (p(Q), 6, 24, 5, 0, p(ids), None),
                 (p(Q), -1, 24, 5, 0, p(ids), p(dist))):
        assert L.hnsw_brute_force_batch(hg.handle, *args) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch(None, p(Q), 6, 24, 5, 0, p(ids), p(dist)) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch(hg.handle, None, 0, 24, 5, 0, None, None) == H.OK          # nq == 0 is a no-op
    assert L.hnsw_brute_force_batch_device(hg.handle, None, 6, 24, 5, 0, None, None, None) == H.ERR_BAD_ARG
    # a wider stride than d
    Qw = np.zeros((6, 40), np.float32)
    Qw[:, :24] = Q
    _same(H.Ohnsw.brute_force_knn(hg, 10, Qw[:, :24]), oracle.brute_force_knn(sp, Q, 10))


def test_registered_and_plain_matrices_agree(H, oracle):
    X, Q = _data(51, 5000, 128, 200)
    want = oracle.brute_force_knn(_space(oracle, 0, X), Q, 10)
    hg = H.Hgraph.flat(X)
    _same(H.Ohnsw.brute_force_knn(hg, 10, Q), want)
    Qp = H.host_empty(Q.shape)
    Qp[:] = Q
    out = (H.host_empty((200, 10), np.int32), H.host_empty((200, 10), np.float32))
    got = H.Ohnsw.brute_force_knn(hg, 10, Qp, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    _same(got, want)
    Qr = H.pin(Q.copy())
    try:
        _same(H.Ohnsw.brute_force_knn(hg, 10, Qr), want)
    finally:
        H.unpin(Qr)


def test_scan_reads_the_float32_rows_whatever_the_searches_read(H, oracle, tmp_path):
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, size=(3000, 32)).astype(np.float32)
    Q = rng.uniform(-1, 1, size=(40, 32)).astype(np.float32)
    want = oracle.brute_force_knn(_space(oracle, 0, X), Q, 10)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    _same(H.Ohnsw.brute_force_knn(hg, 10, Q), want)
    # half rows: the searches read Xh, the scan still X -- and the two differ
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == H.ROWS_HALF
    Xh = X.astype(np.float16).astype(np.float32)
    over_half = oracle.brute_force_knn(_space(oracle, 0, Xh), Q, 10)
    assert not np.array_equal(over_half[1].view(np.uint32), want[1].view(np.uint32))
    _same(H.Ohnsw.brute_force_knn(hg, 10, Q), want)
    hg.set_option("half_rows", 0)
    # a saved and loaded index
    path = str(tmp_path / "index.bin")
    hg.save(path)
    _same(H.Ohnsw.brute_force_knn(H.Hgraph.load(path), 10, Q), want)
    # after an insert the scan covers the grown table
    more = rng.uniform(-1, 1, size=(500, 32)).astype(np.float32)
    H.Ohnsw.insert_batch(hg, more, 8, 40, seed=1)
    grown = np.concatenate([X, more])
    _same(H.Ohnsw.brute_force_knn(hg, 10, Q), oracle.brute_force_knn(_space(oracle, 0, grown), Q, 10))
    # the library's own distances for the same pairs
    ids, dist = H.Ohnsw.brute_force_knn(hg, 10, Q)
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32))


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
def test_byte_rows_in_use_change_nothing(H, oracle, metric):
    rng = np.random.default_rng(71)
    X = rng.integers(0, 256, size=(4000, 128)).astype(np.float32)
    Q = rng.integers(0, 256, size=(30, 128)).astype(np.float32)
    want = oracle.brute_force_knn(_space(oracle, metric, X), Q, 10)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1, metric=metric)
    assert hg.info().row_format == H.ROWS_BYTES
    got = H.Ohnsw.brute_force_knn(hg, 10, Q)
    _same(got, want)
    hg.set_option("byte_rows", 0)
    _same(H.Ohnsw.brute_force_knn(hg, 10, Q), want)
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, got[0]).view(np.uint32), got[1].view(np.uint32))


def test_recall_against_the_scan_is_exact(H, oracle):
    """What it is for: against the scan's distances Recall.compute (epsilon 1e-8) counts exactly the neighbours id recall counts"""
    from ocaml_hnsw_amd import dataset
    rng = np.random.default_rng(81)
    X = rng.uniform(-1, 1, size=(50000, 32)).astype(np.float32)
    Q = rng.uniform(-1, 1, size=(500, 32)).astype(np.float32)
    k = 10
    # the seed: for every query the oracle's (k+1)-th exact distance differs from its k-th (one float32 step is about 2e-7 here)
    od = oracle.brute_force_knn(_space(oracle, 0, X), Q, k + 1)[1]
    assert (od[:, k] != od[:, k - 1]).all()
    hg = H.Ohnsw.build_batch_bigarray(X, 16, 100, seed=1)
    scan_ids, scan_dist = H.Ohnsw.brute_force_knn(hg, k, Q)
    np.testing.assert_array_equal(scan_dist.view(np.uint32), od[:, :k].view(np.uint32))
    knn_ids, knn_dist = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=40)
    by_distance, by_id = dataset.Recall.compute(scan_dist, knn_dist), dataset.Recall.ids(scan_ids, knn_ids)
    print("recall by distance %.6f, by id %.6f; against the float64 CPU ground truth %.6f"
          % (by_distance, by_id, dataset.Recall.compute(dataset.brute_force_knn_l2(X, Q, k), knn_dist)))
    assert by_distance == by_id
    np.testing.assert_array_equal(dataset.brute_force_knn_l2(X, Q[:50], k, device=0).view(np.uint32), scan_dist[:50].view(np.uint32))


def test_full_size_c2_shape(H, oracle):
    """1 M x 128 byte-valued vectors, 64 queries, k 10, against the oracle"""
    rng = np.random.default_rng(91)
    X = rng.integers(0, 256, size=(1000000, 128), dtype=np.uint8).astype(np.float32)
    Q = rng.integers(0, 256, size=(64, 128), dtype=np.uint8).astype(np.float32)
    _same(H.Ohnsw.brute_force_knn(H.Hgraph.flat(X), 10, Q), oracle.brute_force_knn(_space(oracle, 0, X), Q, 10))
