"""Half rows (ocaml-hnsw_amd/csrc/hnsw_rows16.hip, option "half_rows"): the knn searches read a copy of the vectors rounded
to fp16 and convert each half back to float exactly, then run the float32 rows' arithmetic.  The bar is the oracle over
Xh = X.astype(float16).astype(float32) (Space.l2 / ip with the kernel's TREE16 summation): ids, distance bits and hop counts
identical, for both metrics, both accept rules, every lane-grid width, plain and ordered launches, the exactness fallback,
grown and reloaded indices and the device entry points.  The option's states, refusals and the operators that stay on the
float32 rows are checked too, and recall on clustered data against the float32 rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF = 0, 2, 3, 4


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _half(X):
    return np.asarray(X, np.float32).astype(np.float16).astype(np.float32)


def _nch(d):
    per_lane = ((d + 3) // 4 + 15) // 16
    return next(c for c in (1, 2, 4, 8, 16) if per_lane <= c)


def _floats(n, d, seed, scale=3.0):
    """signed float data, most values not representable in fp16"""
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(n, d))).astype(np.float32)


def _unit(n, d, seed):
    X = _floats(n, d, seed, 1.0)
    return X / np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)


def _space(oracle, X, metric):
    return (oracle.Space.ip if metric else oracle.Space.l2)(_half(X), arith=oracle.TREE16)


def _graph(oracle, hg):
    hg.export()
    return oracle.Graph(hg.n, hg.entry_point, hg.deg0, hg.nbr0, hg.upper)


def _ohnsw_parity(H, oracle, hg, g, sp, Q, ef, k, ctx=""):
    ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
    oi, od, ond, onh = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=k, ef=ef, ties=oracle.TIES_CANONICAL, counters=True)
    np.testing.assert_array_equal(ids, oi, err_msg=ctx)
    np.testing.assert_array_equal(dist.view(np.uint32), od.view(np.uint32), err_msg=ctx)
    np.testing.assert_array_equal(nh, onh, err_msg=ctx)
    return ids, dist, nd, nh


def _functor_parity(H, oracle, hg, g, sp, Q, ef, k, ctx=""):
    gi, gd = H._search(hg, Q, ef, k, H.FILL_BA, sem=H.SEM_FUNCTOR)
    cd, ci = oracle.Functor.knn_batch(g, sp, Q, ef, k, ties=oracle.TIES_CANONICAL, with_ids=True)
    np.testing.assert_array_equal(gi, ci, err_msg=ctx)
    np.testing.assert_array_equal(gd.view(np.uint32), cd.view(np.uint32), err_msg=ctx)
    np.testing.assert_array_equal(H.Ba.knn_batch(hg, Q, ef, k).view(np.uint32), cd.view(np.uint32), err_msg=ctx)


# every lane-grid width (NCH 1, 2, 4, 8, 16), rows that fill it (64, 256) and ragged ones, d = 100 (split rows underneath)
@pytest.mark.parametrize("d", [20, 64, 96, 100, 128, 130, 256, 300, 960])
@pytest.mark.parametrize("metric", [0, 1])
def test_half_rows_equal_the_oracle_over_xh(H, oracle, d, metric):
    n, nq, M, efc = (1200, 48, 8, 40) if d > 256 else (3000, 96, 12, 60)
    X = _unit(n, d, 10 + d) if metric else _floats(n, d, 10 + d)
    Q = _unit(nq, d, 20 + d) if metric else _floats(nq, d, 20 + d)
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=3, metric=metric)
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_HALF and hg.row_bytes() == 2 * d
    g, sp = _graph(oracle, hg), _space(oracle, X, metric)
    for ef, k in ((16, 5), (100, 10), (300, 10)):
        ctx = "d %d metric %d ef %d" % (d, metric, ef)
        _ohnsw_parity(H, oracle, hg, g, sp, Q, ef, k, ctx)
        _functor_parity(H, oracle, hg, g, sp, Q[:32], ef, k, ctx + " functor")
    hg.set_option("order_queries", 1)             # the descent pre-pass reads the half rows too
    _ohnsw_parity(H, oracle, hg, g, sp, Q, 100, 10, "ordered d %d metric %d" % (d, metric))
    hg.release()


def test_conversion_edge_cases(H, oracle):
    """round-to-nearest-even ties, fp16 subnormals, -0.0, +-65504 and values that round down to it: the searches equal the
    oracle over numpy's conversion"""
    rng = np.random.default_rng(7)
    n, d = 2500, 32
    X = _floats(n, d, 7)
    specials = np.array([1 + 2 ** -11, 1 + 3 * 2 ** -11, -(1 + 2 ** -11), 2048 + 1, 2048 + 3, -2048 - 1,   # ties
                         2 ** -24, 3 * 2 ** -25, 2 ** -25, 5 * 2 ** -26, -(2 ** -20), 6e-5, 2 ** -14 - 2 ** -25,  # subnormals
                         -0.0, 0.0, 65504.0, -65504.0, 65519.0, -65519.996, 1e-30], np.float32)
    pos = rng.integers(0, n * d, size=(4000,))
    X.reshape(-1)[pos] = specials[rng.integers(0, len(specials), size=pos.shape)]
    Xh = _half(X)
    assert (np.signbit(Xh) == np.signbit(X)).all()                     # -0 (and the signs of underflows) kept
    Q = _floats(64, d, 8)
    Q[:8] = X[:8]
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=5)
    hg.set_option("half_rows", 1)
    g, sp = _graph(oracle, hg), _space(oracle, X, 0)
    for ef, k in ((16, 5), (100, 10), (300, 10)):
        _ohnsw_parity(H, oracle, hg, g, sp, Q, ef, k, "edge ef %d" % ef)
    _functor_parity(H, oracle, hg, g, sp, Q, 100, 10, "edge functor")
    hg.release()


@pytest.mark.parametrize("bad", [65520.0, -65520.0, 1e6, np.inf, np.nan])
def test_values_beyond_fp16_are_refused(H, bad):
    X = _floats(800, 24, 9)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    hg.export()
    Xb = X.copy()
    Xb[517, 11] = bad
    hb = H.Hgraph(Xb, hg.deg0, hg.nbr0, hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree)
    before = hb.info()
    with pytest.raises(H.Failure, match=r"\[-7\].*fp16"):
        hb.set_option("half_rows", 1)
    after = hb.info()
    assert after.row_format == before.row_format == ROWS_F32 and after.device_bytes == before.device_bytes
    assert hb.row_bytes() == 4 * 24
    hb.release()
    hg.set_option("half_rows", 1)                 # the same graph over finite values below 65520 takes the copy
    assert hg.info().row_format == ROWS_HALF
    hg.release()


def test_option_states_and_device_bytes(H):
    for d, plain in ((128, ROWS_F32), (100, ROWS_SPLIT)):      # d = 100: split rows underneath, half rows take precedence
        n = 3000
        X, Q = _floats(n, d, 30 + d), _floats(200, d, 40 + d)
        hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=2)
        fresh = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
        b0 = hg.info().device_bytes
        assert hg.info().row_format == plain and hg.row_bytes() == 4 * d
        hg.set_option("half_rows", 1)
        assert hg.info().row_format == ROWS_HALF and hg.row_bytes() == 2 * d
        assert hg.info().device_bytes == b0 + n * 128 * _nch(d)
        half = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)
        hg.set_option("half_rows", 0)                            # back to what it was, the copy kept
        assert hg.info().row_format == plain and hg.row_bytes() == 4 * d
        assert hg.info().device_bytes == b0 + n * 128 * _nch(d)
        again = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
        for a, b in ((fresh[0], again[0]), (fresh[1].view(np.uint32), again[1].view(np.uint32)), (fresh[3], again[3])):
            np.testing.assert_array_equal(a, b)
        hg.set_option("half_rows", 1)                            # the kept copy serves again
        assert hg.info().row_format == ROWS_HALF
        np.testing.assert_array_equal(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)[1].view(np.uint32), half[1].view(np.uint32))
        hg.set_option("half_rows", -1)                           # ... and freed
        assert hg.info().row_format == plain and hg.info().device_bytes == b0
        np.testing.assert_array_equal(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)[0], fresh[0])
        hg.release()


def test_byte_rows_come_first(H):
    rng = np.random.default_rng(4)
    X = rng.integers(0, 256, size=(1500, 64)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    b0 = hg.info().device_bytes
    assert hg.info().row_format == ROWS_BYTES
    with pytest.raises(H.InvalidArgument, match="byte_rows 0"):
        hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_BYTES and hg.info().device_bytes == b0 and hg.row_bytes() == 64
    want = H.Ohnsw.knn_batch_bigarray(hg, 10, X[:100], ef=64)
    hg.set_option("byte_rows", 0)
    hg.set_option("half_rows", 1)                 # integers 0..255 are exact in fp16: the same results
    assert hg.info().row_format == ROWS_HALF and hg.row_bytes() == 128
    got = H.Ohnsw.knn_batch_bigarray(hg, 10, X[:100], ef=64)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    hg.set_option("byte_rows", 1)
    assert hg.info().row_format == ROWS_BYTES
    hg.release()


def test_ties_and_the_exactness_fallback(H, oracle):
    """the tie-heavy shape of test_gpu_parity.py::test_tie_overflow_beyond_lds_stack (more than 64 tied, evicted, still
    expandable entries) over half rows: the host call's re-run and the device entry point's slab both equal the oracle"""
    import torch
    n = 229
    pos = np.zeros(n, np.float32)
    pos[0] = 20.0
    pos[1:128] = 10.0
    pos[128:228] = 9.0 - 0.01 * np.arange(100)
    pos[228] = 0.1
    rows = [[] for _ in range(n)]
    rows[0] = [1] + list(range(2, 65))
    rows[1] = list(range(65, 128)) + [128]
    for i in range(99):
        rows[128 + i] = [129 + i]
    rows[40] = [228]
    deg0 = np.array([len(r) for r in rows], np.int32)
    nbr0 = np.full((n, 64), -1, np.int32)
    for i, r in enumerate(rows):
        nbr0[i, :len(r)] = r
    X = pos[:, None]
    g = oracle.Graph(n, 0, deg0, nbr0)
    sp = _space(oracle, X, 0)
    hg = H.Hgraph(X, deg0, nbr0, entry_point=0, max_degree=32)
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_HALF
    Q = np.array([[0.0], [0.05], [-0.3]], np.float32)
    want = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=10, ef=128, ties=oracle.TIES_CANONICAL, counters=True)
    got = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=128, counters=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(got[3], want[3])
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    ids = torch.empty((3, 10), dtype=torch.int32, device=dev)
    dd = torch.empty((3, 10), dtype=torch.float32, device=dev)
    nh = torch.zeros(3, dtype=torch.int32, device=dev)
    st = torch.zeros(3, dtype=torch.int32, device=dev)
    hg.set_option("device_fallback_slab_bytes", 4 * n * 8)
    H.search_batch_device(hg, Qd.data_ptr(), 3, 1, 128, 10, ids.data_ptr(), dd.data_ptr(), 0, nh.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ((st.cpu().numpy() & 1) == 0).all()
    np.testing.assert_array_equal(ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(dd.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(nh.cpu().numpy(), want[3])
    hg.set_option("device_fallback_slab_bytes", 0)
    hg.release()


def test_operators_stay_on_float32_rows(H):
    n, d = 3000, 96
    X, T = _floats(n, d, 50), _floats(40, d, 51)
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=6)
    hg.export()
    rng = np.random.default_rng(52)
    ids = rng.integers(0, n, size=(40, 33)).astype(np.int32)
    cands = [list(rng.choice(n, size=40, replace=False)) for _ in range(40)]
    starts = [[int(s)] for s in rng.integers(0, n, size=40)]

    def run():
        return (H.Ohnsw.search_k(hg, 0, starts, T, 10, ef=50, counters=True),
                H.Ohnsw.search_one(hg, 0, 0, T, with_distance=True),
                H.Ohnsw.distance_l2(hg, T, ids),
                H.Ohnsw.select_neighbours(hg, T, cands, 12))
    a = run()
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_HALF
    b = run()
    assert a[0][0] == b[0][0]
    np.testing.assert_array_equal(a[0][1], b[0][1])
    np.testing.assert_array_equal(a[1][0], b[1][0])
    np.testing.assert_array_equal(a[1][1].view(np.uint32), b[1][1].view(np.uint32))
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a[3] == b[3]
    hg.release()


def test_insert_save_load_and_device_entry_points(H, oracle, tmp_path):
    import torch
    n0, m, d = 3000, 1000, 64
    X, Q = _floats(n0 + m, d, 60), _floats(300, d, 61)
    hg = H.Ohnsw.build_batch_bigarray(X[:n0], 12, 60, seed=8)
    hg.set_option("half_rows", 1)
    H.Ohnsw.insert_batch(hg, X[n0:], 12, 60, seed=8)
    assert hg.n == n0 + m and hg.info().row_format == ROWS_HALF
    g, sp = _graph(oracle, hg), _space(oracle, X, 0)
    want = _ohnsw_parity(H, oracle, hg, g, sp, Q, 100, 10, "grown")
    # new vectors that do not fit fp16: the whole insert is refused, the index as it was
    b0, n_before = hg.info().device_bytes, hg.info().n
    bad = _floats(10, d, 62)
    bad[3, 5] = 70000.0
    with pytest.raises(H.Failure, match=r"\[-7\]"):
        H.Ohnsw.insert_batch(hg, bad, 12, 60, seed=8)
    assert hg.info().n == n_before and hg.info().device_bytes == b0 and hg.info().row_format == ROWS_HALF
    got = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    # device-resident queries and results, and submit / wait: the host call's bits
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    ids = torch.empty((300, 10), dtype=torch.int32, device=dev)
    dd = torch.empty((300, 10), dtype=torch.float32, device=dev)
    H.search_batch_device(hg, Qd.data_ptr(), 300, d, 100, 10, ids.data_ptr(), dd.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(dd.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    req = H.submit(hg, Q, 100, 10)
    si, sd = req.wait()[:2]
    np.testing.assert_array_equal(si, want[0])
    np.testing.assert_array_equal(sd.view(np.uint32), want[1].view(np.uint32))
    # saved and loaded: the option is not part of the file
    p = str(tmp_path / "half.bin")
    hg.save(p)
    h2 = H.Hgraph.load(p)
    assert h2.info().row_format == ROWS_F32 and h2.row_bytes() == 4 * d
    h2.set_option("half_rows", 1)
    got = H.Ohnsw.knn_batch_bigarray(h2, 10, Q, ef=100)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for h in (hg, h2):
        h.release()


def test_random_shapes_soak(H, oracle):
    """a short randomised run: shapes, metrics, ef, k and launch order drawn at random; zero mismatches against the oracle"""
    rng = np.random.default_rng(2026)
    for it in range(8):
        d = int(rng.choice([8, 33, 70, 96, 100, 128, 150, 200, 257, 384]))
        metric = int(rng.integers(0, 2))
        n = int(rng.integers(500, 2500))
        M = int(rng.choice([4, 8, 16]))
        X = _unit(n, d, 1000 + it) if metric else _floats(n, d, 1000 + it, float(rng.choice([0.01, 1.0, 100.0])))
        Q = _unit(64, d, 2000 + it) if metric else _floats(64, d, 2000 + it, 1.0) * X.std()
        hg = H.Ohnsw.build_batch_bigarray(X, M, 40, seed=it, metric=metric)
        hg.set_option("half_rows", 1)
        hg.set_option("order_queries", int(rng.integers(0, 2)))
        g, sp = _graph(oracle, hg), _space(oracle, X, metric)
        ef = int(rng.integers(1, 400))
        k = int(rng.integers(1, ef + 1))
        _ohnsw_parity(H, oracle, hg, g, sp, Q, ef, min(k, 100), "soak %d: d %d metric %d n %d M %d ef %d" % (it, d, metric, n, M, ef))
        hg.release()


def _clustered(n, d, centers, seed):
    """L2: Gaussian blobs"""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d)).astype(np.float32) * 4
    return (C[rng.integers(0, centers, n)] + rng.normal(size=(n, d)).astype(np.float32)).astype(np.float32)


def _clustered_unit(n, d, centers, seed, spread=1.5):
    """IP: unit vectors around `centers` directions, bench.py's recipe for C3's clustered set (word-embedding-like).  (On
    unit-normalised Gaussian blobs as tight as _clustered's the half rows lose more: recall@10 0.9973 -> 0.9917 at 50 k x 100;
    fp16's 11 bits cannot order neighbours whose inner products differ by less than ~1e-4.)"""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = C[rng.integers(0, centers, n)] + spread * rng.normal(size=(n, d)) / d ** 0.5
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("d,metric", [(96, 0), (100, 1)])
def test_recall_close_to_float32_rows(H, d, metric):
    import torch
    n, nq, k = 50000, 1000, 10
    X = _clustered_unit(n + nq, d, 256, 70 + d) if metric else _clustered(n + nq, d, 256, 70 + d)
    X, Q = X[:n], X[n:]
    dev = torch.device("cuda", 0)
    Xt, Qt = torch.from_numpy(X).to(dev), torch.from_numpy(Q).to(dev)
    s = Qt @ Xt.T if metric else -(torch.cdist(Qt, Xt))
    truth = torch.topk(s, k, dim=1).indices.cpu().numpy()
    hg = H.Ohnsw.build_batch_bigarray(X, 16, 100, seed=1, metric=metric)

    def recall():
        ids = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=64)[0]
        return np.mean([len(set(a) & set(b)) / k for a, b in zip(ids, truth)])
    r32 = recall()
    hg.set_option("half_rows", 1)
    r16 = recall()
    assert r32 > 0.8, r32
    assert r16 >= r32 - 0.005, (r16, r32)
    hg.release()
