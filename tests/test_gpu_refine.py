"""The exact re-rank (ocaml-hnsw_amd/csrc/hnsw_rerank.hip): hnsw_rerank_batch / _device as an operator, and option "refine", which
runs it over the head of W behind a half-row search.

Operator: the k smallest of the given candidates under (distance key, node id) over the float32 rows, the distance bits those of
hnsw_distance_batch for the same pair.  Option: W is what the oracle returns over Xh = X.astype(float16).astype(float32) with
k := c = min(ef, max(k, R)) (ef for R = -1), the distances are TREE16 over X, the order (distance key, id), the answer the first k.

The order among candidates whose float32 L2 distances are EQUAL is decided by the squared distance the kernels order by (the
square root rounds neighbouring squares to one float): the expected order takes it from the oracle's TREE16 sum for exactly those
pairs, then the id.  (The oracle's batched functor search reports no hop counts: for that rule the hops are held against the
unrefined call's, which the option must not change; for the Ohnsw rule against the oracle's.)"""
import os
import subprocess

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


def _fill_value(fill):
    return np.float32(np.nan) if fill == 0 else np.float32(np.inf)


def _tree16(oracle, X, q, ids0, metric):
    """(order key, distance) of the pairs (q, X[ids0]) in the kernels' summation order, float32"""
    if metric:
        dist = np.array([np.float32(1.0) - np.float32(oracle.dot_tree16(X[j], q)) for j in ids0], np.float32)
        return dist, dist
    sq = np.array([oracle.l2sq_tree16(X[j], q) for j in ids0], np.float32)
    return sq, np.sqrt(sq.astype(np.float64)).astype(np.float32)


def _order(oracle, X, q, ids0, dist, metric):
    """positions of the candidates in ascending (distance key, id): by distance; L2 candidates at one float distance by their
    squared distance; then by id"""
    sub = np.zeros(len(ids0), np.float32)
    if not metric and len(ids0):
        vals, inv, cnt = np.unique(dist, return_inverse=True, return_counts=True)
        for pos in np.flatnonzero(cnt[inv] > 1):
            sub[pos] = oracle.l2sq_tree16(X[ids0[pos]], q)
    return np.lexsort((ids0, sub, dist))


def _expect_rerank(H, oracle, hg, X, Q, cand, k, metric, fill=0):
    """the operator's definition from hnsw_distance_batch's bits"""
    base, n = hg.id_base, X.shape[0]
    real = (cand >= base) & (cand < base + n)
    D = H.Ohnsw.distance_l2(hg, Q, np.where(real, cand, base).astype(np.int32))
    ids = np.full((len(Q), k), -1, np.int32)
    dist = np.full((len(Q), k), _fill_value(fill), np.float32)
    for q in range(len(Q)):
        ids0 = (cand[q][real[q]] - base).astype(np.int64)
        dq = D[q][real[q]]
        o = _order(oracle, X, Q[q], ids0, dq, metric)[:k]
        ids[q, :len(o)] = ids0[o] + base
        dist[q, :len(o)] = dq[o]
    return ids, dist


def _same(got, want, ctx=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx)


def _ragged(rng, nq, stride, n, base):
    """[nq][stride] candidate lists: distinct real ids at random positions, the rest padding (-1, base - 1, -7)"""
    cand = np.empty((nq, stride), np.int32)
    for q in range(nq):
        m = int(rng.integers(0, min(stride, n) + 1)) if q % 3 else min(stride, n)
        row = rng.choice(np.array([-1, base - 1, -7]), size=stride).astype(np.int32)
        row[rng.choice(stride, size=m, replace=False)] = rng.choice(n, size=m, replace=False) + base
        cand[q] = row
    return cand


# ---- the operator ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [20, 64, 100, 128, 300, 960])       # every lane-grid width (NCH 1, 2, 4, 8, 16), full and ragged rows
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("id_base", [0, 1])
def test_rerank_equals_lexsort_of_distance_batch(H, oracle, d, metric, id_base):
    n, nq = 2000, 12
    X = _unit(n, d, 100 + d) if metric else _floats(n, d, 100 + d)
    Q = _unit(nq, d, 200 + d) if metric else _floats(nq, d, 200 + d)
    hg = H.Hgraph.flat(X, metric=metric, id_base=id_base)
    rng = np.random.default_rng(300 + d + metric)
    for stride, k in ((1, 1), (17, 10), (64, 64), (1024, 100)):
        cand = _ragged(rng, nq, stride, n, id_base)
        got = H.Ohnsw.rerank(hg, k, Q, cand)
        _same(got, _expect_rerank(H, oracle, hg, X, Q, cand, k, metric), "d %d metric %d base %d stride %d" % (d, metric, id_base, stride))
    hg.release()


@pytest.mark.parametrize("metric", [0, 1])
def test_forced_ties_come_lowest_id_first(H, oracle, metric):
    d, copies = 48, 20
    B = _unit(50, d, 1) if metric else _floats(50, d, 1)
    X = np.tile(B, (copies, 1))                     # vector j again at j + 50, j + 100, ...
    Q = _unit(6, d, 2) if metric else _floats(6, d, 2)
    hg = H.Hgraph.flat(X, metric=metric)
    rng = np.random.default_rng(3)
    cand = np.full((6, 1024), -1, np.int32)
    for q in range(6):
        cand[q, rng.choice(1024, size=1000, replace=False)] = rng.permutation(1000)
    ids, dist = H.Ohnsw.rerank(hg, 200, Q, cand)
    _same((ids, dist), _expect_rerank(H, oracle, hg, X, Q, cand, 200, metric))
    for q in range(6):                              # ten groups of twenty equal distances, each ascending in id
        groups = ids[q].reshape(10, copies)
        assert (np.diff(groups, axis=1) == 50).all() and (groups[:, 0] < 50).all()
        assert (dist[q].reshape(10, copies) == dist[q].reshape(10, copies)[:, :1]).all()
    hg.release()


@pytest.mark.parametrize("fill", [0, 1])
def test_fewer_than_k_candidates_are_filled(H, oracle, fill):
    X, Q = _floats(300, 24, 4), _floats(3, 24, 5)
    hg = H.Hgraph.flat(X)
    cand = np.full((3, 12), -1, np.int32)
    cand[0, [1, 5, 9]] = [7, 299, 0]
    cand[2] = np.arange(12) + 40
    ids, dist = H.Ohnsw.rerank(hg, 8, Q, cand, fill=H.FILL_BA if fill else H.FILL_OHNSW)
    _same((ids, dist), _expect_rerank(H, oracle, hg, X, Q, cand, 8, 0, fill))
    assert sorted(ids[0, :3]) == [0, 7, 299] and (ids[0, 3:] == -1).all() and (ids[1] == -1).all() and (ids[2] >= 40).all()
    gap = np.concatenate([dist[0, 3:], dist[1]])
    assert (np.isinf(gap) & (gap > 0)).all() if fill else np.isnan(gap).all()
    hg.release()


def test_refusals(H):
    X, Q = _floats(200, 16, 6), _floats(4, 16, 7)
    hg = H.Hgraph.flat(X, id_base=1)
    L = H.load()
    cand = np.tile(np.arange(1, 9, dtype=np.int32), (4, 1))
    ids, dist = np.empty((4, 8), np.int32), np.empty((4, 8), np.float32)

    def rc(k, fill=0, stride=8, c=cand, nq=4):
        return L.hnsw_rerank_batch(hg.handle, Q.ctypes.data, nq, 16, c.ctypes.data, stride, k, fill, ids.ctypes.data, dist.ctypes.data)
    assert rc(8) == H.OK
    assert rc(0) == H.ERR_BAD_ARG and rc(-1) == H.ERR_BAD_ARG
    assert rc(9) == H.ERR_BAD_ARG                                     # k > cand_stride
    assert rc(4, fill=2) == H.ERR_BAD_ARG
    assert rc(4, stride=0) == H.ERR_BAD_ARG
    assert rc(4, stride=1025) == H.ERR_UNSUPPORTED
    big = np.zeros((4, 1025), np.int32)
    assert rc(1025, stride=1025, c=big) == H.ERR_UNSUPPORTED
    bad = cand.copy()
    bad[2, 3] = 201                                                   # id_base + n: the first id that does not exist
    assert rc(4, c=bad) == H.ERR_BAD_ARG and b"out of range" in L.hnsw_last_error()
    bad[2, 3] = 200                                                   # the last one that does
    assert rc(4, c=bad) == H.OK
    assert rc(4, nq=-1) == H.ERR_BAD_ARG
    before = ids.copy()
    assert rc(4, nq=0) == H.OK and (ids == before).all()              # a no-op
    assert L.hnsw_rerank_batch(hg.handle, None, 4, 16, cand.ctypes.data, 8, 4, 0, ids.ctypes.data, dist.ctypes.data) == H.ERR_BAD_ARG
    assert L.hnsw_rerank_batch(hg.handle, Q.ctypes.data, 4, 15, cand.ctypes.data, 8, 4, 0, ids.ctypes.data, dist.ctypes.data) == H.ERR_BAD_ARG
    for k, stride in ((0, 8), (9, 8), (4, 1025)):                     # the device form checks the same before it launches
        want = H.ERR_UNSUPPORTED if stride > 1024 else H.ERR_BAD_ARG
        assert L.hnsw_rerank_batch_device(hg.handle, 1, 4, 16, 1, stride, k, 0, 1, 1, None) == want
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.rerank(hg, 3, Q, cand[:3])
    hg.release()


def test_device_form_on_a_stream_equals_the_host_form(H, oracle):
    import torch
    n, d, nq, stride, k = 3000, 100, 200, 128, 20
    X, Q = _floats(n, d, 8), _floats(nq, d, 9)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)               # (an index with a graph is re-ranked like a flat one)
    cand = _ragged(np.random.default_rng(10), nq, stride, n, 0)
    want = H.Ohnsw.rerank(hg, k, Q, cand)
    _same(want, _expect_rerank(H, oracle, hg, X, Q, cand, k, 0))
    dev = torch.device("cuda", 0)
    past = cand.copy()
    past[cand < 0] = np.where(np.arange((cand < 0).sum()) % 2, n, n + 12345)    # ids past the table: skipped like padding
    Qd, Cd = torch.from_numpy(Q).to(dev), torch.from_numpy(past).to(dev)
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        H.rerank_device(hg, Qd.data_ptr(), nq, d, Cd.data_ptr(), stride, k, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    _same((ids.cpu().numpy(), dd.cpu().numpy()), want)
    # page-locked matrices of the library: read and written in place
    Qp, Cp = H.host_empty((nq, d)), H.host_empty((nq, stride), np.int32)
    out = (H.host_empty((nq, k), np.int32), H.host_empty((nq, k), np.float32))
    Qp[:], Cp[:] = Q, cand
    _same(H.Ohnsw.rerank(hg, k, Qp, Cp, out=out), want)
    hg.release()


def test_result_does_not_depend_on_the_batch(H):
    n, d, nq = 2500, 70, 96
    X, Q = _floats(n, d, 11), _floats(nq, d, 12)
    hg = H.Hgraph.flat(X)
    cand = _ragged(np.random.default_rng(13), nq, 200, n, 0)
    whole = H.Ohnsw.rerank(hg, 30, Q, cand)
    for lo, hi in ((0, 1), (1, 40), (40, 96)):
        _same(H.Ohnsw.rerank(hg, 30, Q[lo:hi], cand[lo:hi]), (whole[0][lo:hi], whole[1][lo:hi]))
    perm = np.random.default_rng(14).permutation(nq)
    got = H.Ohnsw.rerank(hg, 30, Q[perm], cand[perm])
    _same(got, (whole[0][perm], whole[1][perm]))
    hg.release()


def test_cpp_front_end_rerank(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_rerank")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rerank front-end ok" in out.stdout, out.stdout + out.stderr


# ---- the option --------------------------------------------------------------------------------------------------------------

def _refine_c(ef, k, R):
    return ef if R == -1 else min(ef, max(k, R))


def _expect_refined(oracle, g, X, Q, metric, sem, ef, k, R):
    """section "refine" of the header: (ids, distances, hops or None, real candidates per query)"""
    c = _refine_c(ef, k, R)
    sp = _space(oracle, X, metric)
    if sem == 0:
        W, _, _, hops = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=c, ef=ef, ties=oracle.TIES_CANONICAL, counters=True)
    else:
        _, W = oracle.Functor.knn_batch(g, sp, Q, ef, c, ties=oracle.TIES_CANONICAL, with_ids=True)
        hops = None
    ids = np.full((len(Q), k), -1, np.int32)
    dist = np.full((len(Q), k), _fill_value(sem), np.float32)          # (the Ohnsw calls fill NaN, the functor calls +inf)
    real = np.zeros(len(Q), np.uint32)
    for q in range(len(Q)):
        ids0 = W[q][W[q] >= 0].astype(np.int64)
        real[q] = len(ids0)
        key, dq = _tree16(oracle, X, Q[q], ids0, metric)
        o = np.lexsort((ids0, key))[:k]
        ids[q, :len(o)] = ids0[o]
        dist[q, :len(o)] = dq[o]
    return ids, dist, hops, real


def _search(H, hg, Q, ef, k, sem):
    return H._search(hg, Q, ef, k, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)


CASES = ((16, 5, 5), (100, 10, 20), (100, 10, -1), (300, 10, 64), (300, 100, 1))


@pytest.mark.parametrize("d", [20, 96, 100, 128, 256, 300])
@pytest.mark.parametrize("metric", [0, 1])
def test_refined_half_row_search_equals_its_definition(H, oracle, d, metric):
    n, nq, M, efc = (1200, 32, 8, 40) if d > 256 else (3000, 48, 12, 60)
    X = _unit(n, d, 10 + d) if metric else _floats(n, d, 10 + d)
    Q = _unit(nq, d, 20 + d) if metric else _floats(nq, d, 20 + d)
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=3, metric=metric)
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_HALF
    g = _graph(oracle, hg)
    for sem in (0, 1):
        for ef, k, R in CASES:
            ctx = "d %d metric %d rule %d ef %d k %d R %d" % (d, metric, sem, ef, k, R)
            hg.set_option("refine", 0)
            _, _, nd0, nh0 = _search(H, hg, Q, ef, k, sem)
            hg.set_option("refine", R)
            ids, dist, nd, nh = _search(H, hg, Q, ef, k, sem)
            wi, wd, hops, real = _expect_refined(oracle, g, X, Q, metric, sem, ef, k, R)
            _same((ids, dist), (wi, wd), ctx)
            np.testing.assert_array_equal(nh, nh0, err_msg=ctx)
            if hops is not None:
                np.testing.assert_array_equal(nh, hops, err_msg=ctx)
            np.testing.assert_array_equal(nd, nd0 + real, err_msg=ctx)
            # every returned distance is the distance to its own vector
            np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32), err_msg=ctx)
    hg.release()


def test_same_answer_through_every_entry_point(H, oracle):
    import torch
    n0, m, d, nq, ef, k, R = 3000, 1000, 64, 300, 100, 10, 30
    X, Q = _floats(n0 + m, d, 60), _floats(nq, d, 61)
    hg = H.Ohnsw.build_batch_bigarray(X[:n0], 12, 60, seed=8)
    hg.set_option("half_rows", 1)
    hg.set_option("refine", R)
    H.Ohnsw.insert_batch(hg, X[n0:], 12, 60, seed=8)                 # the insert keeps both settings
    assert hg.n == n0 + m and hg.info().row_format == ROWS_HALF
    g = _graph(oracle, hg)
    wi, wd, hops, real = _expect_refined(oracle, g, X, Q, 0, 0, ef, k, R)
    assert (wi[:, :k] >= n0).any()                                   # inserted vectors among the answers
    for order in (0, 1):
        hg.set_option("order_queries", order)
        ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
        _same((ids, dist), (wi, wd), "host order %d" % order)
        np.testing.assert_array_equal(nh, hops)
        # device pointers on a torch stream, counters included
        dev = torch.device("cuda", 0)
        Qd = torch.from_numpy(Q).to(dev)
        di = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
        dnd = torch.zeros(nq, dtype=torch.int32, device=dev)
        dnh = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            H.search_batch_device(hg, Qd.data_ptr(), nq, d, ef, k, di.data_ptr(), dd.data_ptr(), dnd.data_ptr(), dnh.data_ptr(), 0, st.cuda_stream)
        st.synchronize()
        _same((di.cpu().numpy(), dd.cpu().numpy()), (wi, wd), "device order %d" % order)
        np.testing.assert_array_equal(dnd.cpu().numpy().view(np.uint32), nd)
        np.testing.assert_array_equal(dnh.cpu().numpy().view(np.uint32), nh)
        # host queries in, device results out
        di.zero_(); dd.zero_()
        keep = H.search_batch_h2d(hg, Q, ef, k, di.data_ptr(), dd.data_ptr())
        torch.cuda.synchronize()
        _same((di.cpu().numpy(), dd.cpu().numpy()), (wi, wd), "h2d order %d" % order)
        del keep
        # two requests in flight, waited for in the other order
        r1, r2 = H.submit(hg, Q[:170], ef, k), H.submit(hg, Q[170:], ef, k)
        b = r2.wait(counters=True)
        a = r1.wait(counters=True)
        _same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), (wi, wd), "submit order %d" % order)
        np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), nd)
        # registered host matrices, read and written in place
        Qp = H.host_empty((nq, d))
        Qp[:] = Q
        out = (H.host_empty((nq, k), np.int32), H.host_empty((nq, k), np.float32))
        _same(H.Ohnsw.knn_batch_bigarray(hg, k, Qp, ef=ef, out=out), (wi, wd), "registered order %d" % order)
    # the single-query form
    for q in (0, 7, 299):
        one = H.Ohnsw.knn(hg, k, Q[q], ef=ef)
        assert [i for i, _ in one] == list(wi[q]) and [np.float32(x) for _, x in one] == list(wd[q])
    hg.release()


@pytest.mark.parametrize("order", [0, 1])
def test_refine_runs_behind_the_tie_overflow_repair(H, oracle, order):
    """the construction of test_gpu_parity.py::test_tie_overflow_beyond_lds_stack (more than 64 tied, evicted, still expandable
    entries): the host call's re-run and the device entry point's slab are re-ranked, not the flagged first answer"""
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
    hg = H.Hgraph(X, deg0, nbr0, entry_point=0, max_degree=32)
    hg.set_option("half_rows", 1)
    hg.set_option("order_queries", order)
    assert hg.info().row_format == ROWS_HALF
    Q = np.array([[0.0], [0.05], [-0.3]], np.float32)
    dev = torch.device("cuda", 0)
    for R in (20, -1):
        hg.set_option("refine", 0)
        nd0 = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=128, counters=True)[2]
        hg.set_option("refine", R)
        wi, wd, hops, real = _expect_refined(oracle, g, X, Q, 0, 0, 128, 10, R)
        assert 228 in wi[0]                         # the node reachable only through an entry of the overflowed tie list
        got = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=128, counters=True)
        _same(got[:2], (wi, wd), "host R %d" % R)
        np.testing.assert_array_equal(got[3], hops)
        np.testing.assert_array_equal(got[2], nd0 + real)
        a = H.submit(hg, Q, 128, 10).wait(counters=True)
        _same(a[:2], (wi, wd), "submit R %d" % R)
        np.testing.assert_array_equal(a[2], nd0 + real)
        Qd = torch.from_numpy(Q).to(dev)
        ids = torch.empty((3, 10), dtype=torch.int32, device=dev)
        dd = torch.empty((3, 10), dtype=torch.float32, device=dev)
        st = torch.zeros(3, dtype=torch.int32, device=dev)
        hg.set_option("device_fallback_slab_bytes", 4 * n * 8)
        H.search_batch_device(hg, Qd.data_ptr(), 3, 1, 128, 10, ids.data_ptr(), dd.data_ptr(), 0, 0, st.data_ptr(), 0)
        torch.cuda.synchronize()
        assert ((st.cpu().numpy() & 1) == 0).all()
        _same((ids.cpu().numpy(), dd.cpu().numpy()), (wi, wd), "slab R %d" % R)
        hg.set_option("device_fallback_slab_bytes", 0)
    hg.release()


def test_no_op_on_rows_that_are_exact_already(H):
    rng = np.random.default_rng(4)
    sets = ((rng.integers(0, 256, size=(2000, 64)).astype(np.float32), ROWS_BYTES),
            (_floats(3000, 128, 31), ROWS_F32), (_floats(3000, 100, 32), ROWS_SPLIT))
    for X, rows in sets:
        hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=2)
        assert hg.info().row_format == rows
        Q = X[:50] + np.float32(0.25)
        want = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
        for R in (0, 20, -1):
            hg.set_option("refine", R)
            got = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
            _same(got[:2], want[:2], "rows %d R %d" % (rows, R))
            np.testing.assert_array_equal(got[2], want[2])
            np.testing.assert_array_equal(got[3], want[3])
            # "the k farthest of W" is only refused while refine is active
            H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
        hg.release()


def test_option_states(H, oracle):
    n, d = 3000, 96
    X, Q = _floats(n, d, 50), _floats(40, d, 51)
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=6)
    g = _graph(oracle, hg)
    for bad in (1025, -2, 5000, -100):
        with pytest.raises(H.InvalidArgument, match="refine"):
            hg.set_option("refine", bad)
    f32 = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)
    hg.set_option("refine", 5)                      # set before half rows: nothing yet ...
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), f32)
    hg.set_option("half_rows", 1)                   # ... in effect from here on (R = 5 < k: the k first of W re-ranked)
    wi, wd, _, _ = _expect_refined(oracle, g, X, Q, 0, 0, 100, 10, 5)
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), (wi, wd))
    with pytest.raises(H.InvalidArgument, match="refine"):
        H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    for R in (-1, 1024):
        hg.set_option("refine", R)
        wi, wd, _, _ = _expect_refined(oracle, g, X, Q, 0, 0, 100, 10, R)
        _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), (wi, wd), "R %d" % R)
    hg.set_option("refine", 0)                      # off: the half-row search of before
    oi, od = oracle.Ohnsw.knn_batch_bigarray(g, _space(oracle, X, 0), Q, k=10, ef=100, ties=oracle.TIES_CANONICAL)
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), (oi, od))
    H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    hg.set_option("half_rows", 0)
    hg.set_option("refine", -1)
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), f32)
    hg.release()


def _clustered(n, d, centers, seed):
    """L2: Gaussian blobs"""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d)).astype(np.float32) * 4
    return (C[rng.integers(0, centers, n)] + rng.normal(size=(n, d)).astype(np.float32)).astype(np.float32)


def _clustered_unit(n, d, centers, seed, spread=1.5):
    """IP: unit vectors around `centers` directions"""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = C[rng.integers(0, centers, n)] + spread * rng.normal(size=(n, d)) / d ** 0.5
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("d,metric", [(96, 0), (100, 1)])
def test_refining_never_lowers_a_query_recall(H, d, metric):
    """A true neighbour inside the candidate set is among that set's k nearest under the (distance, id) order the exact scan
    uses: for EVERY query the refined answer holds at least as many true neighbours as the unrefined one, and with R = -1
    exactly those of W."""
    n, nq, k, ef = 50000, 1000, 10, 64
    X = _clustered_unit(n + nq, d, 256, 70 + d) if metric else _clustered(n + nq, d, 256, 70 + d)
    X, Q = X[:n], X[n:]
    hg = H.Ohnsw.build_batch_bigarray(X, 16, 100, seed=1, metric=metric)
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]
    hg.set_option("half_rows", 1)

    def hits(ids):
        return np.array([len(set(a) & set(b)) for a, b in zip(ids, truth)])
    plain = hits(H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0])
    W = H.Ohnsw.knn_batch_bigarray(hg, ef, Q, ef=ef)[0]             # all of W, unrefined
    for R in (2 * k, 4 * k, -1):
        hg.set_option("refine", R)
        refined = hits(H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0])
        print("d %d metric %d R %d: recall@%d %.4f -> %.4f" % (d, metric, R, k, plain.mean() / k, refined.mean() / k))
        assert (refined >= plain).all(), (R, np.flatnonzero(refined < plain)[:10])
        if R == -1:
            np.testing.assert_array_equal(refined, hits(W))
        hg.set_option("refine", 0)
    hg.release()
