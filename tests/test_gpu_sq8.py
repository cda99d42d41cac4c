"""Option "sq8_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_sq8.hip): float vectors searched through 8-bit codes under ONE affine map, by
the byte-row kernels, and answered from the float32 rows.

The definition the tests hold it to (include/hnsw_mi355x.h): B, lo, s come from the quantiser restated in numpy below; the walk
is the oracle's search over B.astype(float32) with Q' = (Q - lo) / s (L2) or Q (inner product) and k := c = min(ef, max(k, R)),
R = option "refine" (0: c = k, -1: c = ef); its members are re-ranked over X under (TREE16 distance key, id) and the first k
returned with the bits of hnsw_distance_batch.  out_nhops is the walk's, out_ndist the walk's plus c.

The oracle's batched functor search reports no hop counts and neither oracle search reports the kernel's evaluation count (the
LDS visited cache re-evaluates forgotten nodes): hops and evaluations of the walk are held against the byte-row search of a twin
index -- the same graph over B.astype(float32), which is byte-valued and gets the lossless byte rows -- asked for k := c with Q'.
That is the same kernel over the same bytes; for the Ohnsw rule the hops are held against the oracle's as well."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8 = 0, 2, 3, 4, 5


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


# ---- the quantiser, restated ---------------------------------------------------------------------------------------------------

def _quantise(X):
    """(B uint8 [n][d], lo, s): float32 operations, round to nearest even"""
    X = np.asarray(X, np.float32)
    zero = np.float32(0)
    lo, hi = np.float32(X.min()) + zero, np.float32(X.max()) + zero
    s = np.float32(1) if hi == lo else np.float32(np.float32(hi - lo) / np.float32(255))
    code = np.rint((X - lo) / s)
    assert code.dtype == np.float32
    return np.minimum(np.float32(255), np.maximum(zero, code)).astype(np.uint8), lo, s


def _to_code_space(Q, lo, s, metric):
    Q = np.asarray(Q, np.float32)
    return Q if metric else ((Q - lo) / s).astype(np.float32)


def _nch(d):
    per_lane = ((d + 3) // 4 + 15) // 16
    return next(c for c in (1, 2, 4, 8, 16) if per_lane <= c)


def _floats(n, d, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(n, d))).astype(np.float32)


def _unit(n, d, seed):
    X = _floats(n, d, seed, 1.0)
    return X / np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)


def _graph(oracle, hg):
    hg.export()
    return oracle.Graph(hg.n, hg.entry_point, hg.deg0, hg.nbr0, hg.upper)


def _fill_value(fill):
    return np.float32(np.nan) if fill == 0 else np.float32(np.inf)


def _same(got, want, ctx=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx)


def _c(ef, k, R):
    return ef if R == -1 else min(ef, max(k, R))


def _search(H, hg, Q, ef, k, sem):
    return H._search(hg, Q, ef, k, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)


class Expect:
    """the definition for one (graph, X, Q, metric): walks and TREE16 keys are computed once and shared between the cases"""

    def __init__(self, oracle, g, X, Q, metric):
        self.o, self.g, self.X, self.Q, self.metric = oracle, g, np.asarray(X, np.float32), np.asarray(Q, np.float32), metric
        self.B, self.lo, self.s = _quantise(self.X)
        self.B32 = self.B.astype(np.float32)
        self.Qp = _to_code_space(self.Q, self.lo, self.s, metric)
        self.space = (oracle.Space.ip if metric else oracle.Space.l2)(self.B32, arith=oracle.TREE16)
        self._walks, self._keys = {}, {}

    def walk(self, sem, ef, c):
        """(W [nq][c], hops or None)"""
        key = (sem, ef, c)
        if key not in self._walks:
            o = self.o
            if sem == 0:
                W, _, _, hops = o.Ohnsw.knn_batch_bigarray(self.g, self.space, self.Qp, k=c, ef=ef, ties=o.TIES_CANONICAL, counters=True)
            else:
                _, W = o.Functor.knn_batch(self.g, self.space, self.Qp, ef, c, ties=o.TIES_CANONICAL, with_ids=True)
                hops = None
            self._walks[key] = (W, hops)
        return self._walks[key]

    def key(self, q, j):
        """(order key, distance) of the pair (Q[q], X[j]) over the float32 rows, in the kernels' summation order"""
        if (q, j) not in self._keys:
            if self.metric:
                dist = np.float32(1.0) - np.float32(self.o.dot_tree16(self.X[j], self.Q[q]))
                self._keys[(q, j)] = (dist, dist)
            else:
                sq = np.float32(self.o.l2sq_tree16(self.X[j], self.Q[q]))
                self._keys[(q, j)] = (sq, np.float32(np.sqrt(np.float64(sq))))
        return self._keys[(q, j)]

    def answer(self, sem, ef, k, R):
        """(ids, distances, hops or None, members of W re-ranked per query)"""
        W, hops = self.walk(sem, ef, _c(ef, k, R))
        nq = len(self.Q)
        ids = np.full((nq, k), -1, np.int32)
        dist = np.full((nq, k), _fill_value(sem), np.float32)          # (the Ohnsw calls fill NaN, the functor calls +inf)
        real = np.zeros(nq, np.uint32)
        for q in range(nq):
            ids0 = W[q][W[q] >= 0].astype(np.int64)
            real[q] = len(ids0)
            kd = [self.key(q, int(j)) for j in ids0]
            o = np.lexsort((ids0, np.array([a for a, _ in kd], np.float32)))[:k]
            ids[q, :len(o)] = ids0[o]
            dist[q, :len(o)] = np.array([b for _, b in kd], np.float32)[o]
        return ids, dist, hops, real


def _byte_twin(H, hg, e, metric):
    """the same graph over the codes as float32 vectors: byte-valued data, searched from the lossless byte rows"""
    twin = H.Hgraph(e.B32, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree, metric=metric)
    assert twin.info().row_format == ROWS_BYTES
    return twin


# ---- 1. the quantiser's bits ---------------------------------------------------------------------------------------------------

def _check_copy(hg, X):
    B, lo, s = _quantise(X)
    glo, gs = hg.sq8_params()
    assert glo.dtype == np.float32 and glo.view(np.uint32) == lo.view(np.uint32) and gs.view(np.uint32) == s.view(np.uint32), (glo, lo, gs, s)
    codes = hg.sq8_codes()
    assert codes.shape == X.shape and codes.dtype == np.uint8                 # [n][d]: the padding of the lane grid stays behind
    np.testing.assert_array_equal(codes, B)
    return B, lo, s


@pytest.mark.parametrize("d", [20, 100, 257])
def test_quantiser_bits(H, d):
    n = 700
    X = _floats(n, d, 40 + d)                                                  # signed
    hg = H.Hgraph.flat(X)
    before = hg.info().device_bytes
    hg.set_option("sq8_rows", 1)
    B, lo, s = _check_copy(hg, X)
    assert lo < 0 < lo + np.float32(255) * s and B.min() == 0 and B.max() == 255
    assert hg.info().device_bytes - before == n * 64 * _nch(d)
    hg.release()


def test_quantiser_edge_tables(H):
    # a constant table: s = 1, every code 0
    X = np.full((300, 20), np.float32(-2.75))
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_rows", 1)
    B, lo, s = _check_copy(hg, X)
    assert s == 1 and lo == np.float32(-2.75) and not B.any()
    hg.release()
    # lo = 0, s = 1 and values j + 0.5: exact ties, which go to the even code (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ..., 254.5 -> 254)
    rng = np.random.default_rng(5)
    X = (rng.integers(0, 255, size=(400, 33)) + 0.5).astype(np.float32)
    X[0, 0], X[1, 1] = 0.0, 255.0
    X[2, :8] = np.array([0.5, 1.5, 2.5, 3.5, 252.5, 253.5, 254.5, 127.5], np.float32)
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_rows", 1)
    B, lo, s = _check_copy(hg, X)
    assert lo == 0 and s == 1
    assert list(B[2, :8]) == [0, 2, 2, 4, 252, 254, 254, 128] and not (B[2:] % 2).any()
    hg.release()
    # a negative zero as the minimum counts as +0
    X = np.abs(_floats(200, 12, 6))
    X[7, 3] = np.float32(-0.0)
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_rows", 1)
    _check_copy(hg, X)
    assert hg.sq8_params()[0].view(np.uint32) == 0
    hg.release()


# ---- 2. walk and re-rank parity ------------------------------------------------------------------------------------------------

EFS, KS, RS = (8, 64, 100, 200), (1, 10), (0, 32, -1)


@pytest.mark.parametrize("d", [20, 100, 128, 257, 1024])
@pytest.mark.parametrize("metric", [0, 1])
def test_search_equals_its_definition(H, oracle, d, metric):
    n, nq, M, efc = (600, 10, 6, 30) if d > 256 else (2000, 16, 12, 48)
    X = _unit(n, d, 10 + d) if metric else _floats(n, d, 10 + d)
    Q = _unit(nq, d, 20 + d) if metric else _floats(nq, d, 20 + d)
    hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=3, metric=metric)
    g = _graph(oracle, hg)
    e = Expect(oracle, g, X, Q, metric)
    twin = _byte_twin(H, hg, e, metric)
    hg.set_option("sq8_rows", 1)
    assert hg.info().row_format == ROWS_SQ8 and hg.row_bytes() == d
    _check_copy(hg, X)
    walks = {}
    for sem in (0, 1):
        for ef in EFS:
            for k in KS:
                if k > ef:                                                     # (not a search: k <= ef is required of every rows)
                    with pytest.raises(H.InvalidArgument):
                        _search(H, hg, Q, ef, k, sem)
                    continue
                for R in RS:
                    ctx = "d %d metric %d rule %d ef %d k %d R %d" % (d, metric, sem, ef, k, R)
                    c = _c(ef, k, R)
                    hg.set_option("refine", R)
                    ids, dist, nd, nh = _search(H, hg, Q, ef, k, sem)
                    wi, wd, hops, real = e.answer(sem, ef, k, R)
                    _same((ids, dist), (wi, wd), ctx)
                    if (sem, ef, c) not in walks:                              # the byte path's walk: the same kernel over the same bytes
                        walks[(sem, ef, c)] = _search(H, twin, e.Qp, ef, c, sem)
                    bi, _, bnd, bnh = walks[(sem, ef, c)]
                    np.testing.assert_array_equal(bi, e.walk(sem, ef, c)[0], err_msg=ctx)
                    np.testing.assert_array_equal(nh, bnh, err_msg=ctx)
                    if hops is not None:
                        np.testing.assert_array_equal(nh, hops, err_msg=ctx)
                    np.testing.assert_array_equal(nd, bnd + real, err_msg=ctx)
                    assert (real == c).all() or n < c, ctx                    # (a connected graph of n >= c nodes fills W)
                    # every returned distance is the distance to its own vector
                    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32), err_msg=ctx)
    twin.release()
    hg.release()


# ---- 3. identity on byte-valued data -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,metric", [(64, 0), (100, 0), (128, 1), (300, 0)])
def test_identity_on_byte_valued_data(H, d, metric):
    """lo = 0, s = 1, B = X: the sq8 search at R = 0 is the byte-row search, followed by a re-rank of its own k answers"""
    n, nq, ef, k = 2000, 40, 64, 10
    rng = np.random.default_rng(d)
    X = rng.integers(0, 256, size=(n, d)).astype(np.float32)
    X[0, 0], X[0, 1] = 0.0, 255.0
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 48, seed=2, metric=metric)
    assert hg.info().row_format == ROWS_BYTES
    Qi = rng.integers(0, 256, size=(nq, d)).astype(np.float32)                 # byte-valued: the integer path (d <= 256)
    Qf = (Qi + rng.random(size=(nq, d))).astype(np.float32)                    # fractional: the float path
    want = [H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True) for Q in (Qi, Qf)]
    hg.set_option("byte_rows", 0)
    hg.set_option("sq8_rows", 1)
    assert hg.info().row_format == ROWS_SQ8
    lo, s = hg.sq8_params()
    assert lo == 0 and s == 1
    np.testing.assert_array_equal(hg.sq8_codes(), X.astype(np.uint8))
    for Q, w in zip((Qi, Qf), want):
        got = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
        _same(got[:2], w[:2])
        np.testing.assert_array_equal(got[2], w[2] + k)
        np.testing.assert_array_equal(got[3], w[3])
    hg.release()


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
def test_tie_overflow_is_repaired_before_the_rerank(H, oracle, order):
    """the construction of test_gpu_parity.py::test_tie_overflow_beyond_lds_stack in dimension 0 of a d = 4, n = 2000 table whose
    values lie on few levels (the other nodes have no links): in code space the chain 9.00, 8.99, ... collapses onto 14 codes and the
    127 nodes at 10.0 stay tied, so more than 64 tied, evicted, still expandable entries pile up"""
    import torch
    n, m = 2000, 229
    pos = np.zeros(m, np.float32)
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
    X = np.zeros((n, 4), np.float32)
    X[:m, 0] = pos
    X[m:] = 5.0 * np.random.default_rng(1).integers(0, 5, size=(n - m, 4))     # levels 0, 5, 10, 15, 20
    g = oracle.Graph(n, 0, deg0, nbr0)
    hg = H.Hgraph(X, deg0, nbr0, entry_point=0, max_degree=32)
    hg.set_option("sq8_rows", 1)
    hg.set_option("order_queries", order)
    assert hg.info().row_format == ROWS_SQ8
    Q = np.array([[0.0, 0, 0, 0], [0.05, 0, 0, 0], [-0.3, 0, 0, 0]], np.float32)
    e = Expect(oracle, g, X, Q, 0)
    assert len(np.unique(e.B[128:228, 0])) < 20
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    for R in (0, 20, -1):
        hg.set_option("refine", R)
        wi, wd, hops, real = e.answer(0, 128, 10, R)
        assert 228 in wi[0]                         # the node reachable only through an entry of the overflowed tie list
        host = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=128, counters=True)
        _same(host[:2], (wi, wd), "host R %d" % R)
        np.testing.assert_array_equal(host[3], hops)
        a = H.submit(hg, Q, 128, 10).wait(counters=True)
        _same(a[:2], host[:2], "submit R %d" % R)
        np.testing.assert_array_equal(a[2], host[2])
        ids = torch.empty((3, 10), dtype=torch.int32, device=dev)
        dd = torch.empty((3, 10), dtype=torch.float32, device=dev)
        st = torch.zeros(3, dtype=torch.int32, device=dev)
        H.search_batch_device(hg, Qd.data_ptr(), 3, 4, 128, 10, ids.data_ptr(), dd.data_ptr(), 0, 0, st.data_ptr(), 0)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() & 1).any()         # the list did overflow its 64 LDS slots
        hg.set_option("device_fallback_slab_bytes", 4 * n * 8)
        H.search_batch_device(hg, Qd.data_ptr(), 3, 4, 128, 10, ids.data_ptr(), dd.data_ptr(), 0, 0, st.data_ptr(), 0)
        torch.cuda.synchronize()
        assert ((st.cpu().numpy() & 1) == 0).all()
        _same((ids.cpu().numpy(), dd.cpu().numpy()), host[:2], "slab R %d" % R)
        hg.set_option("device_fallback_slab_bytes", 0)
    hg.release()


# ---- 5. one answer through every form ------------------------------------------------------------------------------------------

def test_same_answer_through_every_entry_point(H, oracle):
    import torch
    n, d, nq, ef, k, R = 3000, 100, 300, 100, 10, 30
    X, Q = _floats(n, d, 60), _floats(nq, d, 61)
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 48, seed=8)
    g = _graph(oracle, hg)
    hg.set_option("sq8_rows", 1)
    hg.set_option("refine", R)
    wi, wd, hops, real = Expect(oracle, g, X, Q, 0).answer(0, ef, k, R)
    dev = torch.device("cuda", 0)
    for order in (0, 1):
        hg.set_option("order_queries", order)
        ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
        _same((ids, dist), (wi, wd), "host order %d" % order)
        np.testing.assert_array_equal(nh, hops)
        # a host matrix whose rows are wider than d and not 16-byte aligned
        wide = np.zeros((nq, d + 3), np.float32)
        wide[:, :d] = Q
        _same(H.Ohnsw.knn_batch_bigarray(hg, k, wide[:, :d], ef=ef), (wi, wd), "strided order %d" % order)
        # device pointers on a torch stream, counters included
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
        # host queries in, device results out: from ordinary and from registered memory
        Qp = H.host_empty((nq, d))
        Qp[:] = Q
        for src in (Q, Qp):
            di.zero_(); dd.zero_()
            keep = H.search_batch_h2d(hg, src, ef, k, di.data_ptr(), dd.data_ptr())
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
        out = (H.host_empty((nq, k), np.int32), H.host_empty((nq, k), np.float32))
        _same(H.Ohnsw.knn_batch_bigarray(hg, k, Qp, ef=ef, out=out), (wi, wd), "registered order %d" % order)
    # the single-query form
    for q in (0, 7, 299):
        one = H.Ohnsw.knn(hg, k, Q[q], ef=ef)
        assert [i for i, _ in one] == list(wi[q]) and [np.float32(x) for _, x in one] == list(wd[q])
    # two replicas on one device, the option set through each replica's handle
    m = H.MultiHgraph(hg, [0, 0])
    m.set_option("sq8_rows", 1)
    m.set_option("refine", R)
    mi, md, mnd, mnh = m.knn_batch_bigarray(k, Q, ef=ef, counters=True)
    _same((mi, md), (wi, wd), "multi")
    np.testing.assert_array_equal(mnd, nd)
    np.testing.assert_array_equal(mnh, nh)
    m.release()
    hg.release()


# ---- 6. option algebra ---------------------------------------------------------------------------------------------------------

def test_option_states(H, oracle, tmp_path):
    n, d = 2000, 100
    X, Q = _floats(n, d, 50), _floats(30, d, 51)
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 48, seed=6)
    g = _graph(oracle, hg)
    e = Expect(oracle, g, X, Q, 0)
    rows0, bytes0 = hg.info().row_format, hg.info().device_bytes
    assert rows0 == ROWS_SPLIT and hg.row_bytes() == 4 * d
    before = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    nearest_k = H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    with pytest.raises(H.InvalidArgument, match="sq8"):
        hg.sq8_params()                             # no copy yet
    with pytest.raises(H.InvalidArgument, match="sq8"):
        hg.sq8_codes()
    hg.set_option("sq8_rows", 1)
    copy = n * 64 * _nch(d)
    assert hg.info().row_format == ROWS_SQ8 and hg.row_bytes() == d and hg.info().device_bytes == bytes0 + copy
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), e.answer(0, 100, 10, 0)[:2])
    with pytest.raises(H.InvalidArgument, match="sq8_rows"):
        H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    with pytest.raises(H.InvalidArgument, match="sq8_rows"):
        hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_SQ8
    hg.set_option("sq8_rows", 1)                    # again: nothing changes
    assert hg.info().device_bytes == bytes0 + copy
    # 0: the previous rows again, the copy kept; results as if the option had never been set
    hg.set_option("sq8_rows", 0)
    assert hg.info().row_format == rows0 and hg.row_bytes() == 4 * d and hg.info().device_bytes == bytes0 + copy
    hg.sq8_params()
    after = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    _same(after[:2], before[:2])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    _same(H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K), nearest_k)
    # refused while half rows are on
    hg.set_option("half_rows", 1)
    with pytest.raises(H.InvalidArgument, match="half_rows"):
        hg.set_option("sq8_rows", 1)
    assert hg.info().row_format == ROWS_HALF
    hg.set_option("half_rows", -1)
    # -1: ... and the copy freed
    hg.set_option("sq8_rows", 1)
    hg.set_option("sq8_rows", -1)
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0
    with pytest.raises(H.InvalidArgument, match="sq8"):
        hg.sq8_params()
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), before[:2])
    # not saved
    hg.set_option("sq8_rows", 1)
    path = os.path.join(str(tmp_path), "index.hnsw")
    hg.save(path)
    back = H.Hgraph.load(path)
    assert back.info().row_format == rows0
    with pytest.raises(H.InvalidArgument, match="sq8"):
        back.sq8_params()
    _same(H.Ohnsw.knn_batch_bigarray(back, 10, Q, ef=100), before[:2])
    back.release()
    hg.release()


def test_refused_with_byte_rows_in_use(H):
    X = np.random.default_rng(3).integers(0, 256, size=(800, 64)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    assert hg.info().row_format == ROWS_BYTES
    bytes0 = hg.info().device_bytes
    with pytest.raises(H.InvalidArgument, match="byte rows"):
        hg.set_option("sq8_rows", 1)
    assert hg.info().row_format == ROWS_BYTES and hg.info().device_bytes == bytes0
    assert H.load().hnsw_index_set_option(hg.handle, b"sq8_rows", 1) == H.ERR_BAD_ARG
    hg.release()


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "range"])
def test_values_that_cannot_be_quantised_leave_the_index_unchanged(H, bad):
    n, d = 900, 40
    X, Q = _floats(n, d, 70), _floats(20, d, 71)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    hg.export()
    Y = X.copy()
    if bad == "range":                               # finite values whose max - min overflows float32
        Y[5, 7], Y[n - 1, d - 1] = np.float32(3e38), np.float32(-3e38)
    else:
        Y[n - 1, d - 1] = np.float32(bad)            # the last value of the table
    hb = H.Hgraph(Y, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree)
    info0 = hb.info()
    before = H.Ohnsw.knn_batch_bigarray(hb, 5, Q[:, :d], ef=40) if bad == "range" else None
    assert H.load().hnsw_index_set_option(hb.handle, b"sq8_rows", 1) == H.ERR_UNSUPPORTED
    info1 = hb.info()
    assert info1.row_format == info0.row_format and info1.device_bytes == info0.device_bytes
    with pytest.raises(H.InvalidArgument):
        hb.sq8_params()
    if before is not None:
        _same(H.Ohnsw.knn_batch_bigarray(hb, 5, Q, ef=40), before)
    hb.release()
    hg.release()


# ---- 7. what must not move -----------------------------------------------------------------------------------------------------

def test_everything_but_the_knn_searches_keeps_reading_the_float32_rows(H):
    n, d, nq = 2000, 100, 24
    X, Q = _floats(n, d, 80), _floats(nq, d, 81)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=4)
    hg.export()
    links = (hg.deg0.copy(), hg.nbr0.copy(), [(a.copy(), b.copy(), c.copy()) for a, b, c in hg.upper])
    cand = np.random.default_rng(9).integers(0, n, size=(nq, 50)).astype(np.int32)
    starts = [[int(hg.entry_point)]] * nq

    def operators():
        return (H.Ohnsw.brute_force_knn(hg, 10, Q), (cand, H.Ohnsw.distance_l2(hg, Q, cand)), H.Ohnsw.rerank(hg, 10, Q, cand),
                H.Ohnsw.search_k(hg, 0, starts, Q, 10, ef=40), H.Ohnsw.search_one(hg, hg.max_layer, hg.entry_point, Q, with_distance=True))
    before = operators()
    hg.set_option("sq8_rows", 1)
    hg.set_option("refine", 32)
    assert hg.info().row_format == ROWS_SQ8
    after = operators()
    for a, b in zip(after[:3], before[:3]):
        _same(a, b)
    assert after[3] == before[3]                                               # [(node, distance)] lists
    np.testing.assert_array_equal(after[4][0], before[4][0])
    np.testing.assert_array_equal(after[4][1].view(np.uint32), before[4][1].view(np.uint32))
    hg.export()
    np.testing.assert_array_equal(hg.deg0, links[0])
    np.testing.assert_array_equal(hg.nbr0, links[1])
    # a build does not depend on the option (it is a handle's, and the builder reads float32 rows): an insert under sq8 gives the
    # links the same insert gives without it
    plain = H.Ohnsw.build_batch_bigarray(X[:1500], 10, 40, seed=4)
    under = H.Ohnsw.build_batch_bigarray(X[:1500], 10, 40, seed=4)
    under.set_option("sq8_rows", 1)
    for h in (plain, under):
        H.Ohnsw.insert_batch(h, X[1500:], 10, 40, seed=4)
        h.export()
    np.testing.assert_array_equal(under.deg0, plain.deg0)
    np.testing.assert_array_equal(under.nbr0, plain.nbr0)
    assert len(under.upper) == len(plain.upper)
    for a, b in zip(under.upper, plain.upper):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    for h in (plain, under, hg):
        h.release()


# ---- 8. insert -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1])
def test_insert_quantises_the_grown_table_again(H, oracle, metric):
    n0, m, d, nq = 1500, 500, 72, 24
    X = _floats(n0 + m, d, 90)
    X[n0:] *= np.float32(2.5)                                                  # the new vectors widen the range
    Q = X[n0:n0 + nq] + _floats(nq, d, 91, 0.5)                                # near the vectors that will be inserted
    hg = H.Ohnsw.build_batch_bigarray(X[:n0], 10, 40, seed=5, metric=metric)
    hg.set_option("sq8_rows", 1)
    hg.set_option("refine", 20)
    _, lo0, s0 = _check_copy(hg, X[:n0])
    H.Ohnsw.insert_batch(hg, X[n0:], 10, 40, seed=5)
    assert hg.n == n0 + m and hg.info().row_format == ROWS_SQ8
    _, lo1, s1 = _check_copy(hg, X)
    assert lo1 < lo0 and s1 > s0
    g = _graph(oracle, hg)
    e = Expect(oracle, g, X, Q, metric)
    for sem, ef, k in ((0, 64, 10), (1, 100, 5)):
        ids, dist, nd, nh = _search(H, hg, Q, ef, k, sem)
        wi, wd, hops, real = e.answer(sem, ef, k, 20)
        _same((ids, dist), (wi, wd), "rule %d" % sem)
        if hops is not None:
            np.testing.assert_array_equal(nh, hops)
    assert (e.answer(0, 64, 10, 20)[0] >= n0).any()                            # inserted vectors among the answers
    # a new vector that is not finite: nothing inserted, codes, parameters and results as before
    codes, params = hg.sq8_codes(), hg.sq8_params()
    want = _search(H, hg, Q, 64, 10, 0)
    bytes0 = hg.info().device_bytes
    for v in (np.nan, np.inf):
        Y = _floats(40, d, 92)
        Y[39, d - 1] = v
        with pytest.raises(H.Failure, match="sq8"):
            H.Ohnsw.insert_batch(hg, Y, 10, 40, seed=5)
        inf = hg.info()
        assert inf.n == n0 + m and inf.row_format == ROWS_SQ8 and inf.device_bytes == bytes0
        np.testing.assert_array_equal(hg.sq8_codes(), codes)
        assert hg.sq8_params() == params
        got = _search(H, hg, Q, 64, 10, 0)
        _same(got[:2], want[:2])
        np.testing.assert_array_equal(got[2], want[2])
    hg.release()


# ---- 9. recall identity --------------------------------------------------------------------------------------------------------

def _clustered(n, d, centers, seed):
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d)).astype(np.float32) * 4
    return (C[rng.integers(0, centers, n)] + rng.normal(size=(n, d)).astype(np.float32)).astype(np.float32)


def _clustered_unit(n, d, centers, seed, spread=1.5):
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(centers, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = C[rng.integers(0, centers, n)] + spread * rng.normal(size=(n, d)) / d ** 0.5
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("d,metric", [(96, 0), (100, 1)])
def test_recall_is_that_of_the_candidate_set(H, d, metric):
    """The top k of a set under the exact scan's total order (distance, id) holds every true neighbour that is in the set: for
    EVERY query, recall = |truth and W_c| / k -- and W_c grows with R, so no query's recall falls as R grows."""
    n, nq, k, ef = 3000, 300, 10, 48
    X = _clustered_unit(n + nq, d, 32, 70 + d) if metric else _clustered(n + nq, d, 32, 70 + d)
    X, Q = X[:n], X[n:]
    hg = H.Ohnsw.build_batch_bigarray(X, 12, 48, seed=1, metric=metric)
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]
    hg.set_option("sq8_rows", 1)

    def hits(ids):
        return np.array([len(set(a) & set(b)) for a, b in zip(ids, truth)])
    last = np.zeros(nq, np.int64)
    for R in (0, 2 * k, 4 * k, -1):
        c = _c(ef, k, R)
        hg.set_option("refine", 0)
        Wc = H.Ohnsw.knn_batch_bigarray(hg, c, Q, ef=ef)[0]                    # the first c members of W (re-ranked: the same set)
        hg.set_option("refine", R)
        got = hits(H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0])
        print("d %d metric %d R %d: recall@%d %.4f" % (d, metric, R, k, got.mean() / k))
        np.testing.assert_array_equal(got, hits(Wc))
        assert (got >= last).all(), (R, np.flatnonzero(got < last)[:10])
        last = got
    hg.release()
