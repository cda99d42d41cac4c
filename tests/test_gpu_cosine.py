"""HNSW_METRIC_COSINE (ocaml-hnsw_amd/csrc/hnsw_cosine.hip).

The yardstick is the twin contract of include/hnsw_mi355x.h: a COSINE index over X answers every call on queries Q with exactly
the bits (ids, distances, counters, stages, graph links) of an IP index over N(X) called with N(Q), N being H.normalise.  So the
normaliser is held against float64 numpy within the bound its float32 arithmetic allows, and every call of a COSINE handle is
compared bit for bit (uint32 views) with the IP twin's -- which the existing tests hold against the oracle."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, M, EFC, SEED, NQ, K = 1500, 8, 40, 3, 64, 10
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _same(got, want, ctx=""):
    """every array of `got` is the array of `want` at its place, as bits"""
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), ctx
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, "%s [%d]" % (ctx, j)
        if a.dtype.itemsize == 4:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg="%s [%d]" % (ctx, j))


def _graph(hg):
    hg.export()
    out = [hg.entry_point, hg.max_layer, hg.deg0, hg.nbr0]
    for nodes, deg, nbr in hg.upper:
        out += [nodes, deg, nbr]
    return out


def _same_graph(hc, hi, ctx=""):
    a, b = _graph(hc), _graph(hi)
    assert a[:2] == b[:2] and len(a) == len(b), ctx
    _same(a[2:], b[2:], ctx + " graph")


# ---- 1. the normaliser ---------------------------------------------------------------------------------------------------------

def _strided(A, stride, lead=0):
    """the rows of A as a view of a larger float32 buffer: rows `stride` floats apart, the first one `lead` floats into it (junk
    between the rows, which nothing may read into the result)"""
    n, d = A.shape
    buf = np.full(lead + max(n, 1) * stride + 4, 7e30, np.float32)
    V = np.lib.stride_tricks.as_strided(buf[lead:], shape=(n, d), strides=(4 * stride, 4))
    V[...] = A
    return V


@pytest.mark.parametrize("d", [1, 3, 4, 20, 64, 100, 128, 130, 300, 960, 1024])
def test_normaliser(H, d):
    padded = (d + 15) // 16 * 16
    rng = np.random.default_rng(100 + d)
    for n in (0, 1, 65):
        A = rng.normal(size=(n, d)).astype(np.float32) * np.float32(1.0)
        A *= rng.choice(np.array([1e-3, 1.0, 1e3], np.float32), size=(n, 1))
        ref64 = A.astype(np.float64)
        nrm64 = np.sqrt((ref64 ** 2).sum(1))
        want = ref64 / nrm64[:, None] if n else ref64
        first = None
        for stride, lead in ((d, 0), (d + 3, 0), (padded, 0), (padded, 1)):          # packed, unaligned (scalar path), padded, padded off by 4 bytes
            V = _strided(A, stride, lead)
            got, norms = H.normalise(V, norms=True)
            assert got.shape == (n, d) and got.dtype == np.float32 and norms.shape == (n,)
            if n:
                # every component within (d/2 + 4) 2^-24 relative of x_i / |x|, the norm within (d/2 + 2) 2^-24: at most d roundings
                # in the sum, halved by the square root, plus the root and the scaling -- whatever the summation order
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= (d / 2 + 4) * EPS * np.abs(want)).all(), (d, n, stride, float((err / np.abs(want)).max() / EPS))
                nerr = np.abs(norms.astype(np.float64) - nrm64)
                assert (nerr <= (d / 2 + 2) * EPS * nrm64).all(), (d, n, stride, float((nerr / nrm64).max() / EPS))
            # the same vectors give the same bits at every stride and alignment
            if first is None:
                first = (got, norms)
            else:
                _same((got, norms), first, "d=%d n=%d stride=%d lead=%d" % (d, n, stride, lead))
            assert H.normalise(V).shape == (n, d)
        if n == 65:
            # ... and at every position and batch size: row 37 alone, first and last of a batch, under another stride
            v = A[37]
            _same(H.normalise(v[None, :]), first[0][37:38], "batch of 1")
            B = rng.normal(size=(65, d)).astype(np.float32)
            for pos in (0, 1, 15, 16, 63, 64):
                B2 = B.copy()
                B2[pos] = v
                _same(H.normalise(_strided(B2, d + 1))[pos], first[0][37], "position %d" % pos)


def _header_n(oracle, A):
    """N(A) and the norms by the header's own arithmetic, on the host: <x,x> on the lane grid with fused multiply-adds and the
    16-lane tree (the oracle's TREE16 dot product), one float32 square root and one float32 division per value, both IEEE"""
    A = np.ascontiguousarray(A, np.float32)
    s = np.array([oracle.dot_tree16(x, x) for x in A], np.float32)
    norm = np.sqrt(s)
    assert norm.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        out = A / norm[:, None]
    out[s == 0] = 0.0
    assert out.dtype == np.float32
    return out, norm


@pytest.mark.parametrize("d", [1, 3, 4, 20, 64, 100, 128, 130, 300, 960, 1024])
def test_normaliser_is_the_header_arithmetic_bit_for_bit(H, oracle, d):
    """The tolerance above leaves two ulp of slack and the twin tests run one kernel on both sides: only this pins the rounding
    of the square root and of the divisions, and the order of the sum."""
    rng = np.random.default_rng(300 + d)
    n = 257
    A = rng.normal(size=(n, d)).astype(np.float32) * rng.choice(np.array([1e-3, 1.0, 1e3], np.float32), size=(n, 1))
    A[5] = 0.0
    want, wnorm = _header_n(oracle, A)
    got, norms = H.normalise(A, norms=True)
    _same((got, norms), (want, wnorm), "d=%d" % d)
    if d == 1:      # one value: the norm is the correctly rounded root of the rounded square
        x = A[:, 0]
        _same(norms, np.sqrt(x * x), "d=1 norms")
    # ... and so are the rows an index stores (the 16-byte path over padded rows, a ragged tail inside a chunk when d % 4 != 0)
    hc = H.Hgraph.flat(_strided(A, d + 3), metric=H.METRIC_COSINE).to_device(0)
    try:
        _same(hc.rows(), want, "stored rows d=%d" % d)
    finally:
        hc.release()


@pytest.mark.parametrize("d", [20, 130])
def test_unaligned_queries_reach_the_kernel(H, oracle, d):
    """H.normalise stages its input in an aligned device buffer, so the kernel's value-by-value path (odd strides, a pointer that is
    no multiple of 16 bytes) and its 16-byte path over rows with a ragged last chunk are reached here: a device matrix and a
    page-locked host matrix read in place, each at (pointer, stride) = (+4 bytes, d + 3) and (aligned, a multiple of 4 above d)."""
    import torch
    n, nq, k = 300, 33, 7
    X = _floats(n, d, 400 + d) * np.float32(5.0)
    Q = _floats(nq, d, 401 + d) * np.float32(0.3)
    hc = H.Hgraph.flat(X, metric=H.METRIC_COSINE).to_device(0)
    hi = H.Hgraph.flat(_header_n(oracle, X)[0], metric=H.METRIC_IP).to_device(0)
    try:
        want = H.Ohnsw.brute_force_knn(hi, k, _header_n(oracle, Q)[0])          # the IP twin on the header's N(Q)
        _same(H.Ohnsw.brute_force_knn(hc, k, Q), want, "contiguous pageable")
        dev = torch.device("cuda", 0)
        for lead, stride in ((1, d + 3), (0, (d + 3) // 4 * 4 + 4), (0, d)):
            # a device matrix
            buf = torch.full((lead + nq * stride + 4,), 7e30, dtype=torch.float32, device=dev)
            view = torch.as_strided(buf, (nq, d), (stride, 1), lead)
            view.copy_(torch.from_numpy(Q).to(dev))
            keep = buf.clone()
            ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
            dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
            st = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            H.brute_force_device(hc, buf.data_ptr() + 4 * lead, nq, stride, k, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            _same((ids.cpu().numpy(), dd.cpu().numpy()), want, "device matrix lead=%d stride=%d" % (lead, stride))
            assert torch.equal(buf, keep)
            # a page-locked host matrix the device reads in place
            hb = H.host_empty((lead + nq * stride + 4,))
            hb[...] = 7e30
            hv = np.lib.stride_tricks.as_strided(hb[lead:], shape=(nq, d), strides=(4 * stride, 4))
            hv[...] = Q
            _same(H.Ohnsw.brute_force_knn(hc, k, hv), want, "page-locked matrix lead=%d stride=%d" % (lead, stride))
            _same(H.Ohnsw.knn_batch_bigarray(hc, 1, hv), H.Ohnsw.knn_batch_bigarray(hi, 1, _header_n(oracle, Q)[0]), "page-locked knn")
            _same(hv, Q, "the caller's matrix is not written")
    finally:
        hc.release()
        hi.release()


def test_normalise_in_place(H):
    A = _floats(40, 24, 500)
    want = H.normalise(A)
    B = A.copy()
    L = H.load()
    H._check(L.hnsw_normalise_batch(0, H._ptr(B), 40, 24, 24, H._ptr(B), 24, None))        # out may be in with the same stride
    _same(B, want, "in place")
    assert L.hnsw_normalise_batch(0, H._ptr(B), 20, 24, 24, H._ptr(B), 48, None) == H.ERR_BAD_ARG


@pytest.mark.parametrize("d", [1, 3, 20, 100, 130, 1024])
def test_normaliser_special_rows(H, d):
    A = _floats(9, d, 7)
    A[2] = 0.0                                   # a zero row: zeros, norm 0
    A[4, d // 2] = np.inf                        # an infinity, a NaN, an overflowing sum of squares: all NaN
    A[5, 0] = np.nan
    A[6] = np.float32(3e19)                      # finite values whose squares overflow float32
    A[7] = np.float32(1e-30)                     # squares underflow to 0: a zero sum of squares
    clean = A.copy()
    clean[[4, 5, 6]] = 1.0
    for stride in (d, d + 3):
        got, norms = H.normalise(_strided(A, stride), norms=True)
        assert not got[2].any() and norms[2] == 0.0 and not np.signbit(got[2]).any()
        for r in (4, 5, 6):
            assert np.isnan(got[r]).all() and not np.isfinite(norms[r]), r
        assert not got[7].any() and norms[7] == 0.0
        _same(got[[0, 1, 3, 8]], H.normalise(clean)[[0, 1, 3, 8]], "rows beside special ones")        # ... and nothing leaks into a neighbour


# ---- 2. twin equality ----------------------------------------------------------------------------------------------------------

class Pair:
    def __init__(self, H, d, n=N):
        self.d = d
        self.X = _floats(n, d, 10 + d) * np.random.default_rng(d).choice(np.array([0.01, 1.0, 50.0], np.float32), size=(n, 1))
        self.Q = _floats(NQ, d, 20 + d) * np.float32(3.0)
        self.NX, self.NQ = H.normalise(self.X), H.normalise(self.Q)
        self.hc = H.Ohnsw.build_batch_bigarray(self.X, M, EFC, seed=SEED, metric=H.METRIC_COSINE)
        self.hi = H.Ohnsw.build_batch_bigarray(self.NX, M, EFC, seed=SEED, metric=H.METRIC_IP)
        self.radius = 1.0 - 1.5 / np.sqrt(d)

    def both(self, call, ctx):
        """call(handle, queries) on the COSINE handle with Q and on the IP twin with N(Q): the same bits"""
        got, want = call(self.hc, self.Q), call(self.hi, self.NQ)
        _same(got, want, "d=%d %s" % (self.d, ctx))
        return got

    def set_option(self, name, value):
        self.hc.set_option(name, value)
        self.hi.set_option(name, value)


@pytest.fixture(scope="module", params=[20, 100, 128])
def pair(H, request):
    p = Pair(H, request.param)
    yield p
    p.hc.release()
    p.hi.release()


def test_twin_graph_and_rows(H, pair):
    assert pair.hc.info().metric == H.METRIC_COSINE == pair.hc.metric and pair.hi.info().metric == H.METRIC_IP
    _same_graph(pair.hc, pair.hi, "built")
    _same(pair.hc.rows(), pair.NX, "rows() is N(X)")
    _same(pair.hi.rows(), pair.NX, "the twin holds what it was handed")
    pick = np.array([5, 0, N - 1, 5, 77], np.int64)
    _same(pair.hc.rows(pick), pair.NX[pick], "rows(ids)")
    assert pair.hc.rows(np.zeros(0, np.int64)).shape == (0, pair.d)
    assert np.array_equal(pair.hc.vectors, pair.X)             # the host copy stays the caller's matrix
    n2 = np.sqrt((pair.hc.rows().astype(np.float64) ** 2).sum(1))
    assert np.abs(n2 - 1.0).max() <= (pair.d / 2 + 4) * EPS    # unit rows, within the normaliser's own bound


def _knn_calls(H):
    O = H.Ohnsw
    return [
        ("knn ef16", lambda h, Q: O.knn_batch_bigarray(h, K, Q, ef=16, counters=True)),
        ("knn ef200", lambda h, Q: O.knn_batch_bigarray(h, K, Q, ef=200, counters=True)),
        ("knn k=ef", lambda h, Q: O.knn_batch_bigarray(h, K, Q, counters=True)),
    ]


def _filtered_and_range_calls(H, p):
    O = H.Ohnsw
    half = np.random.default_rng(1).random(N) < 0.5
    few = np.random.default_rng(2).random(N) < 0.01
    labels = np.random.default_rng(3).integers(0, 3, N)
    which = np.random.default_rng(4).integers(0, 3, NQ).astype(np.int32)

    def each(h, Q):
        fs = h.filters_by_label(labels, 3)
        try:
            return O.knn_batch_filtered_each(h, K, Q, fs, which, ef=16, counters=True)
        finally:
            for f in fs:
                f.release()
    return [
        ("filtered 0.5", lambda h, Q: O.knn_batch_filtered(h, K, Q, half, ef=16, counters=True)),
        ("filtered 0.01", lambda h, Q: O.knn_batch_filtered(h, K, Q, few, ef=16, counters=True)),
        ("filtered each", each),
        ("range", lambda h, Q: O.range_search(h, p.radius, Q, ef=16, counters=True)),
        ("range filtered", lambda h, Q: O.range_search(h, p.radius, Q, ef=16, counters=True, filter=half)),
        ("brute range", lambda h, Q: O.brute_force_range(h, p.radius, Q, counters=True)),
        ("brute range filtered", lambda h, Q: O.brute_force_range(h, p.radius, Q, counters=True, filter=half)),
    ]


def test_twin_knn_forms(H, pair):
    import torch
    O, p = H.Ohnsw, pair
    for name, call in _knn_calls(H):
        ids = p.both(call, name)[0]
        assert (ids >= 0).all()
    # the batch in page-locked memory the device reads in place, and a strided pageable one
    for name, call in _knn_calls(H)[:2]:
        want = call(p.hi, p.NQ)
        Qp = H.host_empty((NQ, p.d))
        Qp[...] = p.Q
        _same(call(p.hc, Qp), want, name + " page-locked")
        _same(Qp, p.Q, "the caller's matrix is not written")
        _same(call(p.hc, _strided(p.Q, p.d + 3)), want, name + " strided")
    # one query (the small block), Ohnsw.knn, Ba.knn_batch (functor rule, +inf fill)
    p.both(lambda h, Q: O.knn_batch_bigarray(h, K, Q[:1], ef=16, counters=True), "one query")
    assert O.knn(p.hc, K, p.Q[3]) == O.knn(p.hi, K, p.NQ[3])
    p.both(lambda h, Q: H.Ba.knn_batch(h, Q, 32, K), "Ba.knn_batch")
    # submit / wait
    p.both(lambda h, Q: H.submit(h, Q, 16, K).wait(counters=True), "submit/wait")
    # the device forms on a stream of their own, and the host-to-device form
    dev = torch.device("cuda", 0)

    def device_knn(h, Q):
        Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        keep = Qd.clone()
        ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        nd = torch.empty(NQ, dtype=torch.int32, device=dev)
        nh = torch.empty(NQ, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        H.search_batch_device(h, Qd.data_ptr(), NQ, p.d, 16, K, ids.data_ptr(), dd.data_ptr(), nd.data_ptr(), nh.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert torch.equal(Qd, keep)                             # the caller's device matrix is not written
        return ids.cpu().numpy(), dd.cpu().numpy(), nd.cpu().numpy(), nh.cpu().numpy()

    def h2d_knn(h, Q):
        ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        keep = H.search_batch_h2d(h, Q, 16, K, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        del keep
        return ids.cpu().numpy(), dd.cpu().numpy()

    def device_scan_and_rerank(h, Q):
        Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        cand = torch.from_numpy(np.random.default_rng(5).integers(0, N, (NQ, 24)).astype(np.int32)).to(dev)
        rid = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        rdd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        H.brute_force_device(h, Qd.data_ptr(), NQ, p.d, K, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
        H.rerank_device(h, Qd.data_ptr(), NQ, p.d, cand.data_ptr(), 24, K, rid.data_ptr(), rdd.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        return ids.cpu().numpy(), dd.cpu().numpy(), rid.cpu().numpy(), rdd.cpu().numpy()

    want = O.knn_batch_bigarray(p.hi, K, p.NQ, ef=16, counters=True)
    got = p.both(device_knn, "device form")
    _same((got[0], got[1], got[2].view(np.uint32), got[3].view(np.uint32)), want, "device form against the host form")
    _same(p.both(h2d_knn, "h2d form"), want[:2], "h2d form against the host form")
    p.both(device_scan_and_rerank, "device scan and re-rank")


def test_twin_exact_and_operator_forms(H, pair):
    O, p = H.Ohnsw, pair
    pick = np.random.default_rng(6).integers(0, N, (NQ, 33)).astype(np.int32)
    dist = p.both(lambda h, Q: O.distance_l2(h, Q, pick), "distance_batch")
    p.both(lambda h, Q: O.brute_force_knn(h, K, Q), "brute_force_knn")
    p.both(lambda h, Q: O.brute_force_knn(h, 37, Q, fill=H.FILL_BA), "brute_force_knn k=37")
    cand = np.random.default_rng(7).integers(-1, N, (NQ, 40)).astype(np.int32)
    p.both(lambda h, Q: O.rerank(h, K, Q, cand), "rerank")
    # what the numbers mean: 1 - cos within (2 d + 9) 2^-24 -- the normalisation error twice, the dot product's (sum |a_i b_i| <= 1
    # for unit rows) and one subtraction
    X64, Q64 = p.X.astype(np.float64), p.Q.astype(np.float64)
    cos = np.einsum("qd,qmd->qm", Q64, X64[pick]) / (np.linalg.norm(Q64, axis=1)[:, None] * np.linalg.norm(X64[pick], axis=2))
    err = np.abs(dist.astype(np.float64) - (1.0 - cos))
    assert err.max() <= (2 * p.d + 9) * EPS, (p.d, float(err.max() / EPS))
    # the layer operators and select_neighbours
    starts = [[int(s)] for s in np.random.default_rng(8).integers(0, N, NQ)]
    a = O.search_k(p.hc, 0, starts, p.Q, 5, ef=20, counters=True)
    b = O.search_k(p.hi, 0, starts, p.NQ, 5, ef=20, counters=True)
    assert [[(i, np.float32(x).tobytes()) for i, x in r] for r in a[0]] == [[(i, np.float32(x).tobytes()) for i, x in r] for r in b[0]]
    _same(a[1:], b[1:], "search_k counters")
    s0 = np.array([s[0] for s in starts], np.int64)
    p.both(lambda h, Q: O.search_one(h, 0, s0, Q, with_distance=True), "search_one")
    p.both(lambda h, Q: H.Ba.search_one(h, 0, s0, Q), "Ba.search_one")
    cl = [list(map(int, np.random.default_rng(9 + i).choice(N, 30, replace=False))) for i in range(NQ)]
    assert O.select_neighbours(p.hc, p.Q, cl, 8) == O.select_neighbours(p.hi, p.NQ, cl, 8)
    assert O.select_neighbours(p.hc, p.Q, cl, 8, keep_all_if_few=True) == O.select_neighbours(p.hi, p.NQ, cl, 8, keep_all_if_few=True)


def test_twin_filtered_and_range(H, pair):
    total = 0
    for name, call in _filtered_and_range_calls(H, pair):
        got = pair.both(call, name)
        if name == "brute range":
            total = len(got[1])
    assert total > NQ                                          # the radius cuts through the data: the range calls return something


@pytest.mark.parametrize("option,value", [("half_rows", 1), ("sq8_rows", 1), ("refine", 40), ("filter_collect", 1)])
def test_twin_under_options(H, pair, option, value):
    p = pair
    rows = {"half_rows": H.ROWS_HALF, "sq8_rows": H.ROWS_SQ8}
    if option == "refine":
        p.set_option("half_rows", 1)
    p.set_option(option, value)
    try:
        if option in rows:
            assert p.hc.info().row_format == p.hi.info().row_format == rows[option]
        if option == "sq8_rows":
            assert p.hc.sq8_params() == p.hi.sq8_params()
            _same(p.hc.sq8_codes(), p.hi.sq8_codes(), "sq8 codes")
        for name, call in _knn_calls(H) + _filtered_and_range_calls(H, p):
            p.both(call, "%s under %s" % (name, option))
    finally:
        p.set_option(option, 0)
        if option == "refine":
            p.set_option("half_rows", 0)
    p.both(_knn_calls(H)[0][1], "after %s" % option)


# ---- 3. life cycle -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [20, 100])
def test_life_cycle(H, d, tmp_path):
    O = H.Ohnsw
    p = Pair(H, d)
    knn = _knn_calls(H)[0][1]

    def still_twins(ctx):
        assert p.hc.n == p.hi.n and p.hc.info().n == p.hi.info().n
        _same_graph(p.hc, p.hi, ctx)
        _same(p.hc.rows(), p.hi.rows(), ctx + " rows")
        p.both(knn, ctx)

    try:
        Y = _floats(130, d, 50) * np.float32(7.0)
        ids = O.insert_batch(p.hc, Y, M, EFC, seed=SEED)
        _same(ids, O.insert_batch(p.hi, H.normalise(Y), M, EFC, seed=SEED), "new ids")
        _same(p.hc.rows(ids), H.normalise(Y), "the new rows are N(Y)")
        _same(p.hc.rows()[:N], p.NX, "the old rows are not normalised again")
        still_twins("insert")
        gone = np.random.default_rng(51).choice(p.hc.n, 50, replace=False).astype(np.int64)
        _same(O.remove_batch(p.hc, gone), O.remove_batch(p.hi, gone), "remove new ids")
        still_twins("remove")
        marked = np.random.default_rng(52).choice(p.hc.n, 40, replace=False).astype(np.int64)
        p.hc.mark_deleted(marked)
        p.hi.mark_deleted(marked)
        got = p.both(knn, "marked")
        assert not np.isin(got[0], marked).any()
        p.both(lambda h, Q: O.brute_force_knn(h, K, Q), "marked brute force")
        p.both(lambda h, Q: O.range_search(h, p.radius, Q, ef=16, counters=True), "marked range")
        _same(p.hc.compact(), p.hi.compact(), "compact new ids")
        still_twins("compact")
        # save and load: the loaded handle holds the saved rows, bit for bit -- nothing is normalised again
        before = p.hc.rows()
        path = str(tmp_path / "cosine.idx")
        p.hc.save(path)
        loaded = H.Hgraph.load(path)
        try:
            assert loaded.info().metric == H.METRIC_COSINE and loaded.metric == H.METRIC_COSINE
            _same(loaded.rows(), before, "loaded rows")
            _same_graph(loaded, p.hi, "loaded")
            _same(knn(loaded, p.Q), knn(p.hi, p.NQ), "loaded knn")
        finally:
            loaded.release()
        # export() then to_device(): the host copy is the caller's matrix, so the fresh handle is the same index
        p.hc.export()
        assert p.hc.vectors.shape == (p.hc.n, d)
        again = H.Hgraph(p.hc.vectors, p.hc.deg0, p.hc.nbr0, p.hc.upper, entry_point=p.hc.entry_point, max_degree=p.hc.max_degree,
                         metric=p.hc.metric).to_device(0)
        try:
            _same(again.rows(), before, "re-created rows")
            _same(knn(again, p.Q), knn(p.hi, p.NQ), "re-created knn")
        finally:
            again.release()
    finally:
        p.hc.release()
        p.hi.release()


# ---- 4. the oracle, and what the numbers mean ----------------------------------------------------------------------------------

def test_oracle_parity(H, oracle):
    d = 20
    X = _floats(N, d, 60) * np.float32(4.0)
    Q = _floats(NQ, d, 61)
    NX, NQm = H.normalise(X), H.normalise(Q)
    sp = oracle.Space.ip(NX, arith=oracle.TREE16)
    g = oracle.build_ohnsw(sp, M, EFC, seed=4)
    hc = H.Hgraph(X, g.deg0, g.nbr0, g.upper, entry_point=g.entry_point, max_degree=M, metric=H.METRIC_COSINE)
    try:
        _same(hc.rows(), NX, "rows")
        for ef, k in ((10, 10), (100, 30)):
            ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hc, k, Q, ef=ef, counters=True)
            oi, od, ond, onh = oracle.Ohnsw.knn_batch_bigarray(g, sp, NQm, k=k, ef=ef, ties=oracle.TIES_CANONICAL, counters=True)
            np.testing.assert_array_equal(ids, oi)
            np.testing.assert_array_equal(dist.view(np.uint32), od.view(np.uint32))
            np.testing.assert_array_equal(nh, onh)
        bi, bd = H.Ohnsw.brute_force_knn(hc, 25, Q)
        oi, od = oracle.brute_force_knn(sp, NQm, 25)
        np.testing.assert_array_equal(bi, oi)
        np.testing.assert_array_equal(bd.view(np.uint32), od.view(np.uint32))
        # every brute-force distance within (2 d + 9) 2^-24 of 1 - cos in float64
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
        cos = (Q64 @ X64.T) / (np.linalg.norm(Q64, axis=1)[:, None] * np.linalg.norm(X64, axis=1)[None, :])
        err = np.abs(bd.astype(np.float64) - (1.0 - np.take_along_axis(cos, bi.astype(np.int64), 1)))
        assert err.max() <= (2 * d + 9) * EPS, float(err.max() / EPS)
        # a zero query: cosine distance 1 to everything, the lowest ids first
        zi, zd = H.Ohnsw.brute_force_knn(hc, 5, np.zeros((1, d), np.float32))
        assert zi.tolist() == [[0, 1, 2, 3, 4]] and (zd == 1.0).all()
    finally:
        hc.release()


# ---- 5. the sharded index ------------------------------------------------------------------------------------------------------

def test_sharded_twin(H):
    d = 20
    X = _floats(N, d, 70) * np.float32(0.2)
    Q = _floats(NQ, d, 71) * np.float32(9.0)
    NX, NQm = H.normalise(X), H.normalise(Q)
    sc = H.ShardedHgraph.build(X, M, EFC, [0, 0, 0], seed=SEED, metric=H.METRIC_COSINE)
    si = H.ShardedHgraph.build(NX, M, EFC, [0, 0, 0], seed=SEED, metric=H.METRIC_IP)
    try:
        assert sc.info()[:4] == (N, d, H.METRIC_COSINE, 0) and sc.metric == H.METRIC_COSINE
        radius = 1.0 - 1.5 / np.sqrt(d)
        allow = np.random.default_rng(72).random(N) < 0.3
        for name, call in (
                ("knn", lambda s, B: s.knn_batch(B, 16, K, counters=True)),
                ("knn ef200", lambda s, B: s.knn_batch(B, 200, K, counters=True)),
                ("brute force", lambda s, B: s.brute_force_knn(K, B)),
                ("filtered", lambda s, B: s.knn_batch_filtered(B, 16, K, allow, counters=True)),
                ("range", lambda s, B: s.range_search(B, radius, ef=16, counters=True)),
                ("range filtered", lambda s, B: s.range_search(B, radius, ef=16, filter=allow, counters=True)),
                ("brute range", lambda s, B: s.brute_force_range(B, radius, counters=True))):
            got = call(sc, Q)
            _same(got, call(si, NQm), "sharded " + name)
        # ... and the exact scan is the one index's over all rows
        one = H.Hgraph.flat(X, metric=H.METRIC_COSINE)
        try:
            a, b = sc.brute_force_knn(K, Q), H.Ohnsw.brute_force_knn(one, K, Q)
            np.testing.assert_array_equal(a[0], b[0].astype(np.int64))
            _same(a[1], b[1], "sharded scan distances")
        finally:
            one.release()
    finally:
        sc.release()
        si.release()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(H):
    d = 20
    X = _floats(300, d, 80)
    bad = X.copy()
    bad[211, 3] = np.inf
    with pytest.raises(H.InvalidArgument, match="row 211"):
        H.Hgraph.flat(bad, metric=H.METRIC_COSINE).to_device(0)
    with pytest.raises(H.InvalidArgument, match="row 211"):
        H.Ohnsw.build_batch_bigarray(bad, M, EFC, seed=SEED, metric=H.METRIC_COSINE)
    bad[17, 0] = np.nan                                        # the FIRST such row is named
    with pytest.raises(H.InvalidArgument, match="row 17"):
        H.Ohnsw.build_batch_bigarray(bad, M, EFC, seed=SEED, metric=H.METRIC_COSINE)
    X[5] = 0.0                                                 # a zero row is accepted
    hc = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=SEED, metric=H.METRIC_COSINE)
    try:
        assert not hc.rows([5]).any()
        before_rows, before_graph = hc.rows(), _graph(hc)
        before = H.Ohnsw.knn_batch_bigarray(hc, K, X[:32], ef=16, counters=True)
        Y = _floats(40, d, 81)
        Y[33, 1] = -np.inf
        with pytest.raises(H.InvalidArgument, match="row 33"):
            H.Ohnsw.insert_batch(hc, Y, M, EFC, seed=SEED)
        with pytest.raises(H.InvalidArgument, match="metric 1 differs from the index's 2"):
            H.Ohnsw.insert_batch(hc, Y[:8], M, EFC, seed=SEED, metric=H.METRIC_IP)
        # the index is as it was after the refused inserts
        assert hc.info().n == 300 == hc.n and hc.vectors.shape == (300, d)
        _same(hc.rows(), before_rows, "rows after a refused insert")
        _same(_graph(hc)[2:], before_graph[2:], "graph after a refused insert")
        _same(H.Ohnsw.knn_batch_bigarray(hc, K, X[:32], ef=16, counters=True), before, "knn after a refused insert")
        with pytest.raises(H.InvalidArgument, match="out of range"):
            hc.rows([0, 300])
        with pytest.raises(H.InvalidArgument, match="out of range"):
            hc.rows([-1])
        with pytest.raises(H.InvalidArgument):
            H._check(H.load().hnsw_index_get_rows(hc.handle, None, 299, H._ptr(np.empty((300, d), np.float32)), d))
        hc.export()
        with pytest.raises(H.Failure, match="cosine: not built for hnsw_multi") as e:
            H.MultiHgraph(hc, [0])
        assert "[%d]" % H.ERR_UNSUPPORTED in str(e.value)
    finally:
        hc.release()
    x = np.ones((2, 1025), np.float32)
    assert H.load().hnsw_normalise_batch(0, H._ptr(x), 2, 1025, 1025, H._ptr(np.empty_like(x)), 1025, None) == H.ERR_UNSUPPORTED
    with pytest.raises(H.Failure, match="d=1025 > 1024"):
        H.normalise(x)


def test_rows_of_other_metrics(H):
    # an L2 handle's rows() are its float32 rows unchanged, also while the searches read the byte copy
    Xb = np.random.default_rng(90).integers(0, 256, (400, 24)).astype(np.float32)
    hb = H.Ohnsw.build_batch_bigarray(Xb, M, EFC, seed=SEED)
    Xf = _floats(400, 100, 91)
    hf = H.Ohnsw.build_batch_bigarray(Xf, M, EFC, seed=SEED, metric=H.METRIC_IP)
    try:
        assert hb.info().row_format == H.ROWS_BYTES
        _same(hb.rows(), Xb, "byte-valued L2 rows")
        _same(hb.rows([399, 0]), Xb[[399, 0]], "byte-valued L2 rows by id")
        _same(hf.rows(), Xf, "IP rows")
        hf.set_option("sq8_rows", 1)
        _same(hf.rows([7, 7, 12]), Xf[[7, 7, 12]], "IP rows under sq8")
    finally:
        hb.release()
        hf.release()
    one = H.Hgraph(Xf[:50], np.zeros(50, np.int32), np.full((50, 1), -1, np.int32), entry_point=1, id_base=1, max_degree=1)
    try:
        _same(one.rows([1, 50]), Xf[[0, 49]], "id_base-based ids")
        with pytest.raises(H.InvalidArgument, match="out of range"):
            one.rows([0])
    finally:
        one.release()


# ---- 7. the C++ front end ------------------------------------------------------------------------------------------------------

def test_cpp_front_end_cosine(H, tmp_path):
    exe = str(tmp_path / "test_front_cosine")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_cosine.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cosine front-end ok" in out.stdout, out.stdout + out.stderr
