"""Option "sq8_dim_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_sq8_dim.hip, hnsw_sq8_dim_walk.hip): float vectors searched through 8-bit
codes under one affine map PER DIMENSION, and answered from the float32 rows.

The definition the tests hold it to (include/hnsw_mi355x.h): C, lo[d], s[d] come from the quantiser restated in numpy below.  The
walk is held against a TWIN index with the same exported graph: for the inner product (and cosine) a byte-row index over
C.astype(float32) searched with Q' = s * Q -- the unchanged byte-row kernels --; for L2 a float32-row index over Z = C * s (numpy
float32) searched with Q'' = Q - lo -- the new row format of the knn kernel computes fl(fl(c * s) - q'') per dimension, which is the
float32 row's arithmetic over Z.  Both are asked for k := c = min(ef, max(k, R)); the walk's members and hops are the twin's, and the
answer is those members re-ranked over X under (TREE16 distance key, id) with the bits of hnsw_distance_batch.  out_nhops is the
walk's, out_ndist the walk's plus c."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8, ROWS_SQ8_DIM = 0, 2, 3, 4, 5, 6
VT_BITS = 11          # both handles of a twin pair get the same visited cache, so that they forget (and re-evaluate) the same nodes


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


# ---- the quantisers, restated --------------------------------------------------------------------------------------------------

def _quantise_dim(X):
    """(C uint8 [n][d], lo [d], s [d]): float32 operations, round to nearest even"""
    X = np.asarray(X, np.float32)
    zero = np.float32(0)
    lo, hi = X.min(axis=0) + zero, X.max(axis=0) + zero
    s = np.where(hi == lo, np.float32(1), (hi - lo) / np.float32(255)).astype(np.float32)
    code = np.rint((X - lo) / s)
    assert lo.dtype == s.dtype == code.dtype == np.float32
    return np.minimum(np.float32(255), np.maximum(zero, code)).astype(np.uint8), lo, s


def _nch(d):
    per_lane = ((d + 3) // 4 + 15) // 16
    return next(c for c in (1, 2, 4, 8, 16) if per_lane <= c)


def _copy_bytes(n, d):
    """the codes and the two per-dimension tables in the lane grid"""
    return n * 64 * _nch(d) + 2 * 4 * 64 * _nch(d)


def _floats(n, d, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(n, d))).astype(np.float32)


def _spread(n, d, seed, cols=None):
    """columns that do not share a range: scales 2^0 .. 2^-12 and an offset per column (cols: the seed of those; queries take
    their table's)"""
    crng = np.random.default_rng(1000 + (seed if cols is None else cols))
    scale, offset = np.exp2(-crng.integers(0, 13, size=d)), crng.normal(size=d)
    return (np.random.default_rng(seed).normal(size=(n, d)) * scale + offset).astype(np.float32)


def _unit(n, d, seed):
    X = _floats(n, d, seed, 1.0)
    return X / np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)


def _same(got, want, ctx=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx)


def _c(ef, k, R):
    return ef if R == -1 else min(ef, max(k, R))


def _search(H, hg, Q, ef, k, sem):
    return H._search(hg, Q, ef, k, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)


def _check_copy(hg, X):
    C, lo, s = _quantise_dim(X)
    glo, gs = hg.sq8_dim_params()
    assert glo.dtype == gs.dtype == np.float32 and glo.shape == gs.shape == (X.shape[1],)
    np.testing.assert_array_equal(glo.view(np.uint32), lo.view(np.uint32))
    np.testing.assert_array_equal(gs.view(np.uint32), s.view(np.uint32))
    codes = hg.sq8_dim_codes()
    assert codes.shape == X.shape and codes.dtype == np.uint8                 # [n][d]: the padding of the lane grid stays behind
    np.testing.assert_array_equal(codes, C)
    return C, lo, s


class Rerank:
    """the members of a walk re-ranked over the float32 rows Xs with the queries Qs (what the index stores and reads: N(X), N(Q) for
    a cosine index), as test_gpu_sq8.py's Expect.answer restates it; the TREE16 keys are computed once and shared between the cases"""

    def __init__(self, oracle, Xs, Qs, metric):
        self.o, self.X, self.Q, self.metric, self._keys = oracle, np.asarray(Xs, np.float32), np.asarray(Qs, np.float32), metric, {}

    def key(self, q, j):
        if (q, j) not in self._keys:
            if self.metric:
                dist = np.float32(1.0) - np.float32(self.o.dot_tree16(self.X[j], self.Q[q]))
                self._keys[(q, j)] = (dist, dist)
            else:
                sq = np.float32(self.o.l2sq_tree16(self.X[j], self.Q[q]))
                self._keys[(q, j)] = (sq, np.float32(np.sqrt(np.float64(sq))))
        return self._keys[(q, j)]

    def answer(self, W, k, sem):
        """(ids, distances, members of W per query)"""
        nq = len(self.Q)
        ids = np.full((nq, k), -1, np.int32)
        dist = np.full((nq, k), np.float32(np.inf) if sem else np.float32(np.nan), np.float32)
        real = np.zeros(nq, np.uint32)
        for q in range(nq):
            ids0 = W[q][W[q] >= 0].astype(np.int64)
            real[q] = len(ids0)
            kd = [self.key(q, int(j)) for j in ids0]
            o = np.lexsort((ids0, np.array([a for a, _ in kd], np.float32)))[:k]
            ids[q, :len(o)] = ids0[o]
            dist[q, :len(o)] = np.array([b for _, b in kd], np.float32)[o]
        return ids, dist, real


def _twin(H, hg, rows, metric, byte_rows):
    """the same exported graph over other rows"""
    hg.export()
    twin = H.Hgraph(rows, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree, metric=metric)
    if not byte_rows:
        twin.set_option("byte_rows", 0)
    assert (twin.info().row_format == ROWS_BYTES) == byte_rows
    return twin


def _pin_visited(*handles):
    for h in handles:
        h.set_option("vt_bits", VT_BITS)
        h.set_option("visited_blocks", 0)


def _check_against_twin(H, hg, twin, rr, Q, Qt, cases, ctx0, entry=None):
    """every (sem, ef, k, R) of cases: our answer against the twin's walk of k := c, re-ranked; hops, evaluations, members"""
    entry = entry or (lambda ef, k, sem: _search(H, hg, Q, ef, k, sem))
    walks = {}
    for sem, ef, k, R in cases:
        ctx = "%s rule %d ef %d k %d R %d" % (ctx0, sem, ef, k, R)
        c = _c(ef, k, R)
        hg.set_option("refine", R)
        ids, dist, nd, nh = entry(ef, k, sem)
        if (sem, ef, c) not in walks:
            walks[(sem, ef, c)] = _search(H, twin, Qt, ef, c, sem)
        W, _, tnd, tnh = walks[(sem, ef, c)]
        wi, wd, real = rr.answer(W, k, sem)
        _same((ids, dist), (wi, wd), ctx)
        np.testing.assert_array_equal(nh, tnh, err_msg=ctx)
        np.testing.assert_array_equal(nd - np.uint32(c), tnd, err_msg=ctx)
        assert (real == c).all(), ctx                                          # (a connected graph of n >= c nodes fills W)
        # the walk's members: ours asked for k := c comes back re-ranked, the same set
        ours = _search(H, hg, Q, ef, c, sem)[0] if c != k else ids
        np.testing.assert_array_equal(np.sort(ours, axis=1), np.sort(W, axis=1), err_msg=ctx)
        # every returned distance is the distance to its own vector
        np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32), err_msg=ctx)
    hg.set_option("refine", 0)


# ---- 1. the quantiser's bits ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [20, 100, 257])
def test_quantiser_bits(H, d):
    n = 700
    X = _spread(n, d, 40 + d)
    hg = H.Hgraph.flat(X)
    before = hg.info().device_bytes
    hg.set_option("sq8_dim_rows", 1)
    assert hg.info().row_format == ROWS_SQ8_DIM and hg.row_bytes() == d
    C, lo, s = _check_copy(hg, X)
    assert (C.min(axis=0) == 0).all() and (C.max(axis=0) == 255).all() and len(np.unique(s)) > 1
    assert hg.info().device_bytes - before == _copy_bytes(n, d)
    hg.release()


def test_quantiser_edge_tables(H):
    # a constant column (s = 1, every code 0) among ordinary ones; a column of +-0, whose bound counts as +0
    X = _floats(300, 20, 3)
    X[:, 4] = np.float32(-2.75)
    X[:, 9] = np.float32(0.0)
    X[::2, 9] = np.float32(-0.0)
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_dim_rows", 1)
    C, lo, s = _check_copy(hg, X)
    glo, gs = hg.sq8_dim_params()
    assert gs[4] == 1 and glo[4] == np.float32(-2.75) and not C[:, 4].any()
    assert gs[9] == 1 and glo[9].view(np.uint32) == 0 and not C[:, 9].any()
    hg.release()
    # exact ties go to the even code: lo = 0, s = 1 in column 0
    X = _floats(300, 12, 4)
    X[:, 0] = (np.arange(300) % 255 + 0.5).astype(np.float32)
    X[0, 0], X[1, 0] = 0.0, 255.0
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_dim_rows", 1)
    C, lo, s = _check_copy(hg, X)
    assert lo[0] == 0 and s[0] == 1 and not (C[2:, 0] % 2).any()
    hg.release()
    # n = 1: every column is constant
    X = _floats(1, 33, 5)
    hg = H.Hgraph.flat(X)
    hg.set_option("sq8_dim_rows", 1)
    C, lo, s = _check_copy(hg, X)
    assert (s == 1).all() and not C.any()
    np.testing.assert_array_equal(lo.view(np.uint32), (X[0] + np.float32(0)).view(np.uint32))
    hg.release()


@pytest.mark.parametrize("bad", ["nan", "inf", "range", "narrow"])
def test_values_that_cannot_be_quantised_leave_the_index_unchanged(H, bad):
    n, d, col = 900, 40, 17
    X, Q = _floats(n, d, 70), _floats(20, d, 71)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    hg.export()
    Y = X.copy()
    if bad == "range":                               # finite values whose max - min overflows float32
        Y[5, col], Y[n - 1, col] = np.float32(3e38), np.float32(-3e38)
    elif bad == "narrow":                            # a subnormal range: (hi - lo) / 255 rounds to 0
        Y[:, col] = np.float32(0)
        Y[3, col] = np.float32(1e-44)
    else:
        Y[n - 1, col] = np.float32(bad)
        Y[7, col + 5] = np.float32(bad)              # a later column as well: the first is named
    hb = H.Hgraph(Y, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree)
    info0 = hb.info()
    before = H.Ohnsw.knn_batch_bigarray(hb, 5, Q, ef=40) if bad in ("range", "narrow") else None
    assert H.load().hnsw_index_set_option(hb.handle, b"sq8_dim_rows", 1) == H.ERR_UNSUPPORTED
    assert ("column %d" % col) in H.load().hnsw_last_error().decode()
    info1 = hb.info()
    assert info1.row_format == info0.row_format and info1.device_bytes == info0.device_bytes
    with pytest.raises(H.InvalidArgument):
        hb.sq8_dim_params()
    if before is not None:
        _same(H.Ohnsw.knn_batch_bigarray(hb, 5, Q, ef=40), before)
    hb.release()
    hg.release()


# ---- 2. the inner product: the byte-row kernels over the codes, the query scaled --------------------------------------------

IP_CASES = [(sem, ef, 10, R) for sem in (0, 1) for ef, R in ((16, 0), (64, 32), (200, -1))]


@pytest.mark.parametrize("d", [100, 257])
def test_inner_product_walk_is_the_byte_row_twin(H, oracle, d):
    n, nq = 1500, 64
    X, Q = _unit(n, d, 10 + d) * np.exp2(-np.arange(d) % 7).astype(np.float32), _unit(nq, d, 20 + d)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=3, metric=H.METRIC_IP)
    hg.set_option("sq8_dim_rows", 1)
    assert hg.info().row_format == ROWS_SQ8_DIM and hg.row_bytes() == d
    C, lo, s = _check_copy(hg, X)
    twin = _twin(H, hg, C.astype(np.float32), H.METRIC_IP, True)
    _pin_visited(hg, twin)
    _check_against_twin(H, hg, twin, Rerank(oracle, X, Q, 1), Q, (s * Q).astype(np.float32), IP_CASES, "ip d %d" % d)
    twin.release()
    hg.release()


def test_cosine_walk_is_its_inner_product_twin(H, oracle):
    n, nq, d = 1200, 64, 72
    X, Q = _spread(n, d, 31), _spread(nq, d, 32, cols=31)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=3, metric=H.METRIC_COSINE)
    NX, NQ = hg.rows(), H.normalise(Q)                                         # what the index stores and what its searches read
    hg.set_option("sq8_dim_rows", 1)
    assert hg.info().row_format == ROWS_SQ8_DIM
    C, lo, s = _check_copy(hg, NX)
    twin = _twin(H, hg, C.astype(np.float32), H.METRIC_IP, True)
    _pin_visited(hg, twin)
    _check_against_twin(H, hg, twin, Rerank(oracle, NX, NQ, 1), Q, (s * NQ).astype(np.float32), IP_CASES[:3] + IP_CASES[4:5], "cosine")
    twin.release()
    hg.release()


# ---- 3. L2: the weighted walk, the new row format of the knn kernel -----------------------------------------------------------

L2_CASES = [(sem, ef, 10, R) for sem in (0, 1) for ef, R in ((16, 0), (64, 32), (200, -1), (300, 32))]


@pytest.fixture(scope="module")
def l2_world(H, oracle):
    """per d: the index with the option on, its float32 twin over Z = C * s, the queries both ways, the re-rank -- built once"""
    made = {}

    def get(d):
        if d not in made:
            n, nq, M, efc = (700, 64, 6, 30) if d > 256 else (1500, 64, 10, 40)
            X, Q = _spread(n, d, 10 + d), _spread(nq, d, 20 + d, cols=10 + d)
            hg = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=3)
            hg.set_option("sq8_dim_rows", 1)
            assert hg.info().row_format == ROWS_SQ8_DIM and hg.row_bytes() == d
            C, lo, s = _check_copy(hg, X)
            Z = C.astype(np.float32) * s
            assert Z.dtype == np.float32
            twin = _twin(H, hg, Z, H.METRIC_L2, False)
            _pin_visited(hg, twin)
            made[d] = (hg, twin, Rerank(oracle, X, Q, 0), Q, (Q - lo).astype(np.float32))
        return made[d]
    yield get
    for hg, twin, _, _, _ in made.values():
        twin.release()
        hg.release()


@pytest.mark.parametrize("d", [20, 100, 128, 257, 1024])
def test_l2_walk_is_the_float32_twin_over_z(H, l2_world, d):
    hg, twin, rr, Q, Qt = l2_world(d)
    hg.set_option("order_queries", 0)
    _check_against_twin(H, hg, twin, rr, Q, Qt, L2_CASES, "l2 d %d" % d)


@pytest.mark.parametrize("d", [20, 100, 128, 257, 1024])
def test_l2_walk_behind_the_ordering_pre_pass(H, l2_world, d):
    """order_queries 1: the descent runs in the pre-pass kernel, over the codes with their scales as well"""
    hg, twin, rr, Q, Qt = l2_world(d)
    hg.set_option("order_queries", 1)
    try:
        _check_against_twin(H, hg, twin, rr, Q, Qt, L2_CASES[1:3] + L2_CASES[5:6], "l2 ordered d %d" % d)
    finally:
        hg.set_option("order_queries", 0)


@pytest.mark.parametrize("d", [100, 1024])
def test_l2_walk_through_knn_and_submit(H, l2_world, d):
    hg, twin, rr, Q, Qt = l2_world(d)

    def submitted(ef, k, sem):
        r1 = H.submit(hg, Q[:40], ef, k, fill=H.FILL_BA if sem else H.FILL_OHNSW, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)
        r2 = H.submit(hg, Q[40:], ef, k, fill=H.FILL_BA if sem else H.FILL_OHNSW, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)
        b, a = r2.wait(counters=True), r1.wait(counters=True)
        return tuple(np.concatenate([x, y]) for x, y in zip(a, b))
    _check_against_twin(H, hg, twin, rr, Q, Qt, [L2_CASES[1], L2_CASES[6]], "l2 submit d %d" % d, entry=submitted)
    ids, dist, _, _ = _search(H, hg, Q, 64, 10, 0)
    for q in (0, 7, 63):
        one = H.Ohnsw.knn(hg, 10, Q[q], ef=64)
        assert [i for i, _ in one] == list(ids[q]) and [np.float32(x).view(np.uint32) for _, x in one] == list(dist[q].view(np.uint32))


# ---- 4. what the option is for -------------------------------------------------------------------------------------------------

def _recall(ids, truth):
    return np.mean([len(set(a) & set(b)) for a, b in zip(ids, truth)]) / truth.shape[1]


def _scan(R, Q, k):
    """exact L2 scan over a reconstruction, float64: ids [nq][k] under (distance, id)"""
    d2 = ((Q.astype(np.float64)[:, None, :] - R.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def test_outliers_in_one_column_cost_the_global_map_its_recall(H):
    """n 2000, d 32, standard normal, 8 rows multiplied by 400 in dimension 0: one map for the whole table spends its codes on
    that column.  First the input is guarded -- the exact scans over the two reconstructions, from the library's own codes and
    parameters, differ by at least 0.3 in recall@10 --, then the searches on ONE handle are compared: no threshold on a walk."""
    n, d, nq, k, ef = 2000, 32, 200, 10, 64
    rng = np.random.default_rng(11)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[rng.choice(n, 8, replace=False), 0] *= np.float32(400)
    Q = rng.normal(size=(nq, d)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 16, 64, seed=2)
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]
    hg.set_option("refine", 0)
    hg.set_option("sq8_rows", 1)
    glo, gs = hg.sq8_params()
    Rg = glo + gs * hg.sq8_codes().astype(np.float32)
    found_global = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
    hg.set_option("sq8_rows", 0)
    hg.set_option("sq8_dim_rows", 1)
    lo, s = hg.sq8_dim_params()
    Rd = lo + s * hg.sq8_dim_codes().astype(np.float32)
    found_dim = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
    scan_global, scan_dim = _recall(_scan(Rg, Q, k), truth), _recall(_scan(Rd, Q, k), truth)
    r_global, r_dim = _recall(found_global, truth), _recall(found_dim, truth)
    print("recall@%d exact scan over X^: global %.4f per-dimension %.4f; search: sq8_rows %.4f sq8_dim_rows %.4f"
          % (k, scan_global, scan_dim, r_global, r_dim))
    assert scan_dim - scan_global >= 0.3
    assert r_dim > r_global
    hg.release()


# ---- 5. life cycle -------------------------------------------------------------------------------------------------------------

def test_option_values_and_exclusions(H, tmp_path):
    n, d = 1500, 100
    X, Q = _spread(n, d, 50), _spread(30, d, 51, cols=50)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    L = H.load()
    rows0, bytes0 = hg.info().row_format, hg.info().device_bytes
    assert rows0 == ROWS_SPLIT and hg.row_bytes() == 4 * d
    before = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    for call in (hg.sq8_dim_params, hg.sq8_dim_codes):
        with pytest.raises(H.InvalidArgument, match="sq8"):
            call()                                   # no copy yet
    for bad in (2, -2, 7):
        assert L.hnsw_index_set_option(hg.handle, b"sq8_dim_rows", bad) == H.ERR_BAD_ARG
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0
    hg.set_option("sq8_dim_rows", 1)
    copy = _copy_bytes(n, d)
    assert hg.info().row_format == ROWS_SQ8_DIM and hg.row_bytes() == d and hg.info().device_bytes == bytes0 + copy
    on = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, on[0]).view(np.uint32), on[1].view(np.uint32))
    with pytest.raises(H.InvalidArgument, match="sq8_dim_rows"):
        H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    # the three options it excludes, while it is on: refused, nothing moves
    for other in ("half_rows", "sq8_rows", "filter_collect"):
        assert L.hnsw_index_set_option(hg.handle, other.encode(), 1) == H.ERR_BAD_ARG, other
        assert "sq8_dim_rows" in L.hnsw_last_error().decode()
        assert hg.info().row_format == ROWS_SQ8_DIM and hg.info().device_bytes == bytes0 + copy
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), on)
    hg.set_option("sq8_dim_rows", 1)                # again: nothing changes
    assert hg.info().device_bytes == bytes0 + copy
    # 0: the previous rows again, the copy kept; results as if the option had never been set
    hg.set_option("sq8_dim_rows", 0)
    assert hg.info().row_format == rows0 and hg.row_bytes() == 4 * d and hg.info().device_bytes == bytes0 + copy
    _check_copy(hg, X)
    after = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    _same(after[:2], before[:2])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    # the reverse: refused while one of the three is on
    for other, rows in (("half_rows", ROWS_HALF), ("sq8_rows", ROWS_SQ8), ("filter_collect", rows0)):
        hg.set_option(other, 1)
        assert L.hnsw_index_set_option(hg.handle, b"sq8_dim_rows", 1) == H.ERR_BAD_ARG, other
        assert other in L.hnsw_last_error().decode()
        assert hg.info().row_format == rows
        hg.set_option(other, 0 if other == "filter_collect" else -1)
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0 + copy
    # -1: ... and the copy freed
    hg.set_option("sq8_dim_rows", 1)
    hg.set_option("sq8_dim_rows", -1)
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0
    with pytest.raises(H.InvalidArgument, match="sq8"):
        hg.sq8_dim_params()
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), before[:2])
    # not saved
    hg.set_option("sq8_dim_rows", 1)
    path = os.path.join(str(tmp_path), "index.hnsw")
    hg.save(path)
    back = H.Hgraph.load(path)
    assert back.info().row_format == rows0
    with pytest.raises(H.InvalidArgument, match="sq8"):
        back.sq8_dim_codes()
    _same(H.Ohnsw.knn_batch_bigarray(back, 10, Q, ef=100), before[:2])
    back.release()
    hg.release()


def test_refused_with_byte_rows_in_use(H):
    X = np.random.default_rng(3).integers(0, 256, size=(800, 64)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    assert hg.info().row_format == ROWS_BYTES
    bytes0 = hg.info().device_bytes
    with pytest.raises(H.InvalidArgument, match="byte rows"):
        hg.set_option("sq8_dim_rows", 1)
    assert hg.info().row_format == ROWS_BYTES and hg.info().device_bytes == bytes0
    hg.release()


def test_insert_and_remove_quantise_the_table_again(H):
    n0, m, d, nq = 1200, 300, 72, 24
    X = _spread(n0 + m, d, 90)
    X[n0:] *= np.float32(2.5)                                                  # the new vectors widen the ranges
    Q = X[n0:n0 + nq] + _floats(nq, d, 91, 0.01)
    hg = H.Ohnsw.build_batch_bigarray(X[:n0], 10, 40, seed=5)
    hg.set_option("sq8_dim_rows", 1)
    _, lo0, s0 = _check_copy(hg, X[:n0])
    H.Ohnsw.insert_batch(hg, X[n0:], 10, 40, seed=5)
    assert hg.n == n0 + m and hg.info().row_format == ROWS_SQ8_DIM
    _, lo1, s1 = _check_copy(hg, X)
    assert (s1 >= s0).all() and (s1 > s0).any()
    ids, dist = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64)
    assert (ids >= n0).any()                                                   # inserted vectors among the answers
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32))
    # a new vector that is not finite: nothing inserted, codes, parameters and results as before
    codes, params, bytes0 = hg.sq8_dim_codes(), hg.sq8_dim_params(), hg.info().device_bytes
    for v in (np.nan, np.inf):
        Y = _floats(40, d, 92)
        Y[39, d - 1] = v
        with pytest.raises(H.Failure, match="sq8_dim_rows"):
            H.Ohnsw.insert_batch(hg, Y, 10, 40, seed=5)
        inf = hg.info()
        assert inf.n == n0 + m and inf.row_format == ROWS_SQ8_DIM and inf.device_bytes == bytes0
        np.testing.assert_array_equal(hg.sq8_dim_codes(), codes)
        for a, b in zip(hg.sq8_dim_params(), params):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64), (ids, dist))
    # remove the widening vectors again: the remaining table is quantised again
    gone = np.arange(n0, n0 + m, dtype=np.int64)
    H.Ohnsw.remove_batch(hg, gone)
    assert hg.n == n0 and hg.info().row_format == ROWS_SQ8_DIM
    _check_copy(hg, hg.rows())
    np.testing.assert_array_equal(hg.rows(), X[:n0])
    hg.release()


def test_filtered_and_range_calls_answer_with_exact_distances(H):
    n, d, nq, k = 1500, 48, 40, 10
    X, Q = _spread(n, d, 60), _spread(nq, d, 61, cols=60)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=8)
    hg.set_option("sq8_dim_rows", 1)
    allow = np.random.default_rng(1).random(n) < 0.5
    ids, dist = H.Ohnsw.knn_batch_filtered(hg, k, Q, allow, ef=64)[:2]
    assert (ids >= 0).all() and allow[ids].all()
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32))
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)
    radius = float(np.median(truth[1][:, -1]))
    lims, rids, rdist = H.Ohnsw.range_search(hg, radius, Q, ef=64)[:3]
    assert lims[-1] > 0
    for q in range(nq):
        seg = slice(int(lims[q]), int(lims[q + 1]))
        if seg.stop > seg.start:
            want = H.Ohnsw.distance_l2(hg, Q[q:q + 1], rids[seg].astype(np.int32)[None, :])[0]
            np.testing.assert_array_equal(want.view(np.uint32), rdist[seg].view(np.uint32))
            assert (rdist[seg] <= np.float32(radius)).all()
    hg.release()


def test_sharded_option_equals_the_merge_of_the_shards(H):
    n, d, nq, k, ef = 2000, 48, 64, 10, 64
    X, Q = _spread(n, d, 62), _spread(nq, d, 63, cols=62)
    s = H.ShardedHgraph.build(X, 10, 40, [0, 0], seed=4)
    s.set_option("sq8_dim_rows", 1)
    ids, dist, first = [], [], []
    for g in range(2):
        hg, lo = s.shard(g)
        assert hg.info().row_format == ROWS_SQ8_DIM
        _check_copy(hg, hg.rows())                                             # per-shard maps
        i, dd = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
        ids.append(i); dist.append(dd); first.append(lo)
    want = H.merge_lists(np.stack(ids), np.stack(dist), first, k, id_base=s.id_base)
    got = s.knn_batch(Q, ef, k)
    _same(got[:2], want)
    s.set_option("sq8_dim_rows", -1)
    assert [s.shard(g)[0].info().row_format for g in range(2)] != [ROWS_SQ8_DIM] * 2
    s.release()


def test_a_handle_that_never_set_the_option_is_untouched(H):
    n, d = 1500, 100
    X, Q = _spread(n, d, 64), _spread(30, d, 65, cols=64)
    plain = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    before = H.Ohnsw.knn_batch_bigarray(plain, 10, Q, ef=100, counters=True)
    other = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    other.set_option("sq8_dim_rows", 1)
    H.Ohnsw.knn_batch_bigarray(other, 10, Q, ef=100)
    after = H.Ohnsw.knn_batch_bigarray(plain, 10, Q, ef=100, counters=True)
    _same(after[:2], before[:2])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    other.release()
    plain.release()
