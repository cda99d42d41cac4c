"""Option "bit_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_bits.hip, hnsw_bits_walk.hip): float vectors searched through ONE BIT per
dimension under Hamming distance, and answered from the float32 rows.

The definition the tests hold it to (include/hnsw_mi355x.h): bit i of a row is x_i > t_i, t = 0 (mode 2) or the column means (mode
1), packed little-endian into uint32 words -- numpy.packbits restates the codes.  The walk is held against a TWIN: a float32-row L2
index with the same exported graph over S = where(X > t, 1, -1), searched with where(Q > t, 1, -1), whatever the metric of the
index itself.  Both are asked for k := c = ef with refine -1; the walk's members, hops and evaluations are the twin's, and the answer
is those members re-ranked over X under (distance key, id) with the bits of hnsw_distance_batch."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8, ROWS_SQ8_DIM, ROWS_BITS = 0, 2, 3, 4, 5, 6, 7
VT_BITS = 11          # both handles of a twin pair get the same visited cache, so that they forget (and re-evaluate) the same nodes
N = 3000
DIMS = [20, 100, 512, 513, 1024]       # part of one word; a ragged last word; a full one-step row; one bit in the second step; two full steps
EFS = [40, 128, 192, 256, 384, 512, 1024]   # W in 1, 2, 3 (two-step rows), 4, 6 (two-step rows), 8 and 16 registers


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


# ---- the definition, restated ----------------------------------------------------------------------------------------------------

def _nw(d):
    return 2 if d > 512 else 1


def _copy_bytes(n, d):
    """the codes and the threshold table: n * 64 * NW + 4 * 512 * NW (the header's formula)"""
    return n * 64 * _nw(d) + 4 * 512 * _nw(d)


def _codes(X, t):
    """uint32 [n][ceil(d / 32)]: dimension i in bit i % 32 of word i // 32"""
    X = np.asarray(X, np.float32)
    b = np.packbits(X > np.asarray(t, np.float32), axis=1, bitorder="little")
    pad = (-b.shape[1]) % 4
    if pad:
        b = np.concatenate([b, np.zeros((b.shape[0], pad), np.uint8)], axis=1)
    return np.ascontiguousarray(b).view("<u4")


def _pm(X, t):
    S = np.where(np.asarray(X, np.float32) > np.asarray(t, np.float32), np.float32(1), np.float32(-1))
    assert S.dtype == np.float32
    return S


def _table(n, d, seed, cols=None):
    """standard normal columns with an offset each (so the two modes cut in different places), and exact zeros of both signs"""
    crng = np.random.default_rng(2000 + (seed if cols is None else cols))
    offset = crng.normal(size=d) * 0.7
    X = (np.random.default_rng(seed).normal(size=(n, d)) + offset).astype(np.float32)
    z = np.random.default_rng(seed + 7).random((n, d))
    X[z < 0.02] = np.float32(0.0)
    X[z > 0.98] = np.float32(-0.0)
    return X


def _same(got, want, ctx=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx)


def _search(H, hg, Q, ef, k, sem):
    return H._search(hg, Q, ef, k, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)


def _check_copy(hg, X, mode):
    """thresholds and codes of the handle against the rule over X (mode 1: against the thresholds the handle reports)"""
    t = hg.bit_params()
    assert t.dtype == np.float32 and t.shape == (X.shape[1],)
    if mode == 2:
        np.testing.assert_array_equal(t.view(np.uint32), np.zeros(X.shape[1], np.uint32))        # +0, every one
    codes = hg.bit_codes()
    assert codes.dtype == np.uint32 and codes.shape == (X.shape[0], (X.shape[1] + 31) // 32)      # the padding words stay behind
    np.testing.assert_array_equal(codes, _codes(X, t))
    return t, codes


def _twin(H, hg, rows):
    """a float32-row L2 index with the same exported graph over other rows"""
    hg.export()
    twin = H.Hgraph(rows, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree, metric=H.METRIC_L2)
    twin.set_option("byte_rows", 0)
    assert twin.info().row_format in (ROWS_F32, ROWS_SPLIT)
    return twin


def _pin_visited(*handles, blocks=0):
    for h in handles:
        h.set_option("vt_bits", VT_BITS)
        h.set_option("visited_blocks", blocks)


def _reranked(H, oracle, hg, Xs, Qs, Q, W, metric, sem):
    """the members W ([nq][c]; -1: W held fewer) in the order of the re-rank: (distance key, id), the distances hnsw_distance_batch's
    bits, what W lacks filled as the search fills it.  The key of L2 is the SQUARED distance: where two members share a float32
    distance, the oracle's TREE16 squares decide before the ids."""
    all_dist = H.Ohnsw.distance_l2(hg, Q, np.maximum(W, 0))
    ids = np.full_like(W, -1)
    out = np.full_like(all_dist, np.float32(np.inf) if sem else np.float32(np.nan))
    for q in range(W.shape[0]):
        real = W[q] >= 0
        w, dist = W[q][real], all_dist[q][real]
        sq = np.zeros(len(w), np.float32)            # compared only inside a class of equal distances: 0 elsewhere
        if metric == H.METRIC_L2:
            vals, counts = np.unique(dist, return_counts=True)
            for v in vals[counts > 1]:
                for j in np.flatnonzero(dist == v):
                    sq[j] = np.float32(oracle.l2sq_tree16(Xs[w[j]], Qs[q]))
        o = np.lexsort((w, sq, dist))
        ids[q, :len(w)], out[q, :len(w)] = w[o], dist[o]
    return ids, out


def _check_against_twin(H, oracle, w, cases, ctx0, entry=None):
    """every (sem, ef) of cases, k := c = ef under refine -1: members, hops and evaluations are the twin's, the rows the re-rank's"""
    hg, twin, Q, Qs = w["hg"], w["twin"], w["Q"], w["Qs"]
    entry = entry or (lambda ef, k, sem: _search(H, hg, Q, ef, k, sem))
    hg.set_option("refine", -1)
    for sem, ef in cases:
        ctx = "%s rule %d ef %d" % (ctx0, sem, ef)
        ids, dist, nd, nh = entry(ef, ef, sem)
        W, _, tnd, tnh = _search(H, twin, Qs, ef, ef, sem)
        # (a walk that starts in a node without neighbours ends with fewer than ef members, -1 in both answers: the re-rank then
        # evaluates the members there are)
        real = (W >= 0).sum(axis=1).astype(np.uint32)
        assert 2 * (real == ef).sum() > len(real), ctx
        np.testing.assert_array_equal(np.sort(ids, axis=1), np.sort(W, axis=1), err_msg=ctx)
        np.testing.assert_array_equal(nh, tnh, err_msg=ctx)
        np.testing.assert_array_equal(nd - real, tnd, err_msg=ctx)
        _same((ids, dist), _reranked(H, oracle, hg, w["Xs"], w["Qn"], Q, W, w["metric"], sem), ctx)
    hg.set_option("refine", 0)


# ---- 1. the quantiser's bits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_quantiser_bits(H, d):
    X = _table(N, d, 40 + d)
    assert (X == 0).any() and np.signbit(X[X == 0]).any() and not np.signbit(X[X == 0]).all()
    hg = H.Hgraph.flat(X)
    before = hg.info().device_bytes
    hg.set_option("bit_rows", 2)
    assert hg.info().row_format == ROWS_BITS and hg.row_bytes() == (d + 7) // 8
    assert hg.info().device_bytes - before == _copy_bytes(N, d)
    t, codes = _check_copy(hg, X, 2)
    np.testing.assert_array_equal(codes, _codes(X, 0))                         # numpy.packbits(X > 0, bitorder="little") as uint32
    hg.set_option("bit_rows", 1)
    assert hg.info().row_format == ROWS_BITS and hg.info().device_bytes - before == _copy_bytes(N, d)
    t1, codes1 = _check_copy(hg, X, 1)
    assert (codes1 != codes).any()
    # the means: a float64 sum of n values in any order is within n * 2^-53 * sum|x| of the exact one, so its quotient by n within
    # n * 2^-53 * mean|x|; twice that for the two sums compared here, plus one float32 rounding: derived, not measured
    mean = X.astype(np.float64).mean(axis=0)
    ref = mean.astype(np.float32)
    bound = np.spacing(np.abs(ref)).astype(np.float64) + N * 2.0 ** -52 * np.abs(X.astype(np.float64)).mean(axis=0)
    err = np.abs(t1.astype(np.float64) - ref.astype(np.float64))
    print("d %d: max |t - mean| %.3g, least bound %.3g" % (d, err.max(), bound.min()))
    assert (err <= bound).all()
    # the same table gives the same thresholds again
    hg.set_option("bit_rows", 0)
    hg.set_option("bit_rows", 1)
    np.testing.assert_array_equal(hg.bit_params().view(np.uint32), t1.view(np.uint32))
    np.testing.assert_array_equal(hg.bit_codes(), codes1)
    hg.release()


def test_equality_with_the_threshold_gives_zero(H):
    # a constant column IS its mean; a column of +-0 under mode 2; one value above in each
    X = _table(300, 40, 3)
    X[:, 4] = np.float32(-2.75)
    X[:, 9] = np.float32(0.0)
    X[::2, 9] = np.float32(-0.0)
    hg = H.Hgraph.flat(X)
    hg.set_option("bit_rows", 1)
    t, codes = _check_copy(hg, X, 1)
    assert t[4] == np.float32(-2.75) and t[9] == 0
    assert not ((codes[:, 0] >> 4) & 1).any() and not ((codes[:, 0] >> 9) & 1).any()
    hg.set_option("bit_rows", 2)
    t, codes = _check_copy(hg, X, 2)
    assert not ((codes[:, 0] >> 4) & 1).any() and not ((codes[:, 0] >> 9) & 1).any()
    hg.release()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_values_that_are_not_finite_leave_the_index_unchanged(H, bad, mode):
    n, d, col = 900, 40, 17
    X, Q = _table(n, d, 70), _table(20, d, 71, cols=70)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    hg.export()
    Y = X.copy()
    Y[n - 1, col] = np.float32(bad)
    Y[7, col + 5] = np.float32(bad)                  # a later column as well: the first is named
    hb = H.Hgraph(Y, hg.deg0, hg.nbr0, upper=hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree)
    info0 = hb.info()
    assert H.load().hnsw_index_set_option(hb.handle, b"bit_rows", mode) == H.ERR_UNSUPPORTED
    assert ("column %d" % col) in H.load().hnsw_last_error().decode()
    info1 = hb.info()
    assert info1.row_format == info0.row_format and info1.device_bytes == info0.device_bytes
    with pytest.raises(H.InvalidArgument):
        hb.bit_params()
    hb.release()
    hg.release()


# ---- 2. the walk is the twin's ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def worlds(H):
    """per (d, metric): ONE index (built once), searched in either mode; per mode its float32 L2 twin over S, the queries both ways"""
    made, twins = {}, {}

    def get(d, metric, mode):
        if (d, metric) not in made:
            nq = 24
            X, Q = _table(N, d, 10 + d), _table(nq, d, 20 + d, cols=10 + d)
            if metric == H.METRIC_IP:        # rows of one length: an inner-product graph over rows of any length has hubs and does not reach ef nodes
                X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
            hg = H.Ohnsw.build_batch_bigarray(X, 6, 30, seed=3, metric=metric)
            made[(d, metric)] = (hg, hg.rows(), Q, H.normalise(Q) if metric == H.METRIC_COSINE else Q)
        hg, Xs, Q, Qn = made[(d, metric)]
        hg.set_option("bit_rows", mode)
        assert hg.info().row_format == ROWS_BITS
        if (d, metric, mode) not in twins:
            t, _ = _check_copy(hg, Xs, mode)
            twins[(d, metric, mode)] = (_twin(H, hg, _pm(Xs, t)), _pm(Qn, t))
        twin, Qs = twins[(d, metric, mode)]
        return {"hg": hg, "twin": twin, "Q": Q, "Qs": Qs, "Qn": Qn, "Xs": Xs, "metric": metric}
    yield get
    for twin, _ in twins.values():
        twin.release()
    for hg, _, _, _ in made.values():
        hg.release()


def _kinds(H):
    # COSINE in mode 2 only: mode 1 would hang a bit-exact claim on numpy restating the device's normalisation
    return [(H.METRIC_L2, 1), (H.METRIC_L2, 2), (H.METRIC_IP, 1), (H.METRIC_IP, 2), (H.METRIC_COSINE, 2)]


@pytest.mark.parametrize("kind", range(5), ids=["l2-means", "l2-signs", "ip-means", "ip-signs", "cosine-signs"])
@pytest.mark.parametrize("d", DIMS)
def test_walk_is_the_float32_l2_twin_over_the_signs(H, oracle, worlds, d, kind):
    metric, mode = _kinds(H)[kind]
    w = worlds(d, metric, mode)
    w["hg"].set_option("order_queries", 0)
    _pin_visited(w["hg"], w["twin"])
    _check_against_twin(H, oracle, w, [(sem, ef) for sem in (0, 1) for ef in EFS], "d %d metric %d mode %d" % (d, metric, mode))


@pytest.mark.parametrize("kind", [1, 4], ids=["l2-signs", "cosine-signs"])
@pytest.mark.parametrize("d", DIMS)
def test_walk_with_visited_blocks(H, oracle, worlds, d, kind):
    """ef > 128 (W in three or more registers): the bitmap-block kernel of the format.  n = 3000 nodes are 12 blocks of 256 codes in a
    directory of at least 64 slots, eight ways: nothing is ever evicted, so both handles evaluate every node at most once whatever
    their locality codes are, and the counts still agree"""
    metric, mode = _kinds(H)[kind]
    w = worlds(d, metric, mode)
    w["hg"].set_option("order_queries", 0)
    _pin_visited(w["hg"], w["twin"], blocks=1)
    try:
        assert all(w["hg"].visited_blocks(ef) >= 6 and w["twin"].visited_blocks(ef) >= 6 for ef in EFS[2:])
        _check_against_twin(H, oracle, w, [(sem, ef) for sem in (0, 1) for ef in EFS[2:]], "blocks d %d metric %d" % (d, metric))
    finally:
        _pin_visited(w["hg"], w["twin"])


@pytest.mark.parametrize("d", DIMS)
def test_walk_behind_the_ordering_pre_pass(H, oracle, worlds, d):
    """order_queries 1: the descent runs in the pre-pass kernel, over the bits as well"""
    w = worlds(d, H.METRIC_IP, 2)
    _pin_visited(w["hg"], w["twin"])
    w["hg"].set_option("order_queries", 1)
    try:
        _check_against_twin(H, oracle, w, [(0, 40), (1, 128), (0, 192), (1, 1024)], "ordered d %d" % d)
    finally:
        w["hg"].set_option("order_queries", 0)


@pytest.mark.parametrize("d", [100, 1024])
def test_walk_through_knn_and_two_requests_in_flight(H, oracle, worlds, d):
    w = worlds(d, H.METRIC_L2, 1)
    hg, Q = w["hg"], w["Q"]
    _pin_visited(hg, w["twin"])

    def submitted(ef, k, sem):
        r1 = H.submit(hg, Q[:10], ef, k, fill=H.FILL_BA if sem else H.FILL_OHNSW, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)
        r2 = H.submit(hg, Q[10:], ef, k, fill=H.FILL_BA if sem else H.FILL_OHNSW, sem=H.SEM_FUNCTOR if sem else H.SEM_OHNSW)
        b, a = r2.wait(counters=True), r1.wait(counters=True)
        return tuple(np.concatenate([x, y]) for x, y in zip(a, b))
    _check_against_twin(H, oracle, w, [(0, 128), (1, 192)], "submit d %d" % d, entry=submitted)
    hg.set_option("refine", -1)
    ids, dist, _, _ = _search(H, hg, Q, 64, 10, 0)
    for q in (0, 7, 23):
        one = H.Ohnsw.knn(hg, 10, Q[q], ef=64)
        assert [i for i, _ in one] == list(ids[q]) and [np.float32(x).view(np.uint32) for _, x in one] == list(dist[q].view(np.uint32))
    hg.set_option("refine", 0)


# ---- 3. the re-rank never costs a query recall -----------------------------------------------------------------------------------

def test_reranking_all_of_w_never_lowers_a_querys_recall(H):
    """refine -1 re-scores all ef members of W, refine 0 the first k by Hamming distance: the same W, so with no tie at the k-th
    place of the exact answer a query's recall@k cannot fall.  Exact, no threshold."""
    n, d, k, ef = N, 96, 10, 128
    X, pool = _table(n, d, 81), _table(200, d, 82, cols=81)
    D = ((pool.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    D.sort(axis=1)
    clear = (D[:, k] - D[:, k - 1]) > 1e-4 * D[:, k]      # float32 distances (relative error ~ d * 2^-24 = 6e-6) cannot tie or swap there
    Q = pool[clear]
    assert len(Q) >= 100
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=2)
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]
    for mode in (1, 2):
        hg.set_option("bit_rows", mode)
        hg.set_option("refine", 0)
        first = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
        hg.set_option("refine", -1)
        every = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)[0]
        r0 = np.array([len(set(a) & set(b)) for a, b in zip(first, truth)])
        r1 = np.array([len(set(a) & set(b)) for a, b in zip(every, truth)])
        print("mode %d: recall@%d %.4f at refine 0, %.4f at refine -1" % (mode, k, r0.mean() / k, r1.mean() / k))
        assert (r1 >= r0).all()
        assert r1.sum() > r0.sum()
    hg.set_option("refine", 0)
    hg.release()


# ---- 4. life cycle ---------------------------------------------------------------------------------------------------------------

def test_option_values_and_exclusions(H, tmp_path):
    n, d = 1500, 100
    X, Q = _table(n, d, 50), _table(30, d, 51, cols=50)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    L = H.load()
    rows0, bytes0 = hg.info().row_format, hg.info().device_bytes
    assert rows0 == ROWS_SPLIT and hg.row_bytes() == 4 * d
    before = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    for call in (hg.bit_params, hg.bit_codes):
        with pytest.raises(H.InvalidArgument, match="bit"):
            call()                                   # the option is off
    for bad in (3, -1, 7):
        assert L.hnsw_index_set_option(hg.handle, b"bit_rows", bad) == H.ERR_BAD_ARG
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0
    copy = _copy_bytes(n, d)
    for mode in (1, 2, 1):
        hg.set_option("bit_rows", mode)
        assert hg.info().row_format == ROWS_BITS and hg.row_bytes() == (d + 7) // 8 and hg.info().device_bytes == bytes0 + copy
        _check_copy(hg, X, mode)
    on = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, on[0]).view(np.uint32), on[1].view(np.uint32))
    with pytest.raises(H.InvalidArgument, match="bit_rows"):
        H._search(hg, Q, 100, 10, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K)
    # the four options it excludes, while it is on: refused, nothing moves
    for other in ("half_rows", "sq8_rows", "sq8_dim_rows", "filter_collect"):
        assert L.hnsw_index_set_option(hg.handle, other.encode(), 1) == H.ERR_BAD_ARG, other
        assert "bit_rows" in L.hnsw_last_error().decode()
        assert hg.info().row_format == ROWS_BITS and hg.info().device_bytes == bytes0 + copy
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), on)
    hg.set_option("bit_rows", 1)                     # again: nothing changes
    assert hg.info().device_bytes == bytes0 + copy
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), on)
    # 0: the previous rows, the previous bytes, results as if the option had never been set
    hg.set_option("bit_rows", 0)
    assert hg.info().row_format == rows0 and hg.row_bytes() == 4 * d and hg.info().device_bytes == bytes0
    with pytest.raises(H.InvalidArgument, match="bit"):
        hg.bit_codes()
    after = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100, counters=True)
    _same(after[:2], before[:2])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    # the reverse: refused while one of the four is on; the index stays as that option left it
    for other, rows in (("half_rows", ROWS_HALF), ("sq8_rows", ROWS_SQ8), ("sq8_dim_rows", ROWS_SQ8_DIM), ("filter_collect", rows0)):
        hg.set_option(other, 1)
        held = hg.info().device_bytes
        kept = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100)
        for mode in (1, 2):
            assert L.hnsw_index_set_option(hg.handle, b"bit_rows", mode) == H.ERR_BAD_ARG, other
            assert other in L.hnsw_last_error().decode()
        assert hg.info().row_format == rows and hg.info().device_bytes == held
        _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), kept)
        hg.set_option(other, 0 if other == "filter_collect" else -1)
    assert hg.info().row_format == rows0 and hg.info().device_bytes == bytes0
    _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=100), before[:2])
    # not saved
    hg.set_option("bit_rows", 2)
    path = os.path.join(str(tmp_path), "index.hnsw")
    hg.save(path)
    back = H.Hgraph.load(path)
    assert back.info().row_format == rows0
    with pytest.raises(H.InvalidArgument, match="bit"):
        back.bit_codes()
    _same(H.Ohnsw.knn_batch_bigarray(back, 10, Q, ef=100), before[:2])
    back.release()
    hg.release()


def test_refused_with_byte_rows_in_use(H):
    X = np.random.default_rng(3).integers(0, 256, size=(800, 64)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    assert hg.info().row_format == ROWS_BYTES
    bytes0 = hg.info().device_bytes
    for mode in (1, 2):
        with pytest.raises(H.InvalidArgument, match="byte rows"):
            hg.set_option("bit_rows", mode)
    assert hg.info().row_format == ROWS_BYTES and hg.info().device_bytes == bytes0
    hg.release()


@pytest.mark.parametrize("mode", [1, 2])
def test_insert_and_remove_quantise_the_table_again(H, mode):
    n0, m, d, nq = 1200, 300, 72, 24
    X = _table(n0 + m, d, 90)
    X[n0:] += np.float32(1.5)                                                  # the new vectors move the means
    Q = X[n0:n0 + nq] + (np.random.default_rng(91).normal(size=(nq, d)) * 0.01).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X[:n0], 10, 40, seed=5)
    hg.set_option("bit_rows", mode)
    hg.set_option("refine", -1)
    t0, _ = _check_copy(hg, X[:n0], mode)
    H.Ohnsw.insert_batch(hg, X[n0:], 10, 40, seed=5)
    assert hg.n == n0 + m and hg.info().row_format == ROWS_BITS
    t1, _ = _check_copy(hg, X, mode)
    if mode == 1:
        assert (t1 > t0).all()                                                 # the means moved
    ids, dist = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64)
    assert (ids >= n0).any()                                                   # inserted vectors among the answers
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32))
    # a new vector that is not finite: nothing inserted, codes, thresholds and results as before
    codes, params, bytes0 = hg.bit_codes(), hg.bit_params(), hg.info().device_bytes
    for v in (np.nan, np.inf):
        Y = _table(40, d, 92)
        Y[39, d - 1] = v
        with pytest.raises(H.Failure, match="bit_rows"):
            H.Ohnsw.insert_batch(hg, Y, 10, 40, seed=5)
        inf = hg.info()
        assert inf.n == n0 + m and inf.row_format == ROWS_BITS and inf.device_bytes == bytes0
        np.testing.assert_array_equal(hg.bit_codes(), codes)
        np.testing.assert_array_equal(hg.bit_params().view(np.uint32), params.view(np.uint32))
        _same(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64), (ids, dist))
    # remove the shifted vectors again: the remaining table is quantised again
    H.Ohnsw.remove_batch(hg, np.arange(n0, n0 + m, dtype=np.int64))
    assert hg.n == n0 and hg.info().row_format == ROWS_BITS
    np.testing.assert_array_equal(hg.rows(), X[:n0])
    t2, _ = _check_copy(hg, X[:n0], mode)
    np.testing.assert_array_equal(t2.view(np.uint32), t0.view(np.uint32))     # (the same table, the same grid: the same means)
    hg.release()


def test_filtered_range_and_grouped_calls_answer_with_exact_distances(H):
    n, d, nq, k = 1500, 48, 40, 10
    X, Q = _table(n, d, 60), _table(nq, d, 61, cols=60)
    hg = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=8)
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)
    hg.set_option("bit_rows", 1)
    allow = np.random.default_rng(1).random(n) < 0.5
    ids, dist = H.Ohnsw.knn_batch_filtered(hg, k, Q, allow, ef=64)[:2]
    assert (ids >= 0).all() and allow[ids].all()
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, ids).view(np.uint32), dist.view(np.uint32))
    radius = float(np.median(truth[1][:, -1]))
    lims, rids, rdist = H.Ohnsw.range_search(hg, radius, Q, ef=64)[:3]
    assert lims[-1] > 0
    for q in range(nq):
        seg = slice(int(lims[q]), int(lims[q + 1]))
        if seg.stop > seg.start:
            want = H.Ohnsw.distance_l2(hg, Q[q:q + 1], rids[seg].astype(np.int32)[None, :])[0]
            np.testing.assert_array_equal(want.view(np.uint32), rdist[seg].view(np.uint32))
            assert (rdist[seg] <= np.float32(radius)).all()
    lab = np.random.default_rng(41).integers(-1, 40, n).astype(np.int32)
    labels = hg.labels(lab, 40)
    got = H.Ohnsw.knn_batch_grouped(hg, k, Q, labels, ef=32, counters=True)
    np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, got[0]).view(np.uint32), got[1].view(np.uint32))
    assert (np.diff(got[1], axis=1) >= 0).all()
    np.testing.assert_array_equal(lab[got[0]], got[2])
    assert all(len(set(r)) == k for r in got[2])
    labels.release()
    hg.release()


def test_sharded_option_equals_the_merge_of_the_shards(H):
    n, d, nq, k, ef = 2000, 48, 64, 10, 64
    X, Q = _table(n, d, 62), _table(nq, d, 63, cols=62)
    s = H.ShardedHgraph.build(X, 10, 40, [0, 0], seed=4)
    s.set_option("bit_rows", 1)
    ids, dist, first, ts = [], [], [], []
    for g in range(2):
        hg, lo = s.shard(g)
        assert hg.info().row_format == ROWS_BITS
        ts.append(_check_copy(hg, hg.rows(), 1)[0])                            # per-shard thresholds
        i, dd = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef)
        ids.append(i); dist.append(dd); first.append(lo)
    assert (ts[0] != ts[1]).any()
    want = H.merge_lists(np.stack(ids), np.stack(dist), first, k, id_base=s.id_base)
    got = s.knn_batch(Q, ef, k)
    _same(got[:2], want)
    s.set_option("bit_rows", 0)
    assert [s.shard(g)[0].info().row_format for g in range(2)] != [ROWS_BITS] * 2
    s.release()


def test_a_handle_that_never_set_the_option_is_untouched(H):
    n, d = 1500, 100
    X, Q = _table(n, d, 64), _table(30, d, 65, cols=64)
    plain = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    before = H.Ohnsw.knn_batch_bigarray(plain, 10, Q, ef=100, counters=True)
    other = H.Ohnsw.build_batch_bigarray(X, 10, 40, seed=6)
    other.set_option("bit_rows", 2)
    H.Ohnsw.knn_batch_bigarray(other, 10, Q, ef=100)
    after = H.Ohnsw.knn_batch_bigarray(plain, 10, Q, ef=100, counters=True)
    _same(after[:2], before[:2])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    other.release()
    plain.release()


# ---- 5. the C++ front end --------------------------------------------------------------------------------------------------------

def test_cpp_front_end_bits(H, tmp_path):
    exe = str(tmp_path / "test_front_bits")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_bits.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bits front-end ok" in out.stdout, out.stdout + out.stderr
