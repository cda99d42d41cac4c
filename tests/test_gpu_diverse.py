"""Diversified k-NN search (ocaml-hnsw_amd/csrc/hnsw_diverse.hip): hnsw_diversify_batch, hnsw_search_batch_diverse and
hnsw_brute_force_batch_diverse against the definition the header gives, restated in numpy below from calls that exist without them:
  rank, r  the row hnsw_rerank_batch returns at k = cand_stride (Ohnsw.rerank), r checked against hnsw_distance_batch;
  D        hnsw_distance_batch with hnsw_index_get_rows of the candidates as the queries (Hgraph.rows, Ohnsw.distance_l2);
  g        lambda * r - mu * m on np.float32 arrays: two products and one difference, each rounded.
Every comparison is exact: ids equal, distances and diversities bit-equal, counters equal."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.25, 0.5, 1.0)


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


# ---- the definition, in numpy ---------------------------------------------------------------------------------------------------------

class Pool:
    """what the selection of one query needs, from public calls: its real candidates in rank order (0-based nodes), r and D"""

    def __init__(self, H, hg, q, ranked_ids, ranked_dist):
        real = ranked_ids >= hg.id_base
        self.nodes = ranked_ids[real].astype(np.int64) - hg.id_base
        c = len(self.nodes)
        ids = (self.nodes + hg.id_base).astype(np.int32)
        self.r = H.Ohnsw.distance_l2(hg, q[None, :], ids[None, :])[0] if c else np.zeros(0, np.float32)
        # (rank's row carries the same floats)
        np.testing.assert_array_equal(self.r.view(np.uint32), ranked_dist[real].view(np.uint32))
        self.D = H.Ohnsw.distance_l2(hg, hg.rows(ids), np.broadcast_to(ids, (c, c))) if c else np.zeros((0, 0), np.float32)


def pools(H, hg, Q, cand):
    """one Pool per query: rank from hnsw_rerank_batch at k = cand_stride"""
    rid, rdist = H.Ohnsw.rerank(hg, cand.shape[1], Q, cand)
    return [Pool(H, hg, Q[q], rid[q], rdist[q]) for q in range(len(Q))]


def select(pool, k, lam):
    """the greedy rule over one pool -> (picks as ranks, m at the moment of selection)"""
    c = len(pool.nodes)
    lam32 = np.float32(lam)
    mu32 = np.float32(1.0) - lam32
    picks, div = [], []
    if c == 0:
        return picks, div
    free = np.ones(c, bool)
    m = np.full(c, np.inf, np.float32)
    picks.append(0)
    div.append(np.float32(np.inf))
    free[0] = False
    while len(picks) < min(k, c):
        m = np.minimum(m, pool.D[picks[-1]])
        left = np.flatnonzero(free)
        a = lam32 * pool.r[left]                      # float32 arrays: each operation rounded on its own
        b = mu32 * m[left]
        g = a - b
        assert g.dtype == np.float32 and a.dtype == np.float32 and b.dtype == np.float32
        j = left[np.argmin(g)]                        # IEEE compare (-0 == +0); the first minimum = the smallest rank
        picks.append(int(j))
        div.append(m[j])
        free[j] = False
    return picks, div


def expect_rows(pool_list, k, lam, id_base, fill=np.nan):
    nq = len(pool_list)
    ids = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), fill, np.float32)
    div = np.full((nq, k), fill, np.float32)
    for q, p in enumerate(pool_list):
        picks, dv = select(p, k, lam)
        ids[q, :len(picks)] = p.nodes[picks] + id_base
        dist[q, :len(picks)] = p.r[picks]
        div[q, :len(picks)] = dv
    return ids, dist, div


def same_rows(got, want, ctx=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx + " ids")
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx + " distance bits")
    np.testing.assert_array_equal(got[2].view(np.uint32), want[2].view(np.uint32), err_msg=ctx + " diversity bits")


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _cands(rng, nq, stride, n, id_base, ragged_rows=()):
    """distinct ids per row; the rows named carry -1 entries in arbitrary positions"""
    c = np.stack([rng.permutation(n)[:stride] for _ in range(nq)]).astype(np.int32) + id_base
    for q in ragged_rows:
        c[q, rng.random(stride) < 0.4] = -1
        c[q, rng.integers(stride)] = -1
    return c


def _metric(H, name):
    return {"l2": H.METRIC_L2, "ip": H.METRIC_IP, "cosine": H.METRIC_COSINE}[name]


# ---- 1. the operator against the reference ----------------------------------------------------------------------------------------------

_flat_cache = {}


def _flat(H, metric, d, n, id_base):
    key = (metric, d, n, id_base)
    if key not in _flat_cache:
        X = _floats(n, d, 100 + d + n)
        _flat_cache[key] = (H.Hgraph.flat(X, metric=_metric(H, metric), id_base=id_base), X)
    return _flat_cache[key]


@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("stride", [1, 2, 63, 64, 65, 200, 1024])
@pytest.mark.parametrize("d", [4, 100, 128, 260])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_operator_against_the_reference(H, metric, d, stride, id_base):
    """ragged chunks and every NCH a small d reaches, strides around the wave width and up to 1024, k in {1, 10, cand_stride} (the last
    round then has one candidate left), every lambda, both fills (a ragged row is short at k = cand_stride)"""
    n = 1100 if stride == 1024 else 300
    nq = 3 if stride == 1024 else 5
    hg, _ = _flat(H, metric, d, n, id_base)
    rng = np.random.default_rng(1000 * d + stride + id_base)
    Q = _floats(nq, d, 7 * d + stride)
    cand = _cands(rng, nq, stride, n, id_base, ragged_rows=(nq - 1,))
    pl = pools(H, hg, Q, cand)
    for k in sorted({1, min(10, stride), stride}):
        for lam in LAMBDAS:
            for fill, ff in ((H.FILL_OHNSW, np.nan), (H.FILL_BA, np.inf)) if k == stride else ((H.FILL_OHNSW, np.nan),):
                got = H.Ohnsw.diversify(hg, k, Q, cand, lam, fill=fill)
                same_rows(got, expect_rows(pl, k, lam, id_base, ff), "%s d=%d stride=%d k=%d lambda=%g fill=%d" % (metric, d, stride, k, lam, fill))
    assert len(pl[-1].nodes) < stride       # (the ragged row really was short)


# ---- 2. ties -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_are_broken_by_rank(H, metric):
    """integer data in 0..3 at d = 4, every row stored three times, lambda = 0.5: many equal g and equal r, so the order must be the
    reference's (g, rank)"""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 4, size=(100, 4)).astype(np.float32)
    X = np.concatenate([base, base, base])
    hg = H.Hgraph.flat(X, metric=_metric(H, metric))
    Q = rng.integers(0, 4, size=(6, 4)).astype(np.float32)
    ties = 0
    for stride in (64, 200):
        cand = _cands(rng, len(Q), stride, len(X), 0)
        pl = pools(H, hg, Q, cand)
        for k in (10, stride):
            same_rows(H.Ohnsw.diversify(hg, k, Q, cand, 0.5), expect_rows(pl, k, 0.5, 0), "%s stride=%d k=%d" % (metric, stride, k))
        ties += sum(len(p.r) - len(np.unique(p.r)) for p in pl)
    assert ties > 100                       # (the data did tie)
    hg.release()


# ---- 3. lambda = 1 is the re-rank; lambda = 0 leaves exact duplicates for last -----------------------------------------------------

@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_lambda_one_is_rerank(H, metric):
    hg, _ = _flat(H, metric, 100, 300, 0)
    rng = np.random.default_rng(11)
    Q = _floats(9, 100, 12)
    cand = _cands(rng, 9, 65, 300, 0, ragged_rows=(2, 5))
    for k in (1, 10, 65):
        ids, dist, _ = H.Ohnsw.diversify(hg, k, Q, cand, 1.0)
        rid, rdist = H.Ohnsw.rerank(hg, k, Q, cand)
        np.testing.assert_array_equal(ids, rid)
        np.testing.assert_array_equal(dist.view(np.uint32), rdist.view(np.uint32))


def test_lambda_zero_picks_exact_duplicates_last(H):
    """three exact copies of the nearest node in the pool, lambda = 0 (g = -m): one copy is pick 1, the others have m = 0 from then on
    and every other candidate m > 0, so they are the last picks and their out_div is 0 under L2"""
    rng = np.random.default_rng(21)
    X = _floats(200, 16, 22)
    X[150] = X[7]
    X[199] = X[7]
    hg = H.Hgraph.flat(X)
    Q = (X[7] + 0.01 * rng.normal(size=16).astype(np.float32))[None, :]
    pool, _ = H.Ohnsw.brute_force_knn(hg, 20, Q)
    assert set(pool[0][:3].tolist()) == {7, 150, 199}
    ids, dist, div = H.Ohnsw.diversify(hg, 20, Q, pool, 0.0)
    same_rows((ids, dist, div), expect_rows(pools(H, hg, Q, pool), 20, 0.0, 0))
    assert ids[0][0] == 7 and sorted(ids[0][-2:].tolist()) == [150, 199]
    assert div[0][0] == np.inf and (div[0][-2:] == 0).all() and (div[0][1:-2] > 0).all()
    hg.release()


# ---- 4. padding ----------------------------------------------------------------------------------------------------------------------

def test_padding_short_rows_and_ids_past_the_table(H):
    import torch
    n, d, stride, k = 300, 24, 40, 12
    hg, _ = _flat(H, "l2", d, n, 1)
    rng = np.random.default_rng(31)
    Q = _floats(6, d, 32)
    cand = _cands(rng, 6, stride, n, 1, ragged_rows=(0, 1, 2))
    cand[3, 5:] = -1                     # fewer than k real candidates
    cand[3, :5] = cand[3, :5][::-1]
    cand[4, :] = 0                       # padding only (ids below id_base = 1), 0 and -1 alike
    cand[4, ::2] = -1
    pl = pools(H, hg, Q, cand)
    assert len(pl[3].nodes) == 5 and len(pl[4].nodes) == 0
    for fill, ff in ((H.FILL_OHNSW, np.nan), (H.FILL_BA, np.inf)):
        got = H.Ohnsw.diversify(hg, k, Q, cand, 0.5, fill=fill)
        same_rows(got, expect_rows(pl, k, 0.5, 1, ff), "fill %d" % fill)
        assert (got[0][4] == -1).all() and (got[0][3][5:] == -1).all()
    # the host form refuses an id past the table, naming it, outputs untouched
    bad = cand.copy()
    bad[2, 7] = n + 1                    # (id_base + n: the first id past the table)
    with pytest.raises(H.InvalidArgument, match="candidate id %d out of range" % (n + 1)):
        H.Ohnsw.diversify(hg, k, Q, bad, 0.5)
    # the device form skips it: the rows of the candidates with those entries as padding
    past = cand.copy()
    holes = cand < 1
    past[holes] = np.where(np.arange(holes.sum()) % 2, n + 1, n + 12345)
    dev = torch.device("cuda", 0)
    Qd, Cd = torch.from_numpy(Q).to(dev), torch.from_numpy(past).to(dev)
    ids = torch.empty((6, k), dtype=torch.int32, device=dev)
    dd = torch.empty((6, k), dtype=torch.float32, device=dev)
    dv = torch.empty((6, k), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        H.diversify_device(hg, Qd.data_ptr(), 6, d, Cd.data_ptr(), stride, k, 0.5, ids.data_ptr(), dd.data_ptr(), dv.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    same_rows((ids.cpu().numpy(), dd.cpu().numpy(), dv.cpu().numpy()), expect_rows(pl, k, 0.5, 1), "device form")
    # ... and without out_div
    ids.fill_(-7)
    with torch.cuda.stream(st):
        H.diversify_device(hg, Qd.data_ptr(), 6, d, Cd.data_ptr(), stride, k, 0.5, ids.data_ptr(), dd.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(ids.cpu().numpy(), expect_rows(pl, k, 0.5, 1)[0])


def test_refusals_with_a_handle_leave_the_outputs_untouched(H):
    import ctypes
    hg, _ = _flat(H, "l2", 24, 300, 1)
    L = H.load()
    Q = _floats(2, 24, 41)
    cand = np.arange(1, 17, dtype=np.int32).reshape(2, 8)
    ids, dist, div = np.full((2, 4), -7, np.int32), np.full((2, 4), 7, np.float32), np.full((2, 4), 7, np.float32)
    P = H._ptr

    def call(q=Q, nq=2, qs=24, c=cand, stride=8, k=4, lam=0.5, fill=0, oi=ids, od=dist):
        return L.hnsw_diversify_batch(hg.handle, P(q), nq, qs, P(c), stride, k, ctypes.c_float(lam), fill, P(oi), P(od), P(div))
    assert call(q=None) == H.ERR_BAD_ARG and call(c=None) == H.ERR_BAD_ARG and call(oi=None) == H.ERR_BAD_ARG and call(od=None) == H.ERR_BAD_ARG
    assert call(nq=-1) == H.ERR_BAD_ARG and call(qs=23) == H.ERR_BAD_ARG
    assert call(stride=0) == H.ERR_BAD_ARG and call(stride=1025) == H.ERR_UNSUPPORTED
    assert call(k=0) == H.ERR_BAD_ARG and call(k=9) == H.ERR_BAD_ARG and call(fill=2) == H.ERR_BAD_ARG
    for lam in (np.nan, -0.1, 1.5):
        assert call(lam=lam) == H.ERR_BAD_ARG and b"lambda" in L.hnsw_last_error()
    assert call(nq=0) == H.OK                                   # a no-op
    assert (ids == -7).all() and (dist == 7).all() and (div == 7).all()
    assert call() == H.OK and (ids >= 1).all() and np.isinf(div[:, 0]).all()
    assert L.hnsw_diversify_batch(hg.handle, P(Q), 2, 24, P(cand), 8, 4, ctypes.c_float(0.5), 0, P(ids), P(dist), None) == H.OK   # out_div may be null


# ---- 5. a query's row depends on its own candidates only ---------------------------------------------------------------------------

def test_batch_independence(H):
    hg, _ = _flat(H, "ip", 100, 300, 0)
    rng = np.random.default_rng(51)
    Q = _floats(70, 100, 52)
    cand = _cands(rng, 70, 48, 300, 0, ragged_rows=range(0, 70, 7))
    ids, dist, div = H.Ohnsw.diversify(hg, 10, Q, cand, 0.25)
    for q in range(70):
        one = H.Ohnsw.diversify(hg, 10, Q[q:q + 1], cand[q:q + 1], 0.25)
        same_rows(one, (ids[q:q + 1], dist[q:q + 1], div[q:q + 1]), "query %d alone" % q)
    same_rows((ids[:3], dist[:3], div[:3]), expect_rows(pools(H, hg, Q[:3], cand[:3]), 10, 0.25, 0))


# ---- 6. COSINE: the twin contract ------------------------------------------------------------------------------------------------

def test_cosine_equals_the_ip_twin(H):
    X = _floats(300, 100, 61) * np.random.default_rng(62).uniform(0.1, 9.0, size=(300, 1)).astype(np.float32)
    Q = _floats(8, 100, 63) * 3.0
    hc = H.Hgraph.flat(X, metric=H.METRIC_COSINE)
    hi = H.Hgraph.flat(hc.rows(), metric=H.METRIC_IP)
    NQ = H.normalise(Q)
    rng = np.random.default_rng(64)
    cand = _cands(rng, 8, 65, 300, 0, ragged_rows=(1,))
    pl = pools(H, hi, NQ, cand)
    for lam in LAMBDAS:
        got = H.Ohnsw.diversify(hc, 10, Q, cand, lam)
        same_rows(got, H.Ohnsw.diversify(hi, 10, NQ, cand, lam), "cosine against the twin, lambda %g" % lam)
        same_rows(got, expect_rows(pl, 10, lam, 0), "cosine against the reference over the twin, lambda %g" % lam)
    same_rows(H.Ohnsw.brute_force_diverse(hc, 10, Q, 40, 0.5), H.Ohnsw.brute_force_diverse(hi, 10, NQ, 40, 0.5), "the exact search")
    hc.release()
    hi.release()


# ---- 7. the searches are compositions ----------------------------------------------------------------------------------------------

N, D_, EF, K = 1000, 100, 64, 10


@pytest.fixture(scope="module")
def world(H):
    X = _floats(N, D_, 71)
    X[500:520] = X[0:20]                 # near-duplicates worth diversifying away
    Q = np.concatenate([X[0:20] + 0.05 * _floats(20, D_, 72), _floats(20, D_, 73)])
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    yield hg, X, Q
    hg.release()


def _composed(H, hg, Q, pool, lam, inner):
    """the inner call at k = pool, then the operator over its id rows"""
    res = inner(pool)
    return H.Ohnsw.diversify(hg, K, Q, res[0], lam), res[2:]


@pytest.mark.parametrize("pool", [10, 64])
def test_search_is_the_plain_search_then_the_operator(H, world, pool):
    hg, _, Q = world
    for lam in (0.25, 0.5, 1.0):
        want, counters = _composed(H, hg, Q, pool, lam, lambda p: H.Ohnsw.knn_batch_bigarray(hg, p, Q, ef=EF, counters=True))
        got = H.Ohnsw.knn_batch_diverse(hg, K, Q, pool, lam, ef=EF, counters=True)
        same_rows(got, want, "pool %d lambda %g" % (pool, lam))
        np.testing.assert_array_equal(got[3], counters[0])
        np.testing.assert_array_equal(got[4], counters[1])
        assert (got[5] == 0).all()
    # the functor's accept rule and fill
    ids, _ = H._search(hg, Q, EF, pool, H.FILL_BA, sem=H.SEM_FUNCTOR)
    want = H.Ohnsw.diversify(hg, K, Q, ids, 0.5, fill=H.FILL_BA)
    same_rows(H.Ba.knn_batch_diverse(hg, Q, EF, K, pool, 0.5), want, "functor, pool %d" % pool)
    if pool == 64:                       # the duplicates are near the head of the pool and lambda = 0.25 moves them down the row
        plain = H.Ohnsw.knn_batch_bigarray(hg, K, Q, ef=EF)[0]
        assert (H.Ohnsw.knn_batch_diverse(hg, K, Q, pool, 0.25, ef=EF)[0] != plain).any()


@pytest.mark.parametrize("pool", [10, 64])
def test_search_under_a_filter(H, world, pool):
    hg, _, Q = world
    rng = np.random.default_rng(81)
    for allow in (rng.random(N) < 0.3, np.isin(np.arange(N), rng.permutation(N)[:7])):       # selectivity 0.3; fewer than the pool allowed
        f = hg.filter(allow)
        want, counters = _composed(H, hg, Q, pool, 0.5, lambda p: H.Ohnsw.knn_batch_filtered(hg, p, Q, f, ef=EF, counters=True))
        got = H.Ohnsw.knn_batch_diverse(hg, K, Q, pool, 0.5, ef=EF, filter=f, counters=True)
        same_rows(got, want, "pool %d, %d allowed" % (pool, allow.sum()))
        for a, b in zip(got[3:], counters):
            np.testing.assert_array_equal(a, b)
        real = got[0][got[0] >= 0]
        assert allow[real].all()
        if allow.sum() < K:
            assert (got[0][:, allow.sum():] == -1).all() and (got[5] == 0xFFFFFFFF).all()
        f.release()


def test_search_on_a_marked_index(H):
    X = _floats(N, D_, 71)
    Q = _floats(30, D_, 91)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    dead = np.random.default_rng(92).permutation(N)[:N // 20].astype(np.int32)
    hg.mark_deleted(dead)
    for pool in (10, 64):
        want, counters = _composed(H, hg, Q, pool, 0.5, lambda p: H.Ohnsw.knn_batch_bigarray(hg, p, Q, ef=EF, counters=True))
        got = H.Ohnsw.knn_batch_diverse(hg, K, Q, pool, 0.5, ef=EF, counters=True)
        same_rows(got, want, "marked, pool %d" % pool)
        np.testing.assert_array_equal(got[3], counters[0])
        np.testing.assert_array_equal(got[4], counters[1])
        assert not np.isin(got[0], dead).any() and (got[0] >= 0).all()
        bf = H.Ohnsw.brute_force_diverse(hg, K, Q, pool, 0.5)
        same_rows(bf, H.Ohnsw.diversify(hg, K, Q, H.Ohnsw.brute_force_knn(hg, pool, Q)[0], 0.5), "marked, exact, pool %d" % pool)
        assert not np.isin(bf[0], dead).any()
    hg.release()


@pytest.mark.parametrize("rows", ["half", "sq8"])
def test_search_over_inexact_rows(H, rows):
    """half_rows + refine -1 and sq8_rows: the inner call re-ranks over the float32 rows, the selection's distances are theirs"""
    X = _floats(N, D_, 71)
    Q = _floats(30, D_, 101)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=1)
    if rows == "half":
        hg.set_option("half_rows", 1)
        hg.set_option("refine", -1)
    else:
        hg.set_option("sq8_rows", 1)
    for pool in (10, 64):
        want, counters = _composed(H, hg, Q, pool, 0.5, lambda p: H.Ohnsw.knn_batch_bigarray(hg, p, Q, ef=EF, counters=True))
        got = H.Ohnsw.knn_batch_diverse(hg, K, Q, pool, 0.5, ef=EF, counters=True)
        same_rows(got, want, "%s rows, pool %d" % (rows, pool))
        np.testing.assert_array_equal(got[3], counters[0])
        np.testing.assert_array_equal(got[4], counters[1])
        exact = H.Ohnsw.distance_l2(hg, Q, got[0])          # over the float32 rows whatever row_format says
        np.testing.assert_array_equal(got[1].view(np.uint32), exact.view(np.uint32))
    hg.release()


@pytest.mark.parametrize("pool", [10, 64, 1024])
def test_exact_search_is_the_scan_then_the_operator(H, world, pool):
    hg, _, Q = world
    Q = Q[:12]
    for fill in (H.FILL_OHNSW, H.FILL_BA):
        pids, _ = H.Ohnsw.brute_force_knn(hg, pool, Q, fill=fill)
        want = H.Ohnsw.diversify(hg, K, Q, pids, 0.5, fill=fill)
        same_rows(H.Ohnsw.brute_force_diverse(hg, K, Q, pool, 0.5, fill=fill), want, "pool %d fill %d" % (pool, fill))
    if pool == 1024:
        assert (pids[:, N:] == -1).all()                    # (the scan's rows of -1 were the padding)


def test_pool_limits_are_refused(H, world):
    hg, _, Q = world
    with pytest.raises(H.InvalidArgument, match="pool must lie in k..ef"):
        H.Ohnsw.knn_batch_diverse(hg, K, Q, EF + 1, 0.5, ef=EF)
    with pytest.raises(H.InvalidArgument, match="pool must lie in k..ef"):
        H.Ohnsw.knn_batch_diverse(hg, K, Q, K - 1, 0.5, ef=EF)
    with pytest.raises(H.Failure, match="pool=1025 > 1024"):
        H.Ohnsw.knn_batch_diverse(hg, K, Q, 1025, 0.5, ef=1025)
    with pytest.raises(H.InvalidArgument, match="pool must lie in k..1024"):
        H.Ohnsw.brute_force_diverse(hg, K, Q, K - 1, 0.5)
    with pytest.raises(H.Failure, match="pool=1025 > 1024"):
        H.Ohnsw.brute_force_diverse(hg, K, Q, 1025, 0.5)
    with pytest.raises(H.InvalidArgument, match="lambda"):
        H.Ohnsw.knn_batch_diverse(hg, K, Q, 32, 1.5, ef=EF)
    ids, dist, div = H.Ohnsw.knn_batch_diverse(hg, K, Q[:0], 32, 0.5, ef=EF)       # nq == 0: a no-op
    assert ids.shape == (0, K)


# ---- 8. after a mutation the operator reads the new table -------------------------------------------------------------------------

def test_after_insert_and_after_remove(H):
    X = _floats(400, 24, 111)
    hg = H.Ohnsw.build_batch_bigarray(X[:300], 8, 40, seed=1)
    H.Ohnsw.insert_batch(hg, X[300:], 8, 40, seed=2)
    rng = np.random.default_rng(112)
    Q = _floats(5, 24, 113)
    cand = _cands(rng, 5, 65, 400, 0)
    cand[:, :8] = np.arange(392, 400)            # (among the new nodes)
    same_rows(H.Ohnsw.diversify(hg, 10, Q, cand, 0.5), expect_rows(pools(H, hg, Q, cand), 10, 0.5, 0), "after insert")
    H.Ohnsw.remove_batch(hg, np.arange(0, 400, 3, dtype=np.int32))
    n = hg.info().n
    assert n == 400 - 134
    cand = _cands(rng, 5, 65, n, 0)
    pl = pools(H, hg, Q, cand)
    same_rows(H.Ohnsw.diversify(hg, 10, Q, cand, 0.5), expect_rows(pl, 10, 0.5, 0), "after remove")
    kept = np.delete(np.arange(400), np.arange(0, 400, 3))
    np.testing.assert_array_equal(hg.rows(cand[0]), X[kept][cand[0]])      # (the table the reference read is the renumbered one)
    with pytest.raises(H.InvalidArgument, match="out of range"):
        H.Ohnsw.diversify(hg, 10, Q, np.full((5, 1), n, np.int32) + np.zeros((5, 65), np.int32), 0.5)
    hg.release()


# ---- 9. the C++ front end ------------------------------------------------------------------------------------------------------------

def test_cpp_front_end_diverse(H, tmp_path):
    from conftest import ROOT
    exe = str(tmp_path / "test_front_diverse")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_diverse.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "diverse front-end ok" in out.stdout, out.stdout + out.stderr
