"""Range search (ocaml-hnsw_amd/csrc/hnsw_range.hip): hnsw_range_search_batch, hnsw_range_brute_force_batch and the result object
against the definition the header gives, restated in numpy below over the oracle's walks and the oracle's exact scan.

W_e(q) comes from the oracle (float32 space, TREE16 summation, canonical ties, k := e); the ladder e = ef, 2 ef, ... 1024, the
stage test (W not saturated), the in-range prefix and the exact stage are `restate`.  The full order of a query is
oracle.brute_force_knn(space, Q, n): (ordered distance key, node id).  Every comparison is exact: ids equal, distances bit-equal.
The oracle reports no evaluation counts of the kernel (its visited cache re-evaluates forgotten nodes) and the functor search no
hops: out_ndist is held against the plain searches of the same handle (the same walks), out_nhops against the oracle's hops
under the Ohnsw rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_HALF, ROWS_SQ8 = 0, 2, 4, 5
EXACT = 0xFFFFFFFF
N, D, NQ = 2003, 20, 64
INF = float("inf")


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _ladder(ef):
    out = [ef]
    while out[-1] < 1024:
        out.append(min(1024, 2 * out[-1]))
    return out


class Walks:
    """W_e of every query, per (accept rule, e): (ids [nq][e] 0-based with -1 past |W|, distances, hops or None), computed once"""

    def __init__(self, oracle, g, space, Q):
        self.o, self.g, self.space, self.Q, self._w = oracle, g, space, np.asarray(Q, np.float32), {}

    def get(self, sem, e):
        if (sem, e) not in self._w:
            o = self.o
            if sem == 0:
                W, Wd, _, hops = o.Ohnsw.knn_batch_bigarray(self.g, self.space, self.Q, k=e, ef=e, ties=o.TIES_CANONICAL, counters=True)
            else:
                Wd, W = o.Functor.knn_batch(self.g, self.space, self.Q, e, e, ties=o.TIES_CANONICAL, with_ids=True)
                hops = None
            self._w[(sem, e)] = (np.asarray(W), np.asarray(Wd, np.float32), hops)
        return self._w[(sem, e)]


class Full:
    """the full order of every query over the float32 rows (oracle.brute_force_knn with k = n) and, from it, every pair's distance
    and rank"""

    def __init__(self, oracle, space, Q, n):
        self.ids, self.dist = oracle.brute_force_knn(space, Q, n) if n else (np.zeros((len(Q), 0), np.int32), np.zeros((len(Q), 0), np.float32))
        nq = len(Q)
        self.rank = np.empty((nq, n), np.int64)
        self.table = np.empty((nq, n), np.float32)
        rows = np.arange(nq)[:, None]
        self.rank[rows, self.ids] = np.arange(n)[None, :]
        self.table[rows, self.ids] = self.dist

    def prefix(self, q, radius):
        c = int((self.dist[q] <= np.float32(radius)).sum())
        assert (self.dist[q][:c] <= np.float32(radius)).all()           # the in-range nodes are a prefix of the order
        return self.ids[q][:c], self.dist[q][:c]


def restate(walks, full, radius, ef, sem, rerank=False):
    """The header's definition -> (segments [(ids 0-based, distances)], stages, hops summed (None under the functor rule),
    members re-ranked summed, walks taken).  rerank: the half / sq8 rule (all members of W re-ranked over the float32 rows: their
    order and distances from `full`)."""
    nq = len(walks.Q)
    r32 = np.float32(radius)
    segs, stage, taken = [None] * nq, np.full(nq, EXACT, np.uint32), [[] for _ in range(nq)]
    hops = np.zeros(nq, np.uint32) if sem == 0 else None
    reranked = np.zeros(nq, np.uint32)
    for q in range(nq):
        for j, e in enumerate(_ladder(ef)):
            W, Wd, hp = walks.get(sem, e)
            taken[q].append(e)
            if hops is not None:
                hops[q] += hp[q]
            real = W[q] >= 0
            ids, d = W[q][real].astype(np.int64), Wd[q][real]
            if rerank:
                o = np.argsort(full.rank[q][ids], kind="stable")
                ids = ids[o]
                d = full.table[q][ids]
                reranked[q] += len(ids)
            if not (len(ids) == e and d[-1] <= r32):                    # not saturated: served here
                c = int((d <= r32).sum())
                assert (d[:c] <= r32).all()
                segs[q], stage[q] = (ids[:c], d[:c]), j
                break
        else:
            segs[q] = full.prefix(q, radius)
    return segs, stage, hops, reranked, taken


def _same_segments(got, want, id_base=0, ctx=""):
    lims, ids, dist = got[:3]
    assert lims[0] == 0 and lims[-1] == len(ids) == len(dist), ctx
    np.testing.assert_array_equal(np.diff(lims), [len(s[0]) for s in want], err_msg=ctx + " segment lengths")
    wi = np.concatenate([s[0] for s in want] + [np.zeros(0, np.int64)]).astype(np.int64) + id_base
    wd = np.concatenate([s[1] for s in want] + [np.zeros(0, np.float32)]).astype(np.float32)
    np.testing.assert_array_equal(ids, wi, err_msg=ctx + " ids")
    np.testing.assert_array_equal(dist.view(np.uint32), wd.view(np.uint32), err_msg=ctx + " distance bits")


def _hist(stage):
    return dict(zip(*[a.tolist() for a in np.unique(stage, return_counts=True)]))


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """the index of the issue: 2003 Gaussian vectors of 20 dimensions, the oracle's graph (M 8, efC 40, seed 1), 64 queries"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.space = oracle.Space.l2(w.X, arith=oracle.TREE16)
    w.g = oracle.build_ohnsw(w.space, 8, 40, seed=1)
    w.hg = H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, id_base=0, max_degree=8)
    assert w.hg.info().row_format == ROWS_F32
    w.walks = Walks(oracle, w.g, w.space, w.Q)
    w.full = Full(oracle, w.space, w.Q, N)
    yield w
    w.hg.release()


def _plain_counts(H, hg, Q, taken, sem=0, minus_e=False):
    """evaluations of the walks each query took, from the plain searches of the same handle with (ef = e, k = e)"""
    cache, out = {}, np.zeros(len(Q), np.uint32)
    for q, es in enumerate(taken):
        for e in es:
            if e not in cache:
                cache[e] = H._search(hg, Q, e, e, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=sem)[2] - np.uint32(e if minus_e else 0)
            out[q] += cache[e][q]
    return out


def _check(H, hg, Q, want, got, n, sem=0, id_base=0, ctx="", minus_e=False):
    segs, stage, hops, reranked, taken = want
    print("%s: stages %s, segment lengths %d..%d" % (ctx, _hist(stage), min(len(s[0]) for s in segs), max(len(s[0]) for s in segs)))
    _same_segments(got, segs, id_base, ctx)
    np.testing.assert_array_equal(got[5], stage, err_msg=ctx + " stage")
    if hops is not None:
        np.testing.assert_array_equal(got[4], hops, err_msg=ctx + " hops")
    nd = _plain_counts(H, hg, Q, taken, sem, minus_e) + reranked + np.where(stage == EXACT, np.uint32(n), np.uint32(0))
    np.testing.assert_array_equal(got[3], nd, err_msg=ctx + " evaluations")


# ---- 1. the ladder -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius,sem", [(3.0, 0), (4.5, 0), (6.0, 0), (4.5, 1)])
def test_ladder(H, world, radius, sem):
    w = world
    want = restate(w.walks, w.full, radius, 16, sem)
    stage, lens = want[1], np.array([len(s[0]) for s in want[0]])
    # the classes this case is here for exist in the restatement itself
    if radius == 3.0:
        assert (lens == 0).any() and (stage == 0).any()
    elif radius == 4.5:
        assert (stage == 0).any() and ((stage >= 1) & (stage <= 3)).any() and ((stage >= 4) & (stage != EXACT)).any(), _hist(stage)
    else:
        assert (stage == EXACT).any() and (stage != EXACT).any(), _hist(stage)
        assert (lens[stage == EXACT] >= 1024).all()
    if sem == 0:
        got = H.Ohnsw.range_search(w.hg, radius, w.Q, ef=16, counters=True)
    else:
        got = H._range_search(w.hg, w.Q, radius, 16, H.SEM_FUNCTOR, True)
    _check(H, w.hg, w.Q, want, got, N, sem, ctx="radius %g rule %d" % (radius, sem))


# ---- 2. batch independence -----------------------------------------------------------------------------------------------------

def _segments(got):
    lims, ids, dist = got[:3]
    return [(ids[lims[q]:lims[q + 1]], dist[lims[q]:lims[q + 1]].view(np.uint32)) + tuple(c[q] for c in got[3:]) for q in range(len(lims) - 1)]


def test_result_does_not_depend_on_the_batch(H, world):
    w = world
    whole = _segments(H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=16, counters=True))
    assert len({int(s[4]) for s in whole}) > 1

    def same(a, b, ctx):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v, err_msg=ctx)

    for q in range(NQ):
        same(_segments(H.Ohnsw.range_search(w.hg, 4.5, w.Q[q:q + 1], ef=16, counters=True)), whole[q:q + 1], "query %d alone" % q)
    for size in (7, 56):
        parts = []
        for q0 in range(0, NQ, size):
            parts += _segments(H.Ohnsw.range_search(w.hg, 4.5, w.Q[q0:q0 + size], ef=16, counters=True))
        same(parts, whole, "calls of %d" % size)
    perm = np.random.default_rng(5).permutation(NQ)
    same(_segments(H.Ohnsw.range_search(w.hg, 4.5, w.Q[perm], ef=16, counters=True)), [whole[p] for p in perm], "permuted")
    # a page-locked query matrix, read in place
    Qp = H.host_empty((NQ, D))
    Qp[:] = w.Q
    same(_segments(H.Ohnsw.range_search(w.hg, 4.5, Qp, ef=16, counters=True)), whole, "page-locked")
    same(_segments(H.Ohnsw.brute_force_range(w.hg, 4.5, Qp)), _segments(H.Ohnsw.brute_force_range(w.hg, 4.5, w.Q)), "page-locked scan")


# ---- 3. row formats ------------------------------------------------------------------------------------------------------------

def _quantise(X):
    """option "sq8_rows": (B uint8 [n][d], lo, s), float32 operations, round to nearest even"""
    zero = np.float32(0)
    lo, hi = np.float32(X.min()) + zero, np.float32(X.max()) + zero
    s = np.float32(1) if hi == lo else np.float32(np.float32(hi - lo) / np.float32(255))
    return np.minimum(np.float32(255), np.maximum(zero, np.rint((X - lo) / s))).astype(np.uint8), lo, s


@pytest.mark.parametrize("rows", ["half_rows", "sq8_rows"])
def test_compact_rows_are_reranked_over_the_float32_rows(H, oracle, world, rows):
    w = world
    hg = H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, max_degree=8)
    hg.set_option(rows, 1)
    if rows == "half_rows":
        assert hg.info().row_format == ROWS_HALF
        walks = Walks(oracle, w.g, oracle.Space.l2(w.X.astype(np.float16).astype(np.float32), arith=oracle.TREE16), w.Q)
    else:
        assert hg.info().row_format == ROWS_SQ8
        B, lo, s = _quantise(w.X)
        walks = Walks(oracle, w.g, oracle.Space.l2(B.astype(np.float32), arith=oracle.TREE16), ((w.Q - lo) / s).astype(np.float32))
    want = restate(walks, w.full, 4.5, 16, 0, rerank=True)
    assert len(np.unique(want[1])) > 2, _hist(want[1])
    for refine in (0, 5):                          # the option does not shorten the list here
        hg.set_option("refine", refine)
        got = H.Ohnsw.range_search(hg, 4.5, w.Q, ef=16, counters=True)
        hg.set_option("refine", 0)
        _check(H, hg, w.Q, want, got, N, ctx="%s refine %d" % (rows, refine), minus_e=rows == "sq8_rows")
        # the returned distances are hnsw_distance_batch's for the returned ids
        lims, ids, dist = got[:3]
        for q in range(0, NQ, 9):
            if lims[q + 1] > lims[q]:
                seg = ids[lims[q]:lims[q + 1]]
                np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, w.Q[q:q + 1], seg[None, :])[0].view(np.uint32), dist[lims[q]:lims[q + 1]].view(np.uint32))
    # the exact form does not look at the row format
    _same_segments(H.Ohnsw.brute_force_range(hg, 4.5, w.Q), [w.full.prefix(q, 4.5) for q in range(NQ)], ctx=rows + " scan")
    hg.release()


def test_byte_rows_match_the_float32_rows(H):
    n, d = 2003, 128
    rng = np.random.default_rng(31)
    X = rng.integers(0, 219, size=(n, d)).astype(np.float32)
    Q = rng.integers(0, 219, size=(NQ, d)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    assert hg.info().row_format == ROWS_BYTES
    nearest = H.Ohnsw.brute_force_knn(hg, 200, Q)[1]
    stages = set()
    for radius in (float(np.median(nearest[:, 5])), float(np.median(nearest[:, 150]))):
        on = H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True)
        hg.set_option("byte_rows", 0)
        assert hg.info().row_format != ROWS_BYTES
        off = H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True)
        hg.set_option("byte_rows", 1)
        assert hg.info().row_format == ROWS_BYTES
        print("byte rows radius %g: stages %s, %d results" % (radius, _hist(on[5]), len(on[1])))
        assert len(on[1]) > 0
        stages |= set(on[5].tolist())
        for a, b in zip(on, off):
            np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert len(stages) > 2, stages
    hg.release()


# ---- 4. id_base 1, the inner product -------------------------------------------------------------------------------------------

def test_id_base_one(H, world):
    w = world
    up = [(nodes + 1, deg, np.where(nbr >= 0, nbr + 1, -1)) for nodes, deg, nbr in w.g.upper]
    hg = H.Hgraph(w.X, w.g.deg0, np.where(w.g.nbr0 >= 0, w.g.nbr0 + 1, -1), up, entry_point=w.g.entry_point + 1, id_base=1, max_degree=8)
    radius = float(np.quantile(w.full.table, 0.05))
    want = restate(w.walks, w.full, radius, 16, 1)
    assert len(np.unique(want[1])) > 1, _hist(want[1])
    got = H.Ba.range_search(hg, w.Q, 16, radius, counters=True)
    _check(H, hg, w.Q, want, got, N, sem=1, id_base=1, ctx="id_base 1 radius %g" % radius)
    _same_segments(H.Ohnsw.brute_force_range(hg, radius, w.Q), [w.full.prefix(q, radius) for q in range(NQ)], id_base=1, ctx="id_base 1 scan")
    hg.release()


def test_inner_product(H, oracle, world):
    w = world
    space = oracle.Space.ip(w.X, arith=oracle.TREE16)
    g = oracle.build_ohnsw(space, 8, 40, seed=1)
    hg = H.Hgraph(w.X, g.deg0, g.nbr0, g.upper, entry_point=g.entry_point, max_degree=8, metric=H.METRIC_IP)
    full = Full(oracle, space, w.Q, N)
    radius = float(np.quantile(full.table, 0.05))
    want = restate(Walks(oracle, g, space, w.Q), full, radius, 16, 0)
    assert len(np.unique(want[1])) > 1, _hist(want[1])
    got = H.Ohnsw.range_search(hg, radius, w.Q, ef=16, counters=True)
    _check(H, hg, w.Q, want, got, N, ctx="inner product radius %g" % radius)
    hg.release()


# ---- 5. the exact range scan, the smallest shapes that can break it ------------------------------------------------------------

SCAN_N, SCAN_NQ = 517, 9        # n: no multiple of 4 * UB for any NCH; nq: one full tile of 8 plus one (NCH 4: two tiles plus one)


def _scan_case(H, oracle, d, metric, seed):
    X, Q = _floats(SCAN_N, d, seed), _floats(SCAN_NQ, d, seed + 1)
    space = (oracle.Space.ip if metric else oracle.Space.l2)(X, arith=oracle.TREE16)
    return X, Q, H.Hgraph.flat(X, metric=metric), Full(oracle, space, Q, SCAN_N)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 200, 300, 600])       # NCH 1, 2, 4, 8 (the tile in LDS), 16
def test_exact_scan(H, oracle, d, metric):
    X, Q, hg, full = _scan_case(H, oracle, d, metric, 100 + d)
    below = -1.0 if metric == 0 else float(np.nextafter(full.dist.min(), np.float32(-np.inf)))
    boundary = float(full.dist[3, 40])                          # exactly one returned distance: the bound is inclusive
    radii = [below, float(np.quantile(full.table, 0.01)), float(np.quantile(full.table, 0.5)), INF, boundary]
    for slabs in (0, 1, 3, 1024):
        hg.set_option("scan_slabs", slabs)
        for radius in radii:
            want = [full.prefix(q, radius) for q in range(SCAN_NQ)]
            got = H.Ohnsw.brute_force_range(hg, radius, Q, counters=True)
            _same_segments(got, want, ctx="d %d metric %d slabs %d radius %g" % (d, metric, slabs, radius))
            assert (got[3] == SCAN_N).all() and (got[4] == 0).all() and (got[5] == EXACT).all()
            if radius == below:
                assert len(got[1]) == 0 and (got[0] == 0).all()
            if radius == INF:
                assert (np.diff(got[0]) == SCAN_N).all()
            if radius == boundary:
                assert got[0][4] - got[0][3] >= 41 and got[2][got[0][3] + 40] == np.float32(boundary)
    hg.release()


def test_equal_keys_come_out_in_id_order_across_slabs(H, oracle):
    d = 100
    X, Q = _floats(SCAN_N, d, 300), _floats(SCAN_NQ, d, 301)
    X[:64] = X[0]                                               # 64 equal keys per query
    hg = H.Hgraph.flat(X)
    full = Full(oracle, oracle.Space.l2(X, arith=oracle.TREE16), Q, SCAN_N)
    radius = float(np.quantile(full.table, 0.6))
    assert (full.table[:, 0] <= radius).any()
    for slabs in (0, 1, 3, 50, 1024):                           # 50: slabs of 11 rows, the run crosses five borders
        hg.set_option("scan_slabs", slabs)
        for r in (radius, INF):
            got = H.Ohnsw.brute_force_range(hg, r, Q)
            _same_segments(got, [full.prefix(q, r) for q in range(SCAN_NQ)], ctx="ties slabs %d radius %g" % (slabs, r))
        lims, ids, dist = got
        for q in range(SCAN_NQ):
            seg, sd = ids[lims[q]:lims[q + 1]], dist[lims[q]:lims[q + 1]]
            at = int(np.flatnonzero(seg == 0)[0])
            np.testing.assert_array_equal(seg[at:at + 64], np.arange(64))
            assert len(np.unique(sd[at:at + 64].view(np.uint32))) == 1
    hg.release()


def test_one_row_and_no_rows(H):
    Q = _floats(SCAN_NQ, 12, 400)
    one = H.Hgraph.flat(Q[4:5].copy())
    lims, ids, dist, nd, nh, stage = H.Ohnsw.brute_force_range(one, INF, Q, counters=True)
    np.testing.assert_array_equal(lims, np.arange(SCAN_NQ + 1))
    assert (ids == 0).all() and dist[4] == 0 and (nd == 1).all() and (stage == EXACT).all()
    lims, ids, dist = H.Ohnsw.brute_force_range(one, 0.0, Q)
    np.testing.assert_array_equal(np.diff(lims), np.arange(SCAN_NQ) == 4)
    assert ids.tolist() == [0] and dist.tolist() == [0.0]
    # the search through the one-node graph: W is never saturated beyond its single member
    got = H.Ohnsw.range_search(one, INF, Q, ef=1, counters=True)
    np.testing.assert_array_equal(got[0], np.arange(SCAN_NQ + 1))
    assert (got[5] == 1).all() and (got[1] == 0).all()          # W_1 is saturated, W_2 has one member of two
    one.release()
    none = H.Hgraph.flat(np.zeros((0, 12), np.float32))
    lims, ids, dist, nd, nh, stage = H.Ohnsw.brute_force_range(none, INF, Q, counters=True)
    assert (lims == 0).all() and len(lims) == SCAN_NQ + 1 and len(ids) == 0 and len(dist) == 0
    assert (nd == 0).all() and (nh == 0).all() and (stage == EXACT).all()
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.range_search(none, 1.0, Q, ef=16)                # the search needs a graph: HNSW_ERR_EMPTY_INDEX
    none.release()


def test_inserted_rows_are_found(H, oracle, world):
    w = world
    hg = H.Ohnsw.build_batch_bigarray(w.X[:500], 8, 40, seed=7)
    extra = w.Q[:20] + np.float32(0.001)                        # right beside the first twenty queries
    H.Ohnsw.insert_batch(hg, extra, 8, 40, seed=7)
    X = np.concatenate([w.X[:500], extra])
    full = Full(oracle, oracle.Space.l2(X, arith=oracle.TREE16), w.Q, 520)
    got = H.Ohnsw.brute_force_range(hg, 1.0, w.Q, counters=True)
    _same_segments(got, [full.prefix(q, 1.0) for q in range(NQ)], ctx="after insert")
    assert (got[3] == 520).all()
    for q in range(20):
        assert 500 + q in got[1][got[0][q]:got[0][q + 1]]
    lims, ids, _ = H.Ohnsw.range_search(hg, 1.0, w.Q, ef=16)
    for q in range(20):
        assert 500 + q in ids[lims[q]:lims[q + 1]]
    hg.release()


# ---- 6. errors and lifetime ----------------------------------------------------------------------------------------------------

def test_errors_leave_out_null(H, world):
    w = world
    L = H.load()

    def search(hg, radius=4.5, ef=16, sem=0, nq=NQ, qs=D, Q=w.Q):
        out = ctypes.c_void_p(1)
        p = H._RangeParams(radius, ef, sem)
        rc = L.hnsw_range_search_batch(hg.handle, Q.ctypes.data if Q is not None else None, nq, qs, ctypes.byref(p), ctypes.byref(out))
        assert rc == H.OK or out.value is None
        return rc, out

    def scan(hg, radius=4.5, nq=NQ, qs=D, Q=w.Q):
        out = ctypes.c_void_p(1)
        rc = L.hnsw_range_brute_force_batch(hg.handle, Q.ctypes.data if Q is not None else None, nq, qs, radius, ctypes.byref(out))
        assert rc == H.OK or out.value is None
        return rc, out

    assert search(w.hg, ef=0)[0] == H.ERR_BAD_ARG
    assert search(w.hg, ef=-3)[0] == H.ERR_BAD_ARG
    assert search(w.hg, ef=1025)[0] == H.ERR_UNSUPPORTED
    assert search(w.hg, sem=H.SEM_FUNCTOR_NEAREST_K)[0] == H.ERR_BAD_ARG
    assert search(w.hg, sem=7)[0] == H.ERR_BAD_ARG
    assert search(w.hg, radius=float("nan"))[0] == H.ERR_BAD_ARG
    assert scan(w.hg, radius=float("nan"))[0] == H.ERR_BAD_ARG
    assert search(w.hg, Q=None)[0] == H.ERR_BAD_ARG and scan(w.hg, Q=None)[0] == H.ERR_BAD_ARG
    assert search(w.hg, qs=D - 1)[0] == H.ERR_BAD_ARG and scan(w.hg, qs=D - 1)[0] == H.ERR_BAD_ARG
    assert search(w.hg, nq=-1)[0] == H.ERR_BAD_ARG and scan(w.hg, nq=-1)[0] == H.ERR_BAD_ARG
    p = H._RangeParams(4.5, 16, 0)
    assert L.hnsw_range_search_batch(w.hg.handle, w.Q.ctypes.data, NQ, D, None, ctypes.byref(ctypes.c_void_p())) == H.ERR_BAD_ARG
    assert L.hnsw_range_search_batch(w.hg.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(p), None) == H.ERR_BAD_ARG
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=0)
    with pytest.raises(H.Failure):
        H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=1025)
    # an empty graph: the search only
    empty = H.Hgraph(w.X[:3], [0, 0, 0], [[-1], [-1], [-1]], entry_point=None, max_degree=1)
    assert search(empty)[0] == H.ERR_EMPTY_INDEX
    rc, out = scan(empty, radius=INF)
    assert rc == H.OK
    r = H.RangeResult(out)
    assert r.size() == (NQ, 3 * NQ)
    r.release()
    empty.release()
    # nq == 0: a valid empty result
    for rc, out in (search(w.hg, nq=0, Q=None), scan(w.hg, nq=0, Q=None)):
        assert rc == H.OK and out.value
        r = H.RangeResult(out)
        assert r.size() == (0, 0)
        lims, ids, dist = r.fetch()
        assert lims.tolist() == [0] and len(ids) == 0 and len(dist) == 0
        r.release()
    # the handle still answers after all that
    assert len(H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=16)[1]) > 0


def test_two_results_alive_at_once(H, world):
    w = world
    L = H.load()
    before = w.hg.info().device_bytes
    a = H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=16, keep=True)
    b = H.Ohnsw.brute_force_range(w.hg, 3.5, w.Q[:10], keep=True)
    c = H.Ohnsw.range_search(w.hg, 6.0, w.Q, ef=16, keep=True)
    assert w.hg.info().device_bytes == before                   # neither results nor scratch are index tables
    assert L.hnsw_range_result_fetch(b.handle, None, None, None, None, None, None) == H.OK      # every pointer NULL
    assert b.size()[0] == 10 and a.size()[0] == NQ
    assert all(p != 0 for p in a.device_pointers()) and a.device_pointers() != c.device_pointers()
    got_c, got_b, got_a = c.fetch(True), b.fetch(True), a.fetch(True)           # fetched in the other order
    for r in (a, b, c):
        r.release()
    with pytest.raises(H.InvalidArgument):
        a.fetch()
    for got, want in ((got_a, H.Ohnsw.range_search(w.hg, 4.5, w.Q, ef=16, counters=True)),
                      (got_b, H.Ohnsw.brute_force_range(w.hg, 3.5, w.Q[:10], counters=True)),
                      (got_c, H.Ohnsw.range_search(w.hg, 6.0, w.Q, ef=16, counters=True))):
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    _same_segments(got_b, [w.full.prefix(q, 3.5) for q in range(10)], ctx="kept scan")


def test_cpp_front_end_range(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_range")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "range front-end ok" in out.stdout, out.stdout + out.stderr
