"""Range search under an allow-mask (ocaml-hnsw_amd/csrc/hnsw_range.hip): hnsw_range_search_batch_filtered and
hnsw_range_brute_force_batch_filtered against the definition the header gives -- the unfiltered call's segment with the nodes the
filter does not allow left out, the unfiltered call's stage and hops, its evaluations with n_allowed for n at the exact stage.

The unfiltered segments come from the oracle as in tests/test_gpu_range.py (the numpy helpers below are copied from there: W_e from
the oracle's walks, the ladder and the stage test restated, the exact stage from oracle.brute_force_knn); stage, hops and
evaluations are held against the unfiltered call on the same handle.  Every comparison is exact: ids equal, distances bit-equal."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_HALF, ROWS_SQ8 = 0, 2, 4, 5
EXACT = 0xFFFFFFFF
N, D, NQ = 2003, 20, 64
INF = float("inf")
SEVEN = (0, 31, 32, 1001, 1002, 1984, 2002)


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
        self.ids, self.dist = oracle.brute_force_knn(space, Q, n)
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
    """The header's definition of the UNFILTERED call -> (segments [(ids 0-based, distances)], stages).  rerank: the half / sq8 rule
    (all members of W re-ranked over the float32 rows: their order and distances from `full`)."""
    nq = len(walks.Q)
    r32 = np.float32(radius)
    segs, stage = [None] * nq, np.full(nq, EXACT, np.uint32)
    for q in range(nq):
        for j, e in enumerate(_ladder(ef)):
            W, Wd, _ = walks.get(sem, e)
            real = W[q] >= 0
            ids, d = W[q][real].astype(np.int64), Wd[q][real]
            if rerank:
                o = np.argsort(full.rank[q][ids], kind="stable")
                ids = ids[o]
                d = full.table[q][ids]
            if not (len(ids) == e and d[-1] <= r32):                    # not saturated: served here
                c = int((d <= r32).sum())
                assert (d[:c] <= r32).all()
                segs[q], stage[q] = (ids[:c], d[:c]), j
                break
        else:
            segs[q] = full.prefix(q, radius)
    return segs, stage


def _drop(segs, allow):
    """the segments with the disallowed nodes left out, the order kept"""
    return [(np.asarray(i)[allow[np.asarray(i, np.int64)]], np.asarray(d)[allow[np.asarray(i, np.int64)]]) for i, d in segs]


def _same_segments(got, want, id_base=0, ctx=""):
    lims, ids, dist = got[:3]
    assert lims[0] == 0 and lims[-1] == len(ids) == len(dist), ctx
    np.testing.assert_array_equal(np.diff(lims), [len(s[0]) for s in want], err_msg=ctx + " segment lengths")
    wi = np.concatenate([s[0] for s in want] + [np.zeros(0, np.int64)]).astype(np.int64) + id_base
    wd = np.concatenate([s[1] for s in want] + [np.zeros(0, np.float32)]).astype(np.float32)
    np.testing.assert_array_equal(ids, wi, err_msg=ctx + " ids")
    np.testing.assert_array_equal(dist.view(np.uint32), wd.view(np.uint32), err_msg=ctx + " distance bits")


def _segments_of(got):
    lims, ids, dist = got[:3]
    return [(ids[lims[q]:lims[q + 1]].astype(np.int64), dist[lims[q]:lims[q + 1]]) for q in range(len(lims) - 1)]


def _hist(stage):
    return dict(zip(*[a.tolist() for a in np.unique(stage, return_counts=True)]))


def _masks(n, seven):
    """the four masks of every case: half the nodes, every 20th node, seven nodes, no node"""
    half = np.random.default_rng(77).permutation(n) < n // 2
    every20 = np.arange(n) % 20 == 0
    few = np.zeros(n, bool)
    few[list(seven)] = True
    return {"half": half, "every 20th": every20, "seven": few, "none": np.zeros(n, bool)}


def _check_counters(got, base, n, n_allowed, ctx):
    """stage and hops are the unfiltered call's; evaluations too, with n_allowed for n at the exact stage; no node allowed: no walk"""
    if n_allowed == 0:
        assert (got[5] == EXACT).all() and (got[3] == 0).all() and (got[4] == 0).all(), ctx
        return
    np.testing.assert_array_equal(got[5], base[5], err_msg=ctx + " stage")
    np.testing.assert_array_equal(got[4], base[4], err_msg=ctx + " hops")
    exact = base[5] == EXACT
    want = base[3].astype(np.int64) - np.where(exact, n, 0) + np.where(exact, n_allowed, 0)
    np.testing.assert_array_equal(got[3].astype(np.int64), want, err_msg=ctx + " evaluations")


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """2003 Gaussian vectors of 20 dimensions, the oracle's graph (M 8, efC 40, seed 1), 64 queries; the four masks as filters"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.space = oracle.Space.l2(w.X, arith=oracle.TREE16)
    w.g = oracle.build_ohnsw(w.space, 8, 40, seed=1)
    w.hg = H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, id_base=0, max_degree=8)
    assert w.hg.info().row_format == ROWS_F32
    w.walks = Walks(oracle, w.g, w.space, w.Q)
    w.full = Full(oracle, w.space, w.Q, N)
    w.masks = _masks(N, SEVEN)
    w.filters = {name: w.hg.filter(m) for name, m in w.masks.items()}
    for name, m in w.masks.items():
        assert w.filters[name].count() == int(m.sum())
    yield w
    for f in w.filters.values():
        f.release()
    w.hg.release()


def _call(H, hg, Q, radius, sem, flt=None):
    return H._range_search(hg, Q, radius, 16, H.SEM_FUNCTOR if sem else H.SEM_OHNSW, True, filter=flt)


# ---- 1. the ladder -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("radius", [3.0, 4.5, 6.0])
def test_ladder(H, world, radius, sem):
    w = world
    segs, stage = restate(w.walks, w.full, radius, 16, sem)
    lens = np.array([len(s[0]) for s in segs])
    if radius == 3.0:                                   # the classes of tests/test_gpu_range.py's test_ladder: the same stage test
        assert (lens == 0).any() and (stage == 0).any()
    elif radius == 4.5:
        assert (stage == 0).any() and ((stage >= 1) & (stage <= 3)).any() and ((stage >= 4) & (stage != EXACT)).any(), _hist(stage)
    else:
        assert (stage == EXACT).any() and (stage != EXACT).any(), _hist(stage)
    base = _call(H, w.hg, w.Q, radius, sem)
    _same_segments(base, segs, ctx="unfiltered radius %g rule %d" % (radius, sem))
    np.testing.assert_array_equal(base[5], stage)
    for name, allow in w.masks.items():
        ctx = "radius %g rule %d mask %s" % (radius, sem, name)
        want = _drop(segs, allow)
        got = _call(H, w.hg, w.Q, radius, sem, w.filters[name])
        print("%s: stages %s, %d of %d results kept" % (ctx, _hist(got[5]), len(got[1]), int(lens.sum())))
        _same_segments(got, want, ctx=ctx)
        _check_counters(got, base, N, int(allow.sum()), ctx)
        if name == "half":
            # the mask takes a node out of a served segment and (where the class exists) out of an exact-stage segment
            cut = np.array([len(s[0]) for s in want]) < lens
            assert (cut & (stage != EXACT)).any(), ctx
            if radius == 6.0:
                assert (cut & (stage == EXACT)).any(), ctx
    # a mask made for this call (what Hgraph.filter takes) through the front end
    got = H.Ohnsw.range_search(w.hg, radius, w.Q, ef=16, filter=w.masks["every 20th"]) if sem == 0 else \
        H.Ba.range_search(w.hg, w.Q, 16, radius, filter=w.masks["every 20th"])
    _same_segments(got, _drop(segs, w.masks["every 20th"]), ctx="front end radius %g rule %d" % (radius, sem))


# ---- 2. the brute-force form on every lane grid --------------------------------------------------------------------------------

SCAN_N, SCAN_NQ = 517, 9        # n: no multiple of 4 * UB for any NCH; nq: one full tile of 8 plus one (NCH 4: two tiles plus one)
SCAN_SEVEN = (0, 31, 32, 255, 256, 480, 516)        # the seven nodes of the 517-node table: word borders, the first and the last node


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [20, 100, 200, 400, 600])      # NCH 1, 2, 4, 8 (the tile in LDS), 16
def test_exact_scan_under_a_mask(H, oracle, d, metric):
    X, Q = _floats(SCAN_N, d, 500 + d), _floats(SCAN_NQ, d, 501 + d)
    space = (oracle.Space.ip if metric else oracle.Space.l2)(X, arith=oracle.TREE16)
    full = Full(oracle, space, Q, SCAN_N)
    hg = H.Hgraph.flat(X, metric=metric)
    radius = float(np.median(full.table))               # neither empty nor full
    masks = _masks(SCAN_N, SCAN_SEVEN)
    filters = {name: hg.filter(m) for name, m in masks.items()}
    for slabs in (1, 3):
        hg.set_option("scan_slabs", slabs)
        for name, allow in masks.items():
            for r in ((radius, INF) if name == "half" else (radius,)):
                ctx = "d %d metric %d slabs %d mask %s radius %g" % (d, metric, slabs, name, r)
                want = _drop([full.prefix(q, r) for q in range(SCAN_NQ)], allow)
                got = H.Ohnsw.brute_force_range(hg, r, Q, counters=True, filter=filters[name])
                _same_segments(got, want, ctx=ctx)
                n_allowed = int(allow.sum())
                assert (got[3] == n_allowed).all() and (got[4] == 0).all() and (got[5] == EXACT).all(), ctx
                lens = np.diff(got[0])
                if name == "half" and r == radius:
                    assert (lens > 0).all() and (lens < n_allowed).all(), ctx
                if r == INF:
                    assert (lens == n_allowed).all(), ctx                  # the segment is the whole mask
                if name == "none":
                    assert len(got[1]) == 0 and (got[0] == 0).all(), ctx
    for f in filters.values():
        f.release()
    hg.release()


# ---- 3. the other row formats --------------------------------------------------------------------------------------------------

def _quantise(X):
    """option "sq8_rows": (B uint8 [n][d], lo, s), float32 operations, round to nearest even"""
    zero = np.float32(0)
    lo, hi = np.float32(X.min()) + zero, np.float32(X.max()) + zero
    s = np.float32(1) if hi == lo else np.float32(np.float32(hi - lo) / np.float32(255))
    return np.minimum(np.float32(255), np.maximum(zero, np.rint((X - lo) / s))).astype(np.uint8), lo, s


@pytest.mark.parametrize("rows", ["half_rows", "sq8_rows"])
def test_compact_rows_are_reranked_first_and_masked_after(H, oracle, world, rows):
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
    segs, stage = restate(walks, w.full, 4.5, 16, 0, rerank=True)
    assert len(np.unique(stage)) > 2, _hist(stage)
    base = _call(H, hg, w.Q, 4.5, 0)
    _same_segments(base, segs, ctx=rows + " unfiltered")
    for name, allow in w.masks.items():
        flt = hg.filter(allow)
        got = _call(H, hg, w.Q, 4.5, 0, flt)
        _same_segments(got, _drop(segs, allow), ctx="%s mask %s" % (rows, name))
        _check_counters(got, base, N, int(allow.sum()), "%s mask %s" % (rows, name))
        flt.release()
    hg.release()


def test_byte_rows(H, oracle):
    n, d = 2003, 128
    rng = np.random.default_rng(31)
    X = rng.integers(0, 219, size=(n, d)).astype(np.float32)
    Q = rng.integers(0, 219, size=(NQ, d)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    assert hg.info().row_format == ROWS_BYTES
    full = Full(oracle, oracle.Space.l2(X, arith=oracle.TREE16), Q, n)
    nearest = full.dist
    masks = _masks(n, SEVEN)
    stages = set()
    for radius in (float(np.median(nearest[:, 5])), float(np.median(nearest[:, 150]))):
        base = _call(H, hg, Q, radius, 0)
        stages |= set(base[5].tolist())
        for name, allow in masks.items():
            flt = hg.filter(allow)
            got = _call(H, hg, Q, radius, 0, flt)
            _same_segments(got, _drop(_segments_of(base), allow), ctx="byte rows radius %g mask %s" % (radius, name))
            _check_counters(got, base, n, int(allow.sum()), "byte rows radius %g mask %s" % (radius, name))
            got = H.Ohnsw.brute_force_range(hg, radius, Q, counters=True, filter=flt)
            _same_segments(got, _drop([full.prefix(q, radius) for q in range(NQ)], allow), ctx="byte rows scan radius %g mask %s" % (radius, name))
            flt.release()
    assert len(stages) > 2, stages
    hg.release()


# ---- 4. batch independence -----------------------------------------------------------------------------------------------------

def test_result_does_not_depend_on_the_batch(H, world):
    w = world
    flt = w.filters["half"]

    def rows(got):
        lims, ids, dist = got[:3]
        return [(ids[lims[q]:lims[q + 1]], dist[lims[q]:lims[q + 1]].view(np.uint32)) + tuple(c[q] for c in got[3:]) for q in range(len(lims) - 1)]

    def same(a, b, ctx):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v, err_msg=ctx)

    whole = rows(_call(H, w.hg, w.Q, 4.5, 0, flt))
    assert len({int(s[4]) for s in whole}) > 1
    same(rows(_call(H, w.hg, w.Q[:32], 4.5, 0, flt)) + rows(_call(H, w.hg, w.Q[32:], 4.5, 0, flt)), whole, "two halves")
    for q in range(NQ):
        same(rows(_call(H, w.hg, w.Q[q:q + 1], 4.5, 0, flt)), whole[q:q + 1], "query %d alone" % q)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------

def test_bad_filters_are_refused_with_out_null(H, world):
    w = world
    L = H.load()

    def search(hg, f, Q=w.Q):
        out = ctypes.c_void_p(1)
        p = H._RangeParams(4.5, 16, 0)
        rc = L.hnsw_range_search_batch_filtered(hg.handle, f, Q.ctypes.data, len(Q), Q.shape[1], ctypes.byref(p), ctypes.byref(out))
        assert rc == H.OK or out.value is None
        if rc == H.OK:
            H.RangeResult(out).release()
        return rc

    def scan(hg, f, Q=w.Q):
        out = ctypes.c_void_p(1)
        rc = L.hnsw_range_brute_force_batch_filtered(hg.handle, f, Q.ctypes.data, len(Q), Q.shape[1], 4.5, ctypes.byref(out))
        assert rc == H.OK or out.value is None
        if rc == H.OK:
            H.RangeResult(out).release()
        return rc

    good = w.filters["half"]
    assert search(w.hg, good.handle) == H.OK and scan(w.hg, good.handle) == H.OK
    assert search(w.hg, None) == H.ERR_BAD_ARG and scan(w.hg, None) == H.ERR_BAD_ARG                 # a null filter
    other = H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, max_degree=8)
    assert search(other, good.handle) == H.ERR_BAD_ARG and "another index" in L.hnsw_last_error().decode()  # a foreign filter
    assert scan(other, good.handle) == H.ERR_BAD_ARG
    other.release()
    small = H.Ohnsw.build_batch_bigarray(w.X[:500], 8, 40, seed=7)
    f = small.filter(np.arange(500) % 2 == 0)
    assert search(small, f.handle) == H.OK
    H.Ohnsw.insert_batch(small, w.X[500:520], 8, 40, seed=7)
    assert search(small, f.handle) == H.ERR_BAD_ARG and scan(small, f.handle) == H.ERR_BAD_ARG        # outgrown by an insert
    f.release()
    small.release()
    # the unfiltered calls' own errors come first and are unchanged
    out = ctypes.c_void_p(1)
    p = H._RangeParams(float("nan"), 16, 0)
    assert L.hnsw_range_search_batch_filtered(w.hg.handle, good.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(p), ctypes.byref(out)) == H.ERR_BAD_ARG
    assert out.value is None
    assert L.hnsw_range_search_batch_filtered(w.hg.handle, good.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(H._RangeParams(4.5, 16, 0)), None) == H.ERR_BAD_ARG
    # nq == 0: a valid empty result
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_brute_force_batch_filtered(w.hg.handle, good.handle, None, 0, 0, 4.5, ctypes.byref(out)) == H.OK and out.value
    r = H.RangeResult(out)
    assert r.size() == (0, 0)
    r.release()
