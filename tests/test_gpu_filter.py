"""Filtered search (ocaml-hnsw_amd/csrc/hnsw_filter.hip): hnsw_filter_* and hnsw_search_batch_filtered against the definition
the header gives, restated in numpy below over the oracle's walks.

W_e(q) comes from the oracle (float32 space, TREE16 summation, canonical ties, k := e) as the parity tests obtain it; the ladder
e = ef, 2 ef, ... 1024, the stage test (k allowed members of W_e), the first-k / re-rank rule and the exact stage are `restate`.
Every query is compared, ids equal and distances bit-equal.  The oracle reports no evaluation counts of the kernel (its visited
cache re-evaluates forgotten nodes) and the functor search no hops: out_ndist is held against the plain searches of the same
handle (the same walks), out_nhops against the oracle's hops under the Ohnsw rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8 = 0, 2, 3, 4, 5
EXACT = 0xFFFFFFFF
N, D, NQ = 2003, 20, 64           # n is no multiple of 32: the mask's last word is partial

# The uniform 10 % mask of test_ladder_is_exercised: np.random.default_rng(seed).random(N) < 0.1.  The seed is the first (from 0
# on) for which the restatement serves some query at stage 0 or 1 -- ten allowed nodes among the 32 of W_32: rare under such a
# mask -- found with _first_mask_seed below on the index of the `world` fixture, and fixed.
LADDER_MASK_SEED = 20


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).normal(size=(n, d))).astype(np.float32)


def _graph(oracle, hg):
    hg.export()
    return oracle.Graph(hg.n, hg.entry_point, hg.deg0, hg.nbr0, hg.upper)


def _fill_value(fill):
    return np.float32(np.nan) if fill == 0 else np.float32(np.inf)


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


def _stages(walks, mask, ef, k, sem):
    """per query the ladder stage that serves it (EXACT: none does), and the e of the walks it takes"""
    nq = len(walks.Q)
    stage = np.full(nq, EXACT, np.uint32)
    taken = [[] for _ in range(nq)]
    if mask.sum() < k:
        return stage, taken
    pending = list(range(nq))
    for j, e in enumerate(_ladder(ef)):
        W = walks.get(sem, e)[0]
        allowed = (W >= 0) & mask[np.maximum(W, 0)]
        still = []
        for q in pending:
            taken[q].append(e)
            if allowed[q].sum() >= k:
                stage[q] = j
            else:
                still.append(q)
        pending = still
        if not pending:
            break
    return stage, taken


def restate(walks, mask, ef, k, sem, fill, key=None, exact=None):
    """The header's definition.  key(q, v) -> (order key, distance) of the pair over the float32 rows: the half / sq8 rule (all
    allowed members of W re-ranked); None: the first k allowed members with the walk's distances.  exact(q) -> (ids, distances) of
    ALL allowed nodes in the exact scan's order.  -> ids (0-based), distances, stages, hops summed (None under the functor rule),
    candidates re-ranked, walks taken"""
    nq = len(walks.Q)
    ids = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), _fill_value(fill), np.float32)
    stage, taken = _stages(walks, mask, ef, k, sem)
    hops = np.zeros(nq, np.uint32) if sem == 0 else None
    reranked = np.zeros(nq, np.uint32)
    ladder = _ladder(ef)
    for q in range(nq):
        if hops is not None:
            hops[q] = sum(int(walks.get(sem, e)[2][q]) for e in taken[q])
        if stage[q] == EXACT:
            ei, ed = exact(q)
            ids[q, :min(k, len(ei))] = ei[:k]
            dist[q, :min(k, len(ei))] = ed[:k]
            continue
        W, Wd, _ = walks.get(sem, ladder[stage[q]])
        ok = (W[q] >= 0) & mask[np.maximum(W[q], 0)]
        A, Ad = W[q][ok].astype(np.int64), Wd[q][ok]
        if key is None:
            ids[q], dist[q] = A[:k], Ad[:k]
        else:
            kd = [key(q, int(v)) for v in A]
            order = np.lexsort((A, np.array([a for a, _ in kd], np.float32)))[:k]
            ids[q], dist[q] = A[order], np.array([b for _, b in kd], np.float32)[order]
            reranked[q] = len(A)
    return ids, dist, stage, hops, reranked, taken


def _exact_from_distance_batch(H, hg, Q, mask):
    """numpy's masked exact order over hnsw_distance_batch's distances: q -> (allowed ids 0-based, distances), by (distance, id)"""
    allowed = np.flatnonzero(mask).astype(np.int32)
    if len(allowed) == 0:
        return lambda q: (allowed, np.zeros(0, np.float32))
    Dm = H.Ohnsw.distance_l2(hg, Q, np.tile(allowed + hg.id_base, (len(Q), 1)))

    def exact(q):
        o = np.lexsort((allowed, Dm[q]))
        return allowed[o], Dm[q][o]
    return exact


def _same(got, want, id_base=0, ctx=""):
    wi = np.where(want[0] >= 0, want[0] + id_base, -1)
    np.testing.assert_array_equal(got[0], wi, err_msg=ctx)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=ctx)


def _tree16_key(oracle, X, Q):
    cache = {}

    def key(q, v):
        if (q, v) not in cache:
            sq = np.float32(oracle.l2sq_tree16(X[v], Q[q]))
            cache[(q, v)] = (sq, np.float32(np.sqrt(np.float64(sq))))
        return cache[(q, v)]
    return key


def _uniform_mask(seed, p, n=N):
    return np.random.default_rng(seed).random(n) < p


def _first_mask_seed(walks, ef=16, k=10, p=0.1, limit=100000):
    """how LADDER_MASK_SEED was chosen (the walks do not depend on the mask: one seed costs two array look-ups)"""
    W16, W32 = walks.get(0, ef)[0], walks.get(0, 2 * ef)[0]
    for seed in range(limit):
        m = _uniform_mask(seed, p)
        if ((m[W16].sum(1) >= k) | (m[W32].sum(1) >= k)).any():
            return seed
    return None


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """the index of the issue: 2003 Gaussian vectors of 20 dimensions, hnsw_build with M 8, efC 40, 64 queries"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.hg = H.Ohnsw.build_batch_bigarray(w.X, 8, 40, seed=7)
    assert w.hg.info().row_format == ROWS_F32
    w.g = _graph(oracle, w.hg)
    w.walks = Walks(oracle, w.g, oracle.Space.l2(w.X, arith=oracle.TREE16), w.Q)
    yield w
    w.hg.release()


def _plain_counts(H, hg, Q, taken, sem=0):
    """evaluations of the walks each query took, from the plain searches of the same handle with (ef = e, k = e)"""
    cache, out = {}, np.zeros(len(Q), np.uint32)
    for q, es in enumerate(taken):
        for e in es:
            if e not in cache:
                cache[e] = H._search(hg, Q, e, e, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=sem)[2]
            out[q] += cache[e][q]
    return out


def _check(H, w, mask, ef, k, sem=0, ctx=""):
    fill = H.FILL_BA if sem else H.FILL_OHNSW
    want = restate(w.walks, mask, ef, k, sem, fill, exact=_exact_from_distance_batch(H, w.hg, w.Q, mask))
    got = H._search_filtered(w.hg, mask, w.Q, ef, k, fill, True, sem=sem)
    print("%s: stages %s" % (ctx, dict(zip(*np.unique(want[2], return_counts=True)))))
    _same(got[:2], want[:2], ctx=ctx)
    np.testing.assert_array_equal(got[4], want[2], err_msg=ctx)
    if want[3] is not None:
        np.testing.assert_array_equal(got[3], want[3], err_msg=ctx)
    nd = _plain_counts(H, w.hg, w.Q, want[5], sem) + np.where(want[2] == EXACT, np.uint32(mask.sum()), np.uint32(0))
    np.testing.assert_array_equal(got[2], nd, err_msg=ctx)
    return want, got


# ---- 1. identity mask ----------------------------------------------------------------------------------------------------------

def test_identity_mask_is_the_plain_search(H, world):
    w = world
    flt = w.hg.filter(np.ones(N, bool))
    assert flt.count() == N
    for ef, k in ((64, 10), (16, 10), (16, 16), (200, 1)):
        plain = H.Ohnsw.knn_batch_bigarray(w.hg, k, w.Q, ef=ef, counters=True)
        got = H.Ohnsw.knn_batch_filtered(w.hg, k, w.Q, flt, ef=ef, counters=True)
        for a, b in zip(got[:4], plain):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="ef %d k %d" % (ef, k))
        assert (got[4] == 0).all()
    flt.release()


# ---- 2. half the nodes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [0, 1])
def test_selectivity_half(H, world, sem):
    want, _ = _check(H, world, _uniform_mask(11, 0.5), 64, 10, sem, "selectivity 0.5 rule %d" % sem)
    assert (want[2] == 0).mean() > 0.5


# ---- 3. a tenth of the nodes: the ladder ---------------------------------------------------------------------------------------

def test_ladder_is_exercised(H, world):
    mask = _uniform_mask(LADDER_MASK_SEED, 0.1)
    want, got = _check(H, world, mask, 16, 10, 0, "selectivity 0.1")
    assert ((want[2] >= 1) & (want[2] != EXACT)).any() and (want[2] <= 1).any(), np.unique(want[2], return_counts=True)
    np.testing.assert_array_equal(got[3], want[3])               # out_nhops: the oracle's hops summed over the stages taken
    assert (got[3] > world.walks.get(0, 16)[2]).any()


# ---- 4. twenty allowed nodes: some queries reach the exact stage ---------------------------------------------------------------

def test_twenty_allowed_nodes(H, world):
    w = world
    mask = np.zeros(N, bool)
    mask[np.random.default_rng(21).choice(N, 20, replace=False)] = True
    want, got = _check(H, w, mask, 16, 10, 0, "twenty allowed")
    assert (want[2] == EXACT).any() and (want[2] != EXACT).any(), np.unique(want[2], return_counts=True)
    exact = _exact_from_distance_batch(H, w.hg, w.Q, mask)
    for q in np.flatnonzero(want[2] == EXACT):
        ei, ed = exact(q)
        np.testing.assert_array_equal(got[0][q], ei[:10])
        np.testing.assert_array_equal(got[1][q].view(np.uint32), ed[:10].view(np.uint32))


# ---- 5. fewer allowed nodes than k ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("id_base", [0, 1])
def test_three_allowed_then_none(H, world, id_base):
    w = world
    if id_base == 0:
        hg = w.hg
    else:       # the same graph as a 1-based index: the Hnsw.Ba-style front, functor rule, +inf fill
        up = [(nodes + 1, deg, np.where(nbr >= 0, nbr + 1, -1)) for nodes, deg, nbr in w.hg.upper]
        hg = H.Hgraph(w.X, w.hg.deg0, np.where(w.hg.nbr0 >= 0, w.hg.nbr0 + 1, -1), up, entry_point=w.hg.entry_point + 1, id_base=1,
                      max_degree=w.hg.max_degree)
    for allowed in ([5, 700, 2002], []):
        mask = np.zeros(N, bool)
        mask[allowed] = True
        exact = _exact_from_distance_batch(H, hg, w.Q, mask)
        for fill in ((H.FILL_OHNSW, H.FILL_BA) if id_base == 0 else (H.FILL_BA,)):
            if id_base == 0:
                got = H._search_filtered(hg, mask, w.Q, 16, 10, fill, True)
            else:
                got = H.Ba.knn_batch_filtered(hg, w.Q, 16, 10, np.array(allowed, np.int64) + 1, counters=True)
            assert (got[4] == EXACT).all()
            assert (got[2] == len(allowed)).all() and (got[3] == 0).all()       # no walk: n_allowed evaluations, no hops
            for q in range(NQ):
                ei, ed = exact(q)
                np.testing.assert_array_equal(got[0][q, :len(allowed)], ei + id_base)
                np.testing.assert_array_equal(got[1][q, :len(allowed)].view(np.uint32), ed.view(np.uint32))
            assert (got[0][:, len(allowed):] == -1).all()
            gap = got[1][:, len(allowed):]
            assert np.isnan(gap).all() if fill == H.FILL_OHNSW else (np.isinf(gap) & (gap > 0)).all()
    if id_base:
        hg.release()


# ---- 6. word edges -------------------------------------------------------------------------------------------------------------

def _raw_filter(H, hg, words, n_bits):
    f = ctypes.c_void_p()
    rc = H.load().hnsw_filter_create(hg.handle, words.ctypes.data, n_bits, ctypes.byref(f))
    if rc != H.OK:
        return rc, None
    flt = H.Filter.__new__(H.Filter)
    flt._f, flt._hg, flt.n = f, hg, n_bits
    return rc, flt


def test_word_edges(H, world):
    w = world
    mask = np.zeros(N, bool)
    mask[[31, 32, 63, 64, 2002]] = True
    for ef, k in ((16, 10), (16, 3)):             # fewer than k allowed: the masked scan alone; k = 3: the ladder first
        want, got = _check(H, w, mask, ef, k, 0, "word edges k %d" % k)
        assert set(got[0][got[0] >= 0]) <= {31, 32, 63, 64, 2002}
        # garbage past n in the last word (bits 19 .. 31 of word 62) changes nothing
        words = H.pack_allow(mask, N)
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(N % 32)
        rc, dirty = _raw_filter(H, w.hg, words, N)
        assert rc == H.OK and dirty.count() == 5
        again = H._search_filtered(w.hg, dirty, w.Q, ef, k, H.FILL_OHNSW, True)
        for a, b in zip(again, got):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        dirty.release()


# ---- 7. row formats ------------------------------------------------------------------------------------------------------------

def _format_pair(H, hg, Q, option, mask, cases):
    """the filtered answers with `option` on and off are the same bits"""
    flt = hg.filter(mask)
    for ef, k in cases:
        hg.set_option(option, 1)
        on = H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef, counters=True)
        hg.set_option(option, 0)
        assert hg.info().row_format == ROWS_F32
        off = H.Ohnsw.knn_batch_filtered(hg, k, Q, flt, ef=ef, counters=True)
        hg.set_option(option, 1)
        for a, b in zip(on, off):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="%s ef %d k %d" % (option, ef, k))
        np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, Q, np.maximum(on[0], 0)).view(np.uint32)[on[0] >= 0], on[1].view(np.uint32)[on[0] >= 0])
        assert len(np.unique(on[4])) > 1 or ef == 64
    flt.release()


def test_byte_rows_match_the_float32_rows(H, world):
    Xb = np.clip(np.rint(world.X * 40 + 128), 0, 255).astype(np.float32)
    Qb = np.clip(np.rint(world.Q * 40 + 128), 0, 255).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(Xb, 8, 40, seed=7)
    assert hg.info().row_format == ROWS_BYTES
    _format_pair(H, hg, Qb, "byte_rows", _uniform_mask(31, 0.5), ((64, 10),))
    _format_pair(H, hg, Qb, "byte_rows", _uniform_mask(32, 0.1), ((16, 10),))
    hg.release()


def test_split_rows_match_the_float32_rows(H):
    n, d = 600, 100                                # 400-byte rows: three 128-byte lines and a 16-byte tail
    X, Q = _floats(n, d, 41), _floats(NQ, d, 42)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    assert hg.info().row_format == ROWS_SPLIT
    _format_pair(H, hg, Q, "split_rows", _uniform_mask(43, 0.5, n), ((64, 10),))
    _format_pair(H, hg, Q, "split_rows", _uniform_mask(44, 0.03, n), ((16, 10),))      # 1024 > n: W holds every reachable node
    hg.release()


def _quantise(X):
    """option "sq8_rows": (B uint8 [n][d], lo, s), float32 operations, round to nearest even"""
    zero = np.float32(0)
    lo, hi = np.float32(X.min()) + zero, np.float32(X.max()) + zero
    s = np.float32(1) if hi == lo else np.float32(np.float32(hi - lo) / np.float32(255))
    return np.minimum(np.float32(255), np.maximum(zero, np.rint((X - lo) / s))).astype(np.uint8), lo, s


@pytest.mark.parametrize("rows", ["half_rows", "sq8_rows"])
def test_compact_rows_are_reranked_over_the_float32_rows(H, oracle, world, rows):
    w = world
    hg = H.Hgraph(w.X, w.hg.deg0, w.hg.nbr0, w.hg.upper, entry_point=w.hg.entry_point, max_degree=w.hg.max_degree)
    hg.set_option(rows, 1)
    if rows == "half_rows":
        assert hg.info().row_format == ROWS_HALF
        walks = Walks(oracle, w.g, oracle.Space.l2(w.X.astype(np.float16).astype(np.float32), arith=oracle.TREE16), w.Q)
    else:
        assert hg.info().row_format == ROWS_SQ8
        B, lo, s = _quantise(w.X)
        walks = Walks(oracle, w.g, oracle.Space.l2(B.astype(np.float32), arith=oracle.TREE16), ((w.Q - lo) / s).astype(np.float32))
    key = _tree16_key(oracle, w.X, w.Q)
    for refine in (0, 5):                          # the option does not shorten the list here
        hg.set_option("refine", refine)
        for mask, ef, k in ((_uniform_mask(51, 0.5), 64, 10), (_uniform_mask(52, 0.1), 16, 10), (_uniform_mask(53, 0.004), 16, 4)):
            ctx = "%s refine %d ef %d k %d" % (rows, refine, ef, k)
            want = restate(walks, mask, ef, k, 0, H.FILL_OHNSW, key=key, exact=_exact_from_distance_batch(H, hg, w.Q, mask))
            got = H.Ohnsw.knn_batch_filtered(hg, k, w.Q, mask, ef=ef, counters=True)
            print("%s: stages %s" % (ctx, dict(zip(*np.unique(want[2], return_counts=True)))))
            _same(got[:2], want[:2], ctx=ctx)
            np.testing.assert_array_equal(got[4], want[2], err_msg=ctx)
            np.testing.assert_array_equal(got[3], want[3], err_msg=ctx)
            # the returned distances are hnsw_distance_batch's for the returned ids
            real = got[0] >= 0
            np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, w.Q, np.maximum(got[0], 0)).view(np.uint32)[real], got[1].view(np.uint32)[real])
            # evaluations: the walks taken (the plain search of (e, e) over the same rows; sq8: minus the e it re-ranks itself),
            # plus the candidates re-ranked, plus n_allowed at the exact stage
            hg.set_option("refine", 0)
            cache, nd = {}, np.zeros(NQ, np.uint32)
            for q, es in enumerate(want[5]):
                for e in es:
                    if e not in cache:
                        cache[e] = H.Ohnsw.knn_batch_bigarray(hg, e, w.Q, ef=e, counters=True)[2] - np.uint32(e if rows == "sq8_rows" else 0)
                    nd[q] += cache[e][q]
            hg.set_option("refine", refine)
            nd += want[4] + np.where(want[2] == EXACT, np.uint32(mask.sum()), np.uint32(0))
            np.testing.assert_array_equal(got[2], nd, err_msg=ctx)
    hg.release()


# ---- 8. batch independence -----------------------------------------------------------------------------------------------------

def test_result_does_not_depend_on_the_batch(H, world):
    w = world
    flt = w.hg.filter(_uniform_mask(LADDER_MASK_SEED, 0.1))
    whole = H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, flt, ef=16, counters=True)
    assert len(np.unique(whole[4])) > 1
    for q in range(NQ):
        one = H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q[q:q + 1], flt, ef=16, counters=True)
        for a, b in zip(one, whole):
            np.testing.assert_array_equal(a[0].view(np.uint32), b[q].view(np.uint32), err_msg="query %d" % q)
    # page-locked matrices, read and written in place
    Qp = H.host_empty((NQ, D))
    Qp[:] = w.Q
    out = (H.host_empty((NQ, 10), np.int32), H.host_empty((NQ, 10), np.float32))
    pinned = H.Ohnsw.knn_batch_filtered(w.hg, 10, Qp, flt, ef=16, out=out)
    assert pinned[0] is out[0]
    _same(pinned, whole[:2])
    flt.release()


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(H, world):
    w = world
    L = H.load()
    flt = w.hg.filter(_uniform_mask(61, 0.5))
    ids = np.full((NQ, 10), 77, np.int32)
    dist = np.full((NQ, 10), 7.5, np.float32)
    cnt = [np.full(NQ, 9, np.uint32) for _ in range(3)]

    def call(hg, f, ef=16, k=10, sem=0):
        p = H._SearchParams(ef, k, H.FILL_OHNSW, sem)
        rc = L.hnsw_search_batch_filtered(hg.handle, f.handle if f is not None else None, w.Q.ctypes.data, NQ, D, ctypes.byref(p),
                                          ids.ctypes.data, dist.ctypes.data, cnt[0].ctypes.data, cnt[1].ctypes.data, cnt[2].ctypes.data)
        assert (ids == 77).all() and (dist == 7.5).all() and all((c == 9).all() for c in cnt)
        return rc

    # a filter from another handle
    other = H.Hgraph.flat(w.X)
    foreign = other.filter(np.ones(N, bool))
    assert call(w.hg, foreign) == H.ERR_BAD_ARG
    assert call(w.hg, None) == H.ERR_BAD_ARG
    # n_bits != n
    words = H.pack_allow(np.ones(N, bool), N)
    for n_bits in (N - 1, N + 1, 0):
        assert _raw_filter(H, w.hg, words, n_bits)[0] == H.ERR_BAD_ARG
    # the parameters
    assert call(w.hg, flt, ef=8, k=10) == H.ERR_BAD_ARG
    assert call(w.hg, flt, ef=1025, k=10) == H.ERR_UNSUPPORTED
    assert call(w.hg, flt, ef=16, k=10, sem=H.SEM_FUNCTOR_NEAREST_K) == H.ERR_BAD_ARG
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, flt, ef=8)
    with pytest.raises(H.Failure):
        H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, flt, ef=1025)
    # an empty index
    empty = H.Hgraph(w.X[:3], [0, 0, 0], [[-1], [-1], [-1]], entry_point=None, max_degree=1)
    ef_ = empty.filter(np.ones(3, bool))
    assert call(empty, ef_) == H.ERR_EMPTY_INDEX
    # a filter made before insert_batch grew the index
    grown = H.Ohnsw.build_batch_bigarray(w.X[:500], 8, 40, seed=7)
    old = grown.filter(np.ones(500, bool))
    assert (H.Ohnsw.knn_batch_filtered(grown, 10, w.Q, old, ef=16)[0] >= 0).all()      # valid until the index grows
    H.Ohnsw.insert_batch(grown, w.X[500:520], 8, 40, seed=7)
    assert call(grown, old) == H.ERR_BAD_ARG
    new = grown.filter(np.ones(520, bool))
    assert (H.Ohnsw.knn_batch_filtered(grown, 10, w.Q, new, ef=16)[0] >= 0).all()
    # the filter of the index itself still works after all that
    assert (H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, flt, ef=16)[0] >= 0).all()
    for f in (flt, foreign, ef_, old, new):
        f.release()
    for h in (other, empty, grown):
        h.release()


# ---- 10. the count -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.001, 0.1, 0.5, 1.0])
def test_filter_count(H, world, p):
    mask = _uniform_mask(70, p) if p < 1 else np.ones(N, bool)
    flt = world.hg.filter(mask)
    assert flt.count() == int(mask.sum())
    by_ids = world.hg.filter(np.flatnonzero(mask))
    assert by_ids.count() == int(mask.sum())
    before = world.hg.info().device_bytes
    more = [world.hg.filter(mask) for _ in range(3)]
    assert world.hg.info().device_bytes == before              # the masks are not index tables
    for f in more + [flt, by_ids]:
        f.release()


def test_cpp_front_end_filter(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_filter")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "filter front-end ok" in out.stdout, out.stdout + out.stderr


if __name__ == "__main__":      # python tests/test_gpu_filter.py: prints the value LADDER_MASK_SEED was fixed to (needs the device)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    import ocaml_hnsw_amd as H_
    from oracle import oracle as o_
    o_.build()
    o_.lib()
    X_, Q_ = _floats(N, D, 1), _floats(NQ, D, 2)
    hg_ = H_.Ohnsw.build_batch_bigarray(X_, 8, 40, seed=7)
    walks_ = Walks(o_, _graph(o_, hg_), o_.Space.l2(X_, arith=o_.TREE16), Q_)
    seed_ = _first_mask_seed(walks_)
    print("LADDER_MASK_SEED", seed_)
    if seed_ is not None:
        print("stages", dict(zip(*np.unique(_stages(walks_, _uniform_mask(seed_, 0.1), 16, 10, 0)[0], return_counts=True))))
