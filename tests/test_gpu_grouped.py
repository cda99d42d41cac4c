"""Grouped search (ocaml-hnsw_amd/csrc/hnsw_group.hip): hnsw_labels_*, hnsw_search_batch_grouped and hnsw_brute_force_batch_grouped
against the definition the header gives, restated in numpy below.

W_e(q) comes from the oracle, as in tests/test_gpu_filter.py (its Walks); the ladder, the stage test |G(W_e)| >= k, the first
eligible member of each label, the re-rank rule of the inexact rows and the exact stage are `restate`.  The exact stage's expected
rows are numpy's grouping of hnsw_distance_batch's distances ordered by (distance, id).  Ids and labels compare equal, distances
bit-equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_gpu_filter import EXACT, Walks, _fill_value, _floats, _graph, _ladder, _plain_counts, _quantise, _same, _tree16_key, _uniform_mask

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_HALF, ROWS_SQ8, ROWS_SQ8_DIM = 0, 4, 5, 6
N, D, NQ = 2003, 20, 64           # n is no multiple of 32
CLUSTERS, PER = 40, 100           # the clustered world: n = 4000

# The clustered world of test_all_classes_of_stage: centres = CLUSTER_SPREAD * normal(40, 20), points = centre + normal, seed
# CLUSTER_SEED.  The seed is the first (from 0 on) for which the restatement alone, over the oracle's walks of the exported graph,
# serves at least 5 queries in each class -- stage 0, a later stage, the exact stage -- found with _first_cluster_seed below
# (python tests/test_gpu_grouped.py), and fixed.
CLUSTER_SEED = 0
CLUSTER_SPREAD = 3.0


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


# ---- the header's definition ---------------------------------------------------------------------------------------------------

def _eligible(lab, mask):
    return (lab >= 0) if mask is None else ((lab >= 0) & mask)


def _G(ids, lab):
    """positions of the first member of each label in the list of (eligible) node ids"""
    _, first = np.unique(lab[ids], return_index=True)
    return np.sort(first)


def _walked(lab, mask, k):
    return len(np.unique(lab[lab >= 0])) >= k and (mask is None or mask.sum() >= k)


def restate(walks, lab, mask, ef, k, sem, fill, exact, key=None):
    """-> ids (0-based), distances, labels, stages, hops summed (None under the functor rule), members re-ranked, walks taken"""
    nq = len(walks.Q)
    elig = _eligible(lab, mask)
    ids = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), _fill_value(fill), np.float32)
    labs = np.full((nq, k), -1, np.int32)
    stage = np.full(nq, EXACT, np.uint32)
    hops = np.zeros(nq, np.uint32) if sem == 0 else None
    reranked = np.zeros(nq, np.uint32)
    taken = [[] for _ in range(nq)]
    walked = _walked(lab, mask, k)
    for q in range(nq):
        for j, e in enumerate(_ladder(ef) if walked else ()):
            W, Wd, wh = walks.get(sem, e)
            taken[q].append(e)
            if hops is not None:
                hops[q] += int(wh[q])
            ok = (W[q] >= 0) & elig[np.maximum(W[q], 0)]
            A, Ad = W[q][ok].astype(np.int64), Wd[q][ok]
            if key is not None:          # ALL eligible members over the float32 rows, then G over that list
                kd = [key(q, int(v)) for v in A]
                order = np.lexsort((A, np.array([a for a, _ in kd], np.float32)))
                A, Ad = A[order], np.array([b for _, b in kd], np.float32)[order]
            reranked[q] += len(A)        # (what the inexact rows re-rank at this stage)
            g = _G(A, lab)
            if len(g) >= k:
                stage[q] = j
                ids[q], dist[q], labs[q] = A[g[:k]], Ad[g[:k]], lab[A[g[:k]]]
                break
        if stage[q] == EXACT:
            ei, ed = exact(q)
            m = min(k, len(ei))
            ids[q, :m], dist[q, :m], labs[q, :m] = ei[:m], ed[:m], lab[ei[:m]]
    return ids, dist, labs, stage, hops, reranked, taken


def _exact_grouped(H, hg, Q, lab, mask=None):
    """numpy's grouping of hnsw_distance_batch's distances: q -> (one node per label 0-based, distances), by (distance, id)"""
    nodes = np.flatnonzero(_eligible(lab, mask)).astype(np.int32)
    if len(nodes) == 0:
        return lambda q: (nodes, np.zeros(0, np.float32))
    Dm = H.Ohnsw.distance_l2(hg, Q, np.tile(nodes + hg.id_base, (len(Q), 1)))

    def exact(q):
        o = np.lexsort((nodes, Dm[q]))
        g = _G(nodes[o], lab)
        return nodes[o][g], Dm[q][o][g]
    return exact


def _same3(got, want, id_base=0, ctx=""):
    _same(got[:2], want[:2], id_base, ctx)
    np.testing.assert_array_equal(got[2], want[2], err_msg=ctx)


def _check(H, w, L, lab, ef, k, sem=0, mask=None, flt=None, ctx=""):
    """the grouped call against the restatement: rows, stages, hops, evaluations"""
    fill = H.FILL_BA if sem else H.FILL_OHNSW
    want = restate(w.walks, lab, mask, ef, k, sem, fill, _exact_grouped(H, w.hg, w.Q, lab, mask))
    got = H._search_grouped(w.hg, L, w.Q, ef, k, fill, True, sem=sem, flt=flt)
    print("%s: stages %s" % (ctx, dict(zip(*np.unique(want[3], return_counts=True)))))
    for name, a, b in zip(("ids", "dist", "labels"), got[:3], want[:3]):
        print("%s %s: %d of %d entries differ" % (ctx, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
    _same3(got, want, ctx=ctx)
    np.testing.assert_array_equal(got[5], want[3], err_msg=ctx)
    if want[4] is not None:
        np.testing.assert_array_equal(got[4], want[4], err_msg=ctx)
    last = int(mask.sum()) if mask is not None else int((lab >= 0).sum())
    nd = _plain_counts(H, w.hg, w.Q, want[6], sem) + np.where(want[3] == EXACT, np.uint32(last), np.uint32(0))
    np.testing.assert_array_equal(got[3], nd, err_msg=ctx)
    return want, got


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """2003 Gaussian vectors of 20 dimensions, hnsw_build with M 8, efC 40, 64 queries: the index of tests/test_gpu_filter.py"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.hg = H.Ohnsw.build_batch_bigarray(w.X, 8, 40, seed=7)
    assert w.hg.info().row_format == ROWS_F32
    w.g = _graph(oracle, w.hg)
    w.walks = Walks(oracle, w.g, oracle.Space.l2(w.X, arith=oracle.TREE16), w.Q)
    yield w
    w.hg.release()


def _cluster_data(seed, spread=CLUSTER_SPREAD):
    """40 Gaussian clusters of 100 points (node v in cluster v // 100), queries at the 40 centres and at 24 midpoints of centres"""
    rng = np.random.default_rng(seed)
    C = (spread * rng.normal(size=(CLUSTERS, D))).astype(np.float32)
    X = (np.repeat(C, PER, axis=0) + rng.normal(size=(CLUSTERS * PER, D))).astype(np.float32)
    pairs = rng.choice(CLUSTERS, size=(NQ - CLUSTERS, 2))
    Q = np.concatenate([C, ((C[pairs[:, 0]] + C[pairs[:, 1]]) / 2).astype(np.float32)])
    return X, Q


def _label_schemes(seed):
    """label = cluster; random labels, n_labels = n / 10; and eight coarse groups of five clusters each.  With clusters of 100
    points a full W_1024 holds nodes of eleven clusters at least, so under label = cluster no query can still be short at 1024:
    the coarse groups are what reaches the exact stage through the ladder."""
    n = CLUSTERS * PER
    cluster = (np.arange(n) // PER).astype(np.int32)
    rnd = np.random.default_rng(seed + 1000).integers(0, n // 10, n).astype(np.int32)
    return {"cluster": (cluster, CLUSTERS), "random": (rnd, n // 10), "coarse": ((cluster % 8).astype(np.int32), 8)}


def _class_counts(walks, schemes, ef=16, k=8):
    """queries served at stage 0, at a later stage, by the exact stage, over all label schemes (the restatement's stage test alone)"""
    s0 = later = exact = 0
    for lab, _ in schemes.values():
        for q in range(len(walks.Q)):
            st = EXACT
            for j, e in enumerate(_ladder(ef)):
                W = walks.get(0, e)[0][q]
                if len(np.unique(lab[W[W >= 0]])) >= k:
                    st = j
                    break
            s0, later, exact = s0 + (st == 0), later + (0 < st < EXACT), exact + (st == EXACT)
    return s0, later, exact


def _first_cluster_seed(H, oracle, limit=20):
    """how CLUSTER_SEED was chosen: builds the index of each seed, exports its graph and runs the restatement over the oracle's walks"""
    for seed in range(limit):
        X, Q = _cluster_data(seed)
        hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
        walks = Walks(oracle, _graph(oracle, hg), oracle.Space.l2(X, arith=oracle.TREE16), Q)
        counts = _class_counts(walks, _label_schemes(seed))
        hg.release()
        print("seed %d: stage 0 / later / exact = %s" % (seed, counts))
        if min(counts) >= 5:
            return seed
    return None


@pytest.fixture(scope="module")
def clusters(H, oracle):
    w = World()
    w.X, w.Q = _cluster_data(CLUSTER_SEED)
    w.hg = H.Ohnsw.build_batch_bigarray(w.X, 8, 40, seed=7)
    assert w.hg.info().row_format == ROWS_F32
    w.g = _graph(oracle, w.hg)
    w.walks = Walks(oracle, w.g, oracle.Space.l2(w.X, arith=oracle.TREE16), w.Q)
    w.schemes = _label_schemes(CLUSTER_SEED)
    yield w
    w.hg.release()


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------

def test_distinct_labels_are_the_plain_search(H, world):
    w = world
    L = w.hg.labels(np.arange(N))
    assert L.info() == (N, N, N)
    plain = H.Ohnsw.knn_batch_bigarray(w.hg, 10, w.Q, ef=32, counters=True)
    got = H.Ohnsw.knn_batch_grouped(w.hg, 10, w.Q, L, ef=32, counters=True)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), plain[1].view(np.uint32))
    np.testing.assert_array_equal(got[2], plain[0])              # a node's label is its id
    np.testing.assert_array_equal(got[3], plain[2])              # out_ndist
    np.testing.assert_array_equal(got[4], plain[3])              # out_nhops
    assert (got[5] == 0).all()
    L.release()
    one = w.hg.labels(np.zeros(N, np.int32))
    assert one.info() == (1, N, 1)
    plain = H.Ohnsw.knn_batch_bigarray(w.hg, 1, w.Q, ef=32)
    got = H.Ohnsw.knn_batch_grouped(w.hg, 1, w.Q, one, ef=32, counters=True)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), plain[1].view(np.uint32))
    assert (got[2] == 0).all() and (got[5] == 0).all()
    one.release()


# ---- 2. all three classes of stage ---------------------------------------------------------------------------------------------

def test_all_classes_of_stage(H, clusters):
    w = clusters
    s0 = later = exact = 0
    assert min(_class_counts(w.walks, w.schemes)) >= 5, _class_counts(w.walks, w.schemes)
    for name, (lab, n_labels) in w.schemes.items():
        L = w.hg.labels(lab, n_labels)
        want, got = _check(H, w, L, lab, 16, 8, ctx="labels by %s" % name)
        s0, later, exact = s0 + int((want[3] == 0).sum()), later + int(((want[3] > 0) & (want[3] != EXACT)).sum()), exact + int((want[3] == EXACT).sum())
        # every row holds eight distinct labels, each the label of its node
        assert all(len(set(r)) == 8 for r in got[2])
        np.testing.assert_array_equal(lab[got[0]], got[2])
        L.release()
    assert s0 >= 5 and later >= 5 and exact >= 5, (s0, later, exact)


# ---- 3. fewer groups than k ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0, 1])
def test_fewer_groups_than_k(H, world, fill):
    w = world
    lab = np.full(N, -1, np.int32)
    lab[::3] = (np.arange(len(lab[::3])) % 5).astype(np.int32)      # five groups over a third of the nodes, the others unlabelled
    L = w.hg.labels(lab, 9)
    n_labelled = int((lab >= 0).sum())
    assert L.info() == (9, n_labelled, 5)
    got = H._search_grouped(w.hg, L, w.Q, 16, 8, fill, True)
    assert (got[5] == EXACT).all() and (got[4] == 0).all() and (got[3] == n_labelled).all()      # no walk was made
    exact = _exact_grouped(H, w.hg, w.Q, lab)
    for q in range(NQ):
        ei, ed = exact(q)
        assert len(ei) == 5
        np.testing.assert_array_equal(got[0][q, :5], ei)
        np.testing.assert_array_equal(got[1][q, :5].view(np.uint32), ed.view(np.uint32))
        np.testing.assert_array_equal(got[2][q, :5], lab[ei])
    assert (got[0][:, 5:] == -1).all() and (got[2][:, 5:] == -1).all()
    gap = got[1][:, 5:]
    assert np.isnan(gap).all() if fill == 0 else (np.isinf(gap) & (gap > 0)).all()
    L.release()


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------

def test_ties(H, oracle):
    """integer coordinates; nodes 1000 .. 1099 duplicate nodes 0 .. 99 under DIFFERENT labels (both come back, equal distances by
    id), nodes 1100 .. 1199 duplicate nodes 100 .. 199 under the SAME label (the lowest id represents it)"""
    rng = np.random.default_rng(5)
    X = rng.integers(-6, 7, size=(N, D)).astype(np.float32)
    X[1000:1100] = X[0:100]
    X[1100:1200] = X[100:200]
    lab = (np.arange(N) % 700).astype(np.int32)
    lab[1000:1100] = lab[0:100] + 700
    lab[1100:1200] = lab[100:200]
    Q = np.concatenate([X[0:16], X[100:116], rng.integers(-6, 7, size=(32, D)).astype(np.float32)])
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    L = hg.labels(lab, 800)
    exact = _exact_grouped(H, hg, Q, lab)
    ids, dist, labs = H.Ohnsw.brute_force_grouped(hg, 10, Q, L)
    for q in range(NQ):
        ei, ed = exact(q)
        np.testing.assert_array_equal(ids[q], ei[:10], err_msg="query %d" % q)
        np.testing.assert_array_equal(dist[q].view(np.uint32), ed[:10].view(np.uint32))
        np.testing.assert_array_equal(labs[q], lab[ei[:10]])
    for q in range(16):
        assert list(ids[q, :2]) == [q, 1000 + q] and dist[q, 0] == 0 and dist[q, 1] == 0
        assert ids[16 + q, 0] == 100 + q and dist[16 + q, 0] == 0 and dist[16 + q, 1] > 0 and 1100 + q not in ids[16 + q]
    # the ladder over the same data: W's own order among equal distances is the oracle's canonical one
    w = World()
    w.hg, w.Q = hg, Q
    w.walks = Walks(oracle, _graph(oracle, hg), oracle.Space.l2(X, arith=oracle.TREE16), Q)
    want, got = _check(H, w, L, lab, 32, 10, ctx="ties")
    assert (want[3] == 0).sum() >= 32
    L.release()
    hg.release()


# ---- 5. the exact call ---------------------------------------------------------------------------------------------------------

def _integer_world(H, n, d, span, metric, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-span, span + 1, size=(n, d)).astype(np.float32)
    Q = rng.integers(-span, span + 1, size=(NQ, d)).astype(np.float32)
    return X, Q, H.Hgraph.flat(X, metric=metric)


def _expect_exact(H, hg, Q, lab, k, got, mask=None, ctx=""):
    exact = _exact_grouped(H, hg, Q, lab, mask)
    for q in range(len(Q)):
        ei, ed = exact(q)
        m = min(k, len(ei))
        np.testing.assert_array_equal(got[0][q, :m], ei[:m], err_msg="%s query %d" % (ctx, q))
        np.testing.assert_array_equal(got[1][q, :m].view(np.uint32), ed[:m].view(np.uint32), err_msg="%s query %d" % (ctx, q))
        np.testing.assert_array_equal(got[2][q, :m], lab[ei[:m]], err_msg="%s query %d" % (ctx, q))
        assert (got[0][q, m:] == -1).all() and (got[2][q, m:] == -1).all() and np.isnan(got[1][q, m:]).all()


def test_exact_call_slabs_batches_and_sparse_labels(H):
    X, Q, hg = _integer_world(H, N, D, 10, H.METRIC_L2, 11)
    lab = np.random.default_rng(12).integers(-1, 150, N).astype(np.int32)
    L = hg.labels(lab, 150)
    first = H.Ohnsw.brute_force_grouped(hg, 10, Q, L)
    _expect_exact(H, hg, Q, lab, 10, first, ctx="plain")
    for slabs in (1, 3, 1024, 0):
        hg.set_option("scan_slabs", slabs)
        again = H.Ohnsw.brute_force_grouped(hg, 10, Q, L)
        for a, b in zip(again, first):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="scan_slabs %d" % slabs)
    for nq in (1, 7, 64):
        part = H.Ohnsw.brute_force_grouped(hg, 10, Q[:nq], L)
        for a, b in zip(part, first):
            np.testing.assert_array_equal(a.view(np.uint32), b[:nq].view(np.uint32), err_msg="batch of %d" % nq)
    # k above the number of groups, both fills
    for fill in (H.FILL_OHNSW, H.FILL_BA):
        wide = H.Ohnsw.brute_force_grouped(hg, 200, Q[:7], L, fill=fill)
        groups = len(np.unique(lab[lab >= 0]))
        assert (wide[0][:, :groups] >= 0).all() and (wide[0][:, groups:] == -1).all() and (wide[2][:, groups:] == -1).all()
        gap = wide[1][:, groups:]
        assert np.isnan(gap).all() if fill == H.FILL_OHNSW else (np.isinf(gap) & (gap > 0)).all()
        for a, b in zip(wide, first):
            np.testing.assert_array_equal(a[:, :10].view(np.uint32), b[:7].view(np.uint32))
    L.release()
    # n_labels far larger than the labels in use: 1 000 000 cells of 8 bytes per query, so the 64 queries go in two pieces of 32
    far = hg.labels(np.where(lab >= 0, lab * 6000 + 17, -1), 1000000)
    assert far.info() == (1000000, int((lab >= 0).sum()), len(np.unique(lab[lab >= 0])))
    got = H.Ohnsw.brute_force_grouped(hg, 10, Q, far)
    np.testing.assert_array_equal(got[0], first[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), first[1].view(np.uint32))
    np.testing.assert_array_equal(got[2], np.where(first[2] >= 0, first[2] * 6000 + 17, -1))
    far.release()
    # every node its own label among 40 060 cells: a row picked from in three stripes, all of them holding real words -- the plain
    # exact scan's rows, each label its node's
    own = hg.labels(np.arange(N) * 20, 20 * N)
    got = H.Ohnsw.brute_force_grouped(hg, 10, Q, own)
    plain = H.Ohnsw.brute_force_knn(hg, 10, Q)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), plain[1].view(np.uint32))
    np.testing.assert_array_equal(got[2], plain[0] * 20)
    wide = H.Ohnsw.brute_force_grouped(hg, 1024, Q[:7], own)           # k above a stripe's share of the nodes
    plain = H.Ohnsw.brute_force_knn(hg, 1024, Q[:7])
    np.testing.assert_array_equal(wide[0], plain[0])
    np.testing.assert_array_equal(wide[1].view(np.uint32), plain[1].view(np.uint32))
    own.release()
    hg.release()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d,span", [(20, 10), (100, 5), (257, 3)])
def test_exact_call_shapes(H, d, span, metric):
    n = 1501
    X, Q, hg = _integer_world(H, n, d, span, H.METRIC_L2 if metric == "l2" else H.METRIC_IP, 20 + d)
    lab = np.random.default_rng(d).integers(-1, 60, n).astype(np.int32)
    L = hg.labels(lab, 60)
    _expect_exact(H, hg, Q, lab, 10, H.Ohnsw.brute_force_grouped(hg, 10, Q, L), ctx="d %d %s" % (d, metric))
    mask = _uniform_mask(d, 0.3, n)
    _expect_exact(H, hg, Q, lab, 10, H.Ohnsw.brute_force_grouped(hg, 10, Q, L, filter=mask), mask, ctx="d %d %s masked" % (d, metric))
    L.release()
    hg.release()


# ---- 6. with a filter ----------------------------------------------------------------------------------------------------------

def test_with_a_filter(H, world):
    w = world
    lab = np.random.default_rng(31).integers(-1, N // 10, N).astype(np.int32)
    L = w.hg.labels(lab, N // 10)
    mask = _uniform_mask(32, 0.5)
    flt = w.hg.filter(mask)
    want, got = _check(H, w, L, lab, 16, 10, mask=mask, flt=flt, ctx="half the nodes allowed")
    assert mask[got[0]].all() and len(np.unique(want[3])) > 1
    flt.release()
    # fewer allowed nodes than k: straight to the exact stage, no walk
    few = np.zeros(N, bool)
    few[[5, 700, 701, 2002]] = True
    lab2 = lab.copy()
    lab2[[5, 700, 701, 2002]] = [3, 4, 4, 9]
    L2 = w.hg.labels(lab2, N // 10)
    got = H.Ohnsw.knn_batch_grouped(w.hg, 10, w.Q, L2, ef=16, filter=few, counters=True)
    assert (got[5] == EXACT).all() and (got[4] == 0).all() and (got[3] == 4).all()
    _expect_exact(H, w.hg, w.Q, lab2, 10, got, few, ctx="four allowed")
    assert (np.sort(got[2][:, :3], axis=1) == [3, 4, 9]).all()
    L.release()
    L2.release()


# ---- 7. half, sq8 and sq8_dim rows ---------------------------------------------------------------------------------------------

class _PlainWalks:
    """W_e as the header's point 3 reads for the inexact rows, from public calls alone: hnsw_search_batch of (ef = e, k = e) on the
    same handle re-ranks ALL e members of W over the float32 rows, so its row is W_e re-ranked, and the eligible members in that
    order are the list G is taken over.  (ids, distances, hops) as Walks.get gives them."""

    def __init__(self, H, hg, Q):
        self.H, self.hg, self.Q, self._w = H, hg, np.asarray(Q, np.float32), {}

    def get(self, sem, e):
        assert sem == 0
        if e not in self._w:
            ids, dist, _, hops = self.H.Ohnsw.knn_batch_bigarray(self.hg, e, self.Q, ef=e, counters=True)
            self._w[e] = (ids, dist, hops)
        return self._w[e]


@pytest.mark.parametrize("rows", ["half_rows", "sq8_rows", "sq8_dim_rows"])
def test_inexact_rows_are_reranked_over_the_float32_rows(H, oracle, world, rows):
    w = world
    hg = H.Hgraph(w.X, w.hg.deg0, w.hg.nbr0, w.hg.upper, entry_point=w.hg.entry_point, max_degree=w.hg.max_degree)
    hg.set_option(rows, 1)
    if rows == "half_rows":
        assert hg.info().row_format == ROWS_HALF
        walks = Walks(oracle, w.g, oracle.Space.l2(w.X.astype(np.float16).astype(np.float32), arith=oracle.TREE16), w.Q)
    elif rows == "sq8_rows":
        assert hg.info().row_format == ROWS_SQ8
        B, lo, s = _quantise(w.X)
        walks = Walks(oracle, w.g, oracle.Space.l2(B.astype(np.float32), arith=oracle.TREE16), ((w.Q - lo) / s).astype(np.float32))
    else:
        assert hg.info().row_format == ROWS_SQ8_DIM
        walks = _PlainWalks(H, hg, w.Q)
    lab = np.random.default_rng(41).integers(-1, 40, N).astype(np.int32)
    L = hg.labels(lab, 40)
    key = _tree16_key(oracle, w.X, w.Q)
    for ef, k in ((32, 10), (16, 12)):
        ctx = "%s ef %d k %d" % (rows, ef, k)
        got = H.Ohnsw.knn_batch_grouped(hg, k, w.Q, L, ef=ef, counters=True)
        # the returned distances are hnsw_distance_batch's for the returned ids, ascending; the labels are the nodes' and distinct
        np.testing.assert_array_equal(H.Ohnsw.distance_l2(hg, w.Q, got[0]).view(np.uint32), got[1].view(np.uint32), err_msg=ctx)
        assert (np.diff(got[1], axis=1) >= 0).all()
        np.testing.assert_array_equal(lab[got[0]], got[2])
        assert all(len(set(r)) == k for r in got[2])
        want = restate(walks, lab, None, ef, k, 0, H.FILL_OHNSW, _exact_grouped(H, hg, w.Q, lab), key=None if rows == "sq8_dim_rows" else key)
        print("%s: stages %s" % (ctx, dict(zip(*np.unique(want[3], return_counts=True)))))
        _same3(got, want, ctx=ctx)
        np.testing.assert_array_equal(got[5], want[3], err_msg=ctx)
        np.testing.assert_array_equal(got[4], want[4], err_msg=ctx)
        # evaluations: the walks taken (the plain search of (e, e) over the same rows; sq8: minus the e it re-ranks itself), plus
        # the members re-ranked at every stage walked
        cache, nd = {}, np.zeros(NQ, np.uint32)
        for q, es in enumerate(want[6]):
            for e in es:
                if e not in cache:
                    cache[e] = H.Ohnsw.knn_batch_bigarray(hg, e, w.Q, ef=e, counters=True)[2] - np.uint32(0 if rows == "half_rows" else e)
                nd[q] += cache[e][q]
        np.testing.assert_array_equal(got[3], nd + want[5], err_msg=ctx)
        assert len(np.unique(want[3])) > 1 or ef == 32
    L.release()
    hg.release()


# ---- 8. functor semantics ------------------------------------------------------------------------------------------------------

def test_functor_semantics(H, world):
    w = world
    lab = np.random.default_rng(51).integers(0, 12, N).astype(np.int32)
    L = w.hg.labels(lab, 12)           # twelve groups, k 10, W of 16: some queries are served at once, others climb
    want, got = _check(H, w, L, lab, 16, 10, sem=1, ctx="functor rule")
    assert len(np.unique(want[3])) > 1
    # the Hnsw.Ba front: the same rows, +inf fill
    ba = H.Ba.knn_batch_grouped(w.hg, w.Q, 16, 10, L, counters=True)
    for a, b in zip(ba, got):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    L.release()


# ---- 9. marks and staleness ----------------------------------------------------------------------------------------------------

def test_marks_and_staleness(H, world):
    w = world
    hg = H.Ohnsw.build_batch_bigarray(w.X[:1000], 8, 40, seed=7)
    lab = (np.arange(1000) % 50).astype(np.int32)
    marked = np.arange(0, 1000, 7)
    hg.mark_deleted(marked)
    L = hg.labels(lab, 50)
    held = L.get()
    assert (held[marked] == -1).all() and (np.delete(held, marked) == np.delete(lab, marked)).all()
    assert L.info() == (50, 1000 - len(marked), 50)
    got = H.Ohnsw.knn_batch_grouped(hg, 10, w.Q, L, ef=32)
    assert (got[0] >= 0).all() and not np.isin(got[0], marked).any()
    np.testing.assert_array_equal(lab[got[0]], got[2])
    x = H.Ohnsw.brute_force_grouped(hg, 50, w.Q, L)
    assert (x[0] >= 0).all() and not np.isin(x[0], marked).any()
    _expect_exact(H, hg, w.Q, held, 50, x, ctx="marked")

    def stale(labels):
        with pytest.raises(H.InvalidArgument, match="stale"):
            H.Ohnsw.knn_batch_grouped(hg, 10, w.Q, labels, ef=32)
        with pytest.raises(H.InvalidArgument, match="stale"):
            H.Ohnsw.brute_force_grouped(hg, 10, w.Q, labels)

    hg.mark_deleted([1])
    stale(L)
    L2 = hg.labels(lab, 50)
    hg.unmark_deleted([1])
    stale(L2)
    L3 = hg.labels(lab, 50)
    H.Ohnsw.insert_batch(hg, w.X[1000:1010], 8, 40, seed=7)
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_grouped(hg, 10, w.Q, L3, ef=32)
    L4 = hg.labels(np.arange(1010) % 50, 50)
    H.Ohnsw.remove_batch(hg, [1009])
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_grouped(hg, 10, w.Q, L4, ef=32)
    # labels made for another handle
    mine = w.hg.labels(np.arange(N) % 50, 50)
    other = H.Hgraph.flat(w.X)
    with pytest.raises(H.InvalidArgument, match="another index"):
        H.Ohnsw.brute_force_grouped(other, 10, w.Q, mine)
    assert (H.Ohnsw.knn_batch_grouped(w.hg, 10, w.Q, mine, ef=32)[0] >= 0).all()
    for o in (L, L2, L3, L4, mine):
        o.release()
    other.release()
    hg.release()


# ---- 10. determinism -----------------------------------------------------------------------------------------------------------

def test_result_does_not_depend_on_the_batch(H, clusters):
    w = clusters
    lab, n_labels = w.schemes["coarse"]
    L = w.hg.labels(lab, n_labels)
    whole = H.Ohnsw.knn_batch_grouped(w.hg, 8, w.Q, L, ef=16, counters=True)
    assert len(np.unique(whole[5])) > 1
    a = H.Ohnsw.knn_batch_grouped(w.hg, 8, w.Q[:NQ // 2], L, ef=16, counters=True)
    b = H.Ohnsw.knn_batch_grouped(w.hg, 8, w.Q[NQ // 2:], L, ef=16, counters=True)
    r = H.Ohnsw.knn_batch_grouped(w.hg, 8, w.Q[::-1], L, ef=16, counters=True)
    for x, y, z, full in zip(a, b, r, whole):
        np.testing.assert_array_equal(np.concatenate([x, y]).view(np.uint32), full.view(np.uint32))
        np.testing.assert_array_equal(z[::-1].view(np.uint32), full.view(np.uint32))
    # page-locked query matrix, read in place
    Qp = H.host_empty((NQ, D))
    Qp[:] = w.Q
    pinned = H.Ohnsw.knn_batch_grouped(w.hg, 8, Qp, L, ef=16, counters=True)
    for x, full in zip(pinned, whole):
        np.testing.assert_array_equal(x.view(np.uint32), full.view(np.uint32))
    L.release()


# ---- 11. errors ----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(H, world):
    w = world
    Lib = H.load()
    lab = (np.arange(N) % 100).astype(np.int32)
    L = w.hg.labels(lab, 100)
    flt = w.hg.filter(np.ones(N, bool))
    ids = np.full((NQ, 10), 77, np.int32)
    dist = np.full((NQ, 10), 7.5, np.float32)
    labs = np.full((NQ, 10), 55, np.int32)
    cnt = [np.full(NQ, 9, np.uint32) for _ in range(3)]

    def untouched():
        assert (ids == 77).all() and (dist == 7.5).all() and (labs == 55).all() and all((c == 9).all() for c in cnt)

    def call(hg, l, f=None, ef=16, k=10, sem=0, nq=NQ, qs=D, q=w.Q, out=ids, refused=True):
        p = H._SearchParams(ef, k, H.FILL_OHNSW, sem)
        rc = Lib.hnsw_search_batch_grouped(hg.handle, l.handle if l is not None else None, f.handle if f is not None else None,
                                           q.ctypes.data if q is not None else None, nq, qs, ctypes.byref(p),
                                           out.ctypes.data if out is not None else None, dist.ctypes.data, labs.ctypes.data,
                                           cnt[0].ctypes.data, cnt[1].ctypes.data, cnt[2].ctypes.data)
        if refused:
            untouched()
        return rc

    def scan(hg, l, f=None, k=10, fill=0, nq=NQ, qs=D, refused=True):
        rc = Lib.hnsw_brute_force_batch_grouped(hg.handle, l.handle if l is not None else None, f.handle if f is not None else None,
                                                w.Q.ctypes.data, nq, qs, k, fill, ids.ctypes.data, dist.ctypes.data, labs.ctypes.data)
        if refused:
            untouched()
        return rc

    assert call(w.hg, L, ef=8, k=10) == H.ERR_BAD_ARG                       # k > ef
    assert call(w.hg, L, ef=1025, k=10) == H.ERR_UNSUPPORTED
    assert call(w.hg, L, sem=H.SEM_FUNCTOR_NEAREST_K) == H.ERR_BAD_ARG
    assert call(w.hg, None) == H.ERR_BAD_ARG                                # null labels
    assert call(w.hg, L, qs=D - 1) == H.ERR_BAD_ARG                         # strides
    assert call(w.hg, L, q=None) == H.ERR_BAD_ARG and call(w.hg, L, out=None) == H.ERR_BAD_ARG
    assert call(w.hg, L, nq=-1) == H.ERR_BAD_ARG
    assert call(w.hg, L, nq=0) == H.OK                                      # a no-op
    other = H.Hgraph.flat(w.X)
    foreign, foreign_f = other.labels(lab, 100), other.filter(np.ones(N, bool))
    assert call(w.hg, foreign) == H.ERR_BAD_ARG and call(w.hg, L, foreign_f) == H.ERR_BAD_ARG
    assert scan(w.hg, foreign) == H.ERR_BAD_ARG and scan(w.hg, L, foreign_f) == H.ERR_BAD_ARG and scan(w.hg, None) == H.ERR_BAD_ARG
    assert scan(w.hg, L, k=0) == H.ERR_BAD_ARG and scan(w.hg, L, k=1025) == H.ERR_UNSUPPORTED and scan(w.hg, L, fill=2) == H.ERR_BAD_ARG
    assert scan(w.hg, L, qs=D - 1) == H.ERR_BAD_ARG and scan(w.hg, L, nq=0) == H.OK
    empty = H.Hgraph(w.X[:3], [0, 0, 0], [[-1], [-1], [-1]], entry_point=None, max_degree=1)
    el = empty.labels([0, 1, 2], 3)
    assert call(empty, el) == H.ERR_EMPTY_INDEX
    assert scan(empty, el, k=3, nq=1, refused=False) == H.OK and sorted(ids.ravel()[:3]) == [0, 1, 2]       # the exact call needs no graph
    ids.ravel()[:3], dist.ravel()[:3], labs.ravel()[:3] = 77, 7.5, 55
    # creation: every refusal is found on the host and leaves *out NULL
    for bad, n_labels, n in ((lab, 0, N), (lab, 100, N - 1), (np.where(lab == 5, 100, lab), 100, N), (np.where(lab == 5, -2, lab), 100, N)):
        out = ctypes.c_void_p(7)
        bad = np.ascontiguousarray(bad, np.int32)
        assert Lib.hnsw_labels_create(w.hg.handle, bad.ctypes.data, n, n_labels, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    before = w.hg.info().device_bytes
    more = [w.hg.labels(lab, 100) for _ in range(3)]
    assert w.hg.info().device_bytes == before                               # label objects are not index tables
    # everything still works after all that
    assert call(w.hg, L, flt, refused=False) == H.OK and (ids != 77).all()
    for o in more + [L, flt, foreign, foreign_f, el]:
        o.release()
    other.release()
    empty.release()


# ---- 12. the C++ front end -----------------------------------------------------------------------------------------------------

def test_cpp_front_end_grouped(H, tmp_path):
    from conftest import ROOT
    exe = str(tmp_path / "test_front_grouped")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_grouped.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "grouped front-end ok" in out.stdout, out.stdout + out.stderr


if __name__ == "__main__":      # python tests/test_gpu_grouped.py: prints the value CLUSTER_SEED was fixed to (needs the device)
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
    print("CLUSTER_SEED", _first_cluster_seed(H_, o_))
