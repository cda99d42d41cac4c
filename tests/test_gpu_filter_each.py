"""One filter per query (hnsw_search_batch_filtered_each) and filters from labels (hnsw_filter_create_by_label, hnsw_filter_bits),
ocaml-hnsw_amd/csrc/hnsw_filter.hip.

The yardstick is the single-filter call on the same handle, which tests/test_gpu_filter.py holds against the oracle: row q of all
five outputs of the per-query call is bit for bit the row hnsw_search_batch_filtered gives query q under filters[which[q]].  Every
query of every case is compared: ids equal, distances bit-equal, ndist, nhops and stage equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_HALF, ROWS_SQ8 = 0, 4, 5
EXACT = 0xFFFFFFFF
N, D, NQ = 2003, 20, 64           # the index of test_gpu_filter.py: n is no multiple of 32; NCH 1, scan tiles of 8 queries
LADDER_MASK_SEED = 20             # ... and its uniform 10 % mask that serves some query at stage 0 or 1
NAMES = ("ids", "dist", "ndist", "nhops", "stage")


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _uniform_mask(seed, p, n=N):
    return np.random.default_rng(seed).random(n) < p


def _mask_of(nodes, n=N):
    m = np.zeros(n, bool)
    m[list(nodes)] = True
    return m


def _one_based(H, hg, X):
    """the same graph as a 1-based index: the Hnsw.Ba-style front (functor rule, +inf fill)"""
    hg.export()
    up = [(nodes + 1, deg, np.where(nbr >= 0, nbr + 1, -1)) for nodes, deg, nbr in hg.upper]
    return H.Hgraph(X, hg.deg0, np.where(hg.nbr0 >= 0, hg.nbr0 + 1, -1), up, entry_point=hg.entry_point + 1, id_base=1,
                    max_degree=hg.max_degree)


def _assert_rows(got, refs, which, ctx=""):
    """row q of each output of `got` is row q of refs[which[q]]'s, as bits"""
    assert len(got) == 5
    for j, name in enumerate(NAMES):
        want = np.stack([refs[f][j][q] for q, f in enumerate(which)]) if len(which) else got[j]
        np.testing.assert_array_equal(got[j].view(np.uint32), want.view(np.uint32), err_msg="%s %s" % (ctx, name))


def _classes(ref):
    """per query of a single-filter result: 0 served at stage 0, 1 at a later ladder stage, 2 the exact stage after the whole
    ladder, 3 the exact stage without a walk"""
    stage, nhops = ref[4], ref[3]
    return np.where(stage == 0, 0, np.where(stage != EXACT, 1, np.where(nhops > 0, 2, 3)))


def _choose_which(refs):
    """Which filter each query takes, from the single-filter results alone: q % 4, then for every class of _classes missing among
    the selected rows one more query is given a filter under which it has that class (first such (query, filter); a query that is
    the chosen representative of a class is not reassigned)."""
    nq = len(refs[0][0])
    cls = np.stack([_classes(r) for r in refs])               # [filter][query]
    which = np.arange(nq) % len(refs)
    pinned = set()
    for c in range(4):
        have = [q for q in range(nq) if cls[which[q], q] == c]
        if have:
            pinned.add(have[0])
    for c in range(4):
        if any(cls[which[q], q] == c for q in range(nq)):
            continue
        for q in range(nq):
            fs = [f for f in range(len(refs)) if cls[f, q] == c]
            if q not in pinned and fs:
                which[q] = fs[0]
                pinned.add(q)
                break
    return which.astype(np.int32), np.array([cls[which[q], q] for q in range(nq)])


class World:
    pass


@pytest.fixture(scope="module")
def world(H):
    """2003 Gaussian vectors of 20 dimensions, hnsw_build with M 8, efC 40, 64 queries; the four masks of case 1"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.hg = H.Ohnsw.build_batch_bigarray(w.X, 8, 40, seed=7)
    assert w.hg.info().row_format == ROWS_F32
    w.masks = [_uniform_mask(11, 0.5), _uniform_mask(LADDER_MASK_SEED, 0.1),
               _mask_of(np.random.default_rng(21).choice(N, 20, replace=False)), _mask_of([5, 700, 2002])]
    w.filters = [w.hg.filter(m) for m in w.masks]
    # the reference, computed once: the four single-filter calls over all 64 queries, per accept rule
    w.refs = {sem: [H._search_filtered(w.hg, f, w.Q, 16, 10, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=sem) for f in w.filters]
              for sem in (0, 1)}
    w.which, w.classes = _choose_which(w.refs[0])
    yield w
    for f in w.filters:
        f.release()
    w.hg.release()


# ---- 1. mixed stages, both accept rules ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [0, 1])
def test_mixed_stages(H, world, sem):
    w = world
    which, classes = (w.which, w.classes) if sem == 0 else _choose_which(w.refs[1])
    print("rule %d: classes %s, filters %s" % (sem, np.bincount(classes, minlength=4), np.bincount(which, minlength=4)))
    # a stage 0, a stage in 1 .. 6, an exact-stage query that walked and one that did not, all in ONE call
    assert set(classes) == {0, 1, 2, 3}, np.bincount(classes, minlength=4)
    got = H._search_filtered_each(w.hg, w.filters, which, w.Q, 16, 10, H.FILL_BA if sem else H.FILL_OHNSW, True, sem=sem)
    _assert_rows(got, w.refs[sem], which, "rule %d" % sem)
    nowalk = classes == 3
    assert (got[4][nowalk] == EXACT).all() and (got[3][nowalk] == 0).all() and (got[2][nowalk] == 3).all()


# ---- 2. tile and group edges of the exact stage --------------------------------------------------------------------------------

def _edge_case(H, hg, X, Q, sizes, n):
    """five disjoint filters of three nodes (nobody walks: k = 10), a sixth of none that one query uses and a seventh no query
    uses; groups of `sizes` queries (+ the one of the sixth) dealt out through a fixed permutation, so that no group is contiguous
    in query order; the Ohnsw front (0-based, NaN fill) and the Ba front (1-based, +inf fill)"""
    nq = len(Q)
    assert sum(sizes) + 1 == nq
    node_sets = [[i, n // 3 + i, n - 1 - i] for i in range(5)] + [[], []]
    perm = np.random.default_rng(5).permutation(nq)
    which = np.zeros(nq, np.int32)
    at = 0
    for f, size in enumerate(list(sizes) + [1]):
        which[perm[at:at + size]] = f
        at += size
    assert (np.diff(np.flatnonzero(which == 4)) > 1).any()                       # not contiguous
    hg1 = _one_based(H, hg, X)
    for g, id_base in ((hg, 0), (hg1, 1)):
        filters = [g.filter(np.array(s, np.int64) + id_base) for s in node_sets]
        assert [f.count() for f in filters] == [3, 3, 3, 3, 3, 0, 0]
        if id_base == 0:
            refs = [H.Ohnsw.knn_batch_filtered(g, 10, Q, f, ef=16, counters=True) for f in filters]
            got = H.Ohnsw.knn_batch_filtered_each(g, 10, Q, filters, which, ef=16, counters=True)
        else:
            refs = [H.Ba.knn_batch_filtered(g, Q, 16, 10, f, counters=True) for f in filters]
            got = H.Ba.knn_batch_filtered_each(g, Q, 16, 10, filters, which, counters=True)
        _assert_rows(got, refs, which, "id_base %d" % id_base)
        assert (got[4] == EXACT).all() and (got[3] == 0).all()
        np.testing.assert_array_equal(got[2], np.where(which == 5, 0, 3))         # ndist: the query's own filter's n_allowed
        for q in range(nq):
            want = sorted(v + id_base for v in node_sets[which[q]])
            assert sorted(got[0][q][got[0][q] >= 0]) == want
            gap = got[1][q, len(want):]
            assert np.isnan(gap).all() if id_base == 0 else (np.isinf(gap) & (gap > 0)).all()
        for f in filters:
            f.release()
    hg1.release()


def test_exact_stage_tiles_and_groups(H, world):
    # NCH 1, tiles of 8: groups of 1, 7, 8, 9 and 39 queries
    _edge_case(H, world.hg, world.X, _floats(65, D, 2), (1, 7, 8, 9, 39), N)


@pytest.mark.parametrize("d,sizes", [(130, (1, 3, 4, 5, 51)), (450, (1, 7, 8, 9, 39))])
def test_exact_stage_tiles_and_groups_wider_rows(H, d, sizes):
    # d 130: NCH 4, tiles of 4 queries in registers; d 450: NCH 8, tiles of 8 shared through LDS
    n = 600
    X, Q = _floats(n, d, 41), _floats(65, d, 42)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    _edge_case(H, hg, X, Q, sizes, n)
    hg.release()


def test_exact_stage_in_more_than_one_piece(H):
    """more rows than one scan launch takes (16 384): the second piece's tiles read their filters from the tile table's middle.
    Cheap: 600 nodes of 8 dimensions, nobody walks."""
    n, nq = 600, 20001
    X, Q = _floats(n, 8, 51), _floats(nq, 8, 52)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    filters = [hg.filter(np.array(s)) for s in ([0, 200, 599], [1, 201, 598], [2, 202, 597, 31, 32])]
    which = np.random.default_rng(53).integers(0, 3, nq).astype(np.int32)
    refs = [H.Ohnsw.knn_batch_filtered(hg, 10, Q, f, ef=16, counters=True) for f in filters]
    got = H.Ohnsw.knn_batch_filtered_each(hg, 10, Q, filters, which, ef=16, counters=True)
    for j, name in enumerate(NAMES):
        want = np.choose(which.reshape((-1,) + (1,) * (refs[0][j].ndim - 1)), [r[j].view(np.uint32) for r in refs])
        np.testing.assert_array_equal(got[j].view(np.uint32), want, err_msg=name)
    assert (got[4] == EXACT).all() and (got[2] == np.array([3, 3, 5])[which]).all()
    for f in filters:
        f.release()
    hg.release()


# ---- 3. half and sq8 rows: the re-rank path with per-query padding -------------------------------------------------------------

@pytest.mark.parametrize("rows", ["half_rows", "sq8_rows"])
def test_compact_rows(H, world, rows):
    w = world
    w.hg.export()
    hg = H.Hgraph(w.X, w.hg.deg0, w.hg.nbr0, w.hg.upper, entry_point=w.hg.entry_point, max_degree=w.hg.max_degree)
    hg.set_option(rows, 1)
    assert hg.info().row_format == (ROWS_HALF if rows == "half_rows" else ROWS_SQ8)
    filters = [hg.filter(m) for m in w.masks]
    refs = [H.Ohnsw.knn_batch_filtered(hg, 10, w.Q, f, ef=16, counters=True) for f in filters]
    got = H.Ohnsw.knn_batch_filtered_each(hg, 10, w.Q, filters, w.which, ef=16, counters=True)
    _assert_rows(got, refs, w.which, rows)
    assert (got[4] == EXACT).any() and (got[4] != EXACT).any()
    for f in filters:
        f.release()
    hg.release()


# ---- 4. batch independence -----------------------------------------------------------------------------------------------------

def test_result_does_not_depend_on_the_batch(H, world):
    w = world
    whole = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, w.filters, w.which, ef=16, counters=True)
    _assert_rows(whole, w.refs[0], w.which, "whole")
    # permuting queries and which together permutes the rows
    perm = np.random.default_rng(9).permutation(NQ)
    moved = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q[perm], w.filters, w.which[perm], ef=16, counters=True)
    for a, b, name in zip(moved, whole, NAMES):
        np.testing.assert_array_equal(a.view(np.uint32), b[perm].view(np.uint32), err_msg="permuted " + name)
    # the two halves of the batch, called separately
    for lo, hi in ((0, NQ // 2), (NQ // 2, NQ)):
        part = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q[lo:hi], w.filters, w.which[lo:hi], ef=16, counters=True)
        for a, b, name in zip(part, whole, NAMES):
            np.testing.assert_array_equal(a.view(np.uint32), b[lo:hi].view(np.uint32), err_msg="half " + name)
    # a table of one filter with which all 0 is the single-filter call
    for f in range(4):
        one = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, [w.filters[f]], np.zeros(NQ, np.int32), ef=16, counters=True)
        _assert_rows(one, [w.refs[0][f]], np.zeros(NQ, np.int32), "table of one, filter %d" % f)
    # a handle twice in the table
    twice = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, w.filters + w.filters, w.which + 4 * (np.arange(NQ) % 2).astype(np.int32),
                                            ef=16, counters=True)
    _assert_rows(twice, w.refs[0], w.which, "twice")
    # page-locked matrices, read and written in place
    Qp = H.host_empty((NQ, D))
    Qp[:] = w.Q
    out = (H.host_empty((NQ, 10), np.int32), H.host_empty((NQ, 10), np.float32))
    pinned = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, Qp, w.filters, w.which, ef=16, out=out)
    assert pinned[0] is out[0] and pinned[1] is out[1]
    np.testing.assert_array_equal(pinned[0], whole[0])
    np.testing.assert_array_equal(pinned[1].view(np.uint32), whole[1].view(np.uint32))


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(H, world):
    w = world
    L = H.load()
    ids = np.full((NQ, 10), 77, np.int32)
    dist = np.full((NQ, 10), 7.5, np.float32)
    cnt = [np.full(NQ, 9, np.uint32) for _ in range(3)]
    ok_which = (np.arange(NQ) % 2).astype(np.int32)

    def call(hg, filters, which, ef=16, k=10, sem=0, n_filters=None, nq=NQ, null_table=False):
        table = (ctypes.c_void_p * max(len(filters), 1))(*[f.handle if f is not None else None for f in filters])
        p = H._SearchParams(ef, k, H.FILL_OHNSW, sem)
        rc = L.hnsw_search_batch_filtered_each(hg.handle, None if null_table else table, len(filters) if n_filters is None else n_filters,
                                               which.ctypes.data if which is not None else None, w.Q.ctypes.data, nq, D, ctypes.byref(p),
                                               ids.ctypes.data, dist.ctypes.data, cnt[0].ctypes.data, cnt[1].ctypes.data, cnt[2].ctypes.data)
        assert (ids == 77).all() and (dist == 7.5).all() and all((c == 9).all() for c in cnt)
        return rc

    a, b = w.filters[0], w.filters[1]
    # the table and which
    assert call(w.hg, [a, b], ok_which, n_filters=0) == H.ERR_BAD_ARG
    assert call(w.hg, [a, b], ok_which, n_filters=-1) == H.ERR_BAD_ARG
    assert call(w.hg, [a, b], ok_which, null_table=True) == H.ERR_BAD_ARG
    assert call(w.hg, [a, b], None) == H.ERR_BAD_ARG
    for bad in (-1, 2, 2 ** 31 - 1):
        which = ok_which.copy()
        which[NQ - 1] = bad
        assert call(w.hg, [a, b], which) == H.ERR_BAD_ARG
    # an entry no query names: null, from another handle, outgrown
    assert call(w.hg, [a, b, None], ok_which) == H.ERR_BAD_ARG
    other = H.Hgraph.flat(w.X)
    foreign = other.filter(np.ones(N, bool))
    assert call(w.hg, [a, b, foreign], ok_which) == H.ERR_BAD_ARG
    assert call(w.hg, [foreign, b], ok_which) == H.ERR_BAD_ARG
    grown = H.Ohnsw.build_batch_bigarray(w.X[:500], 8, 40, seed=7)
    old = [grown.filter(np.ones(500, bool)), grown.filter(_uniform_mask(3, 0.5, 500))]
    assert (H.Ohnsw.knn_batch_filtered_each(grown, 10, w.Q, old, ok_which, ef=16)[0] >= 0).all()      # valid until the index grows
    H.Ohnsw.insert_batch(grown, w.X[500:520], 8, 40, seed=7)
    new = grown.filter(np.ones(520, bool))
    assert call(grown, [new, new, old[0]], ok_which) == H.ERR_BAD_ARG
    assert (H.Ohnsw.knn_batch_filtered_each(grown, 10, w.Q, [new, new], ok_which, ef=16)[0] >= 0).all()
    # the parameters
    assert call(w.hg, [a, b], ok_which, ef=8, k=10) == H.ERR_BAD_ARG
    assert call(w.hg, [a, b], ok_which, ef=1025, k=10) == H.ERR_UNSUPPORTED
    assert call(w.hg, [a, b], ok_which, sem=H.SEM_FUNCTOR_NEAREST_K) == H.ERR_BAD_ARG
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, [a, b], ok_which, ef=8)
    with pytest.raises(H.Failure):
        H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, [a, b], ok_which, ef=1025)
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, [a, b], ok_which[:5], ef=16)
    # an empty index
    empty = H.Hgraph(w.X[:3], [0, 0, 0], [[-1], [-1], [-1]], entry_point=None, max_degree=1)
    ef_ = empty.filter(np.ones(3, bool))
    assert call(empty, [ef_, ef_], ok_which) == H.ERR_EMPTY_INDEX
    # no queries: a no-op, which may be null
    assert call(w.hg, [a, b], None, nq=0) == H.OK
    # and the call still works after all that
    got = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, w.filters, w.which, ef=16, counters=True)
    _assert_rows(got, w.refs[0], w.which, "after the errors")
    for f in [foreign, ef_, new] + old:
        f.release()
    for h in (other, empty, grown):
        h.release()


# ---- 6. filters by label -------------------------------------------------------------------------------------------------------

def _check_labels(H, hg, labels, n_labels):
    n = len(labels)
    before = hg.info().device_bytes
    filters = hg.filters_by_label(labels, n_labels)
    assert len(filters) == n_labels and hg.info().device_bytes == before       # the masks are not index tables
    counts = np.bincount(labels[labels >= 0], minlength=n_labels)
    for l, f in enumerate(filters):
        assert f.count() == counts[l], l
        bits = f.bits()
        assert bits.dtype == np.uint32
        np.testing.assert_array_equal(bits, H.pack_allow(labels == l, n), err_msg="label %d" % l)
    return filters


def test_filters_by_label(H, world):
    w = world
    labels = np.random.default_rng(31).integers(-1, 5, N)
    filters = _check_labels(H, w.hg, labels, 6)                 # label 5: no node
    assert filters[5].count() == 0 and not filters[5].bits().any()
    # an ordinary filter gives its bits back too, and both kinds serve both entry points alike
    for l in (0, 4, 5):
        plain = w.hg.filter(labels == l)
        np.testing.assert_array_equal(plain.bits(), H.pack_allow(labels == l, N))
        a = H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, filters[l], ef=16, counters=True)
        b = H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q, plain, ef=16, counters=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
        plain.release()
    # the default n_labels: max label + 1
    assert len(w.hg.filters_by_label(labels)) == 5
    # each filter is released on its own: the others go on working
    filters[0].release()
    filters[2].release()
    assert filters[1].count() == int((labels == 1).sum())
    np.testing.assert_array_equal(filters[3].bits(), H.pack_allow(labels == 3, N))
    # n_labels 1: everybody or nobody
    one = _check_labels(H, w.hg, np.where(np.arange(N) % 3 == 0, -1, 0), 1)
    assert one[0].count() == N - (N + 2) // 3
    # a label outside -1 .. n_labels - 1: nothing is made
    L = H.load()
    for bad in (6, -2):
        lab = labels.astype(np.int32)
        lab[N - 1] = bad
        out = (ctypes.c_void_p * 6)(*([1] * 6))
        assert L.hnsw_filter_create_by_label(w.hg.handle, lab.ctypes.data, N, 6, out) == H.ERR_BAD_ARG
        assert [out[i] for i in range(6)] == [None] * 6
        with pytest.raises(H.InvalidArgument):
            w.hg.filters_by_label(lab, 6)
    out = (ctypes.c_void_p * 6)(*([1] * 6))
    assert L.hnsw_filter_create_by_label(w.hg.handle, labels.astype(np.int32).ctypes.data, N - 1, 6, out) == H.ERR_BAD_ARG      # n is not the index's
    assert [out[i] for i in range(6)] == [None] * 6


@pytest.mark.parametrize("n", [33, 64])
def test_filters_by_label_word_edges(H, n):
    hg = H.Hgraph.flat(_floats(n, 8, 3))
    labels = np.random.default_rng(n).integers(-1, 3, n)
    labels[[0, 31, 32, n - 1]] = [0, 1, 2, 1]
    _check_labels(H, hg, labels, 3)
    _check_labels(H, hg, np.full(n, 2), 3)                      # every node under one label: whole words set, the others empty
    hg.release()


# ---- 7. the tenant flow end to end ---------------------------------------------------------------------------------------------

def test_tenants_in_one_call(H, world):
    w = world
    tenant_of_node = np.random.default_rng(41).integers(0, 5, N)
    filters = w.hg.filters_by_label(tenant_of_node, 5)
    which = np.random.default_rng(42).integers(0, 5, NQ).astype(np.int32)
    got = H.Ohnsw.knn_batch_filtered_each(w.hg, 10, w.Q, filters, which, ef=16, counters=True)
    assert ((got[0] >= 0).all(1)).all()
    assert (tenant_of_node[got[0]] == which[:, None]).all()     # every neighbour is the query's tenant's
    for t in range(5):                                          # the loop the one call replaces
        mine = np.flatnonzero(which == t)
        ref = H.Ohnsw.knn_batch_filtered(w.hg, 10, w.Q[mine], filters[t], ef=16, counters=True)
        for a, b, name in zip(got, ref, NAMES):
            np.testing.assert_array_equal(a[mine].view(np.uint32), b.view(np.uint32), err_msg="tenant %d %s" % (t, name))


# ---- 8. the C++ front end ------------------------------------------------------------------------------------------------------

def test_cpp_front_end_filter_each(H, tmp_path):
    exe = str(tmp_path / "test_front_filter_each")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_filter_each.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "filter-each front-end ok" in out.stdout, out.stdout + out.stderr
