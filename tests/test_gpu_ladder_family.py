"""What the ladder's one driver (Ladder::run, ocaml-hnsw_amd/csrc/hnsw_filter.hip) guarantees across the searches that climb it.

The filtered call, the paged call from HNSW_CURSOR_START and the grouped call with every node its own label have the same serve
condition under one mask -- k allowed members in W -- and the same exact stage, so on float32 rows they walk the same queries at
the same stages: per query out_stage, out_ndist and out_nhops are equal across the three, and so are the rows as sets of
(distance, id) pairs (the paged call orders equal distances by id, the others keep W's order).

The world is the clustered one of tests/test_gpu_grouped.py at d = 16 -- 40 clusters of 100 points, queries at the centres and
at midpoints of centres -- with every coordinate a multiple of 1/4: such values are exact as halves and their squared distances
are exact in float32 whatever the order of the sum, so the half-row twin of the index walks bit for bit what the float32 rows
walk.  The mask allows cluster 0 and every 199th node, one node in 33: a query inside cluster 0 is served by W_16, a query whose
W reaches cluster 0 by 1024 at a stage in between, the others by the exact stage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT = 0xFFFFFFFF
ROWS_F32, ROWS_HALF = 0, 4
CLUSTERS, PER, D, NQ = 40, 100, 16, 64
N = CLUSTERS * PER
EF, K = 16, 10


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _quarters(a):
    return (np.round(4 * a) / 4).astype(np.float32)


def _data(seed=0, spread=3.0):
    rng = np.random.default_rng(seed)
    C = _quarters(spread * rng.normal(size=(CLUSTERS, D)))
    X = _quarters(np.repeat(C, PER, axis=0) + rng.normal(size=(N, D)))
    pairs = rng.choice(CLUSTERS, size=(NQ - CLUSTERS, 2))
    Q = np.concatenate([C, _quarters((C[pairs[:, 0]] + C[pairs[:, 1]]) / 2)])
    return X, Q


def _sparse_mask():
    allow = np.zeros(N, bool)
    allow[:PER] = True
    allow[::199] = True
    return allow


class World:
    pass


@pytest.fixture(scope="module")
def world(H):
    w = World()
    w.X, w.Q = _data()
    assert np.array_equal(w.X.astype(np.float16).astype(np.float32), w.X)
    w.hg = H.Ohnsw.build_batch_bigarray(w.X, 8, 40, seed=7)
    assert w.hg.info().row_format == ROWS_F32
    w.labels = w.hg.labels(np.arange(N, dtype=np.int32), N)
    w.calls = {}
    yield w
    w.labels.release()
    w.hg.release()


def _three(H, hg, labels, Q, allow):
    """(ids, dist, ndist, nhops, stage) of the filtered, the paged and the grouped call under one mask"""
    flt = hg.filter(allow)
    try:
        f = H.Ohnsw.knn_batch_filtered(hg, K, Q, flt, ef=EF, counters=True)
        a = H.Ohnsw.knn_batch_after(hg, K, Q, None, ef=EF, filter=flt, counters=True)
        g = H.Ohnsw.knn_batch_grouped(hg, K, Q, labels, ef=EF, filter=flt, counters=True)
    finally:
        flt.release()
    assert np.array_equal(g[2], np.where(g[0] >= 0, g[0] - hg.id_base, -1)), "a node is its own label"
    return {"filtered": f, "paged": (a[0], a[1]) + tuple(a[3:]), "grouped": (g[0], g[1]) + tuple(g[3:])}


def _pairs(ids, dist):
    """each row as its (distance, id) pairs, sorted: distances by their bits (no -0.0 here, NaN fills last)"""
    key = dist.view(np.uint32).astype(np.int64) << 32 | (ids.astype(np.int64) & 0xFFFFFFFF)
    return np.sort(key, axis=1)


def _sparse_calls(H, w):
    if "sparse" not in w.calls:
        w.calls["sparse"] = _three(H, w.hg, w.labels, w.Q, _sparse_mask())
    return w.calls["sparse"]


def test_same_stage_counters_and_rows_under_a_sparse_mask(H, world):
    got = _sparse_calls(H, world)
    f = got["filtered"]
    stages = set(int(s) for s in f[4])
    print("stages: %s" % dict(zip(*np.unique(f[4], return_counts=True))))
    assert 0 in stages and EXACT in stages and any(0 < s < EXACT for s in stages), stages
    assert (f[0] >= world.hg.id_base).all(), "more than k nodes are allowed: every row is full"
    for name in ("paged", "grouped"):
        o = got[name]
        np.testing.assert_array_equal(o[4], f[4], err_msg="%s out_stage" % name)
        np.testing.assert_array_equal(o[2], f[2], err_msg="%s out_ndist" % name)
        np.testing.assert_array_equal(o[3], f[3], err_msg="%s out_nhops" % name)
        np.testing.assert_array_equal(_pairs(o[0], o[1]), _pairs(f[0], f[1]), err_msg="%s rows" % name)


def test_nobody_walks_when_fewer_than_k_are_allowed(H, world):
    allow = np.zeros(N, bool)
    allow[[3, 777, 1500, 2222, 2223, 3100, 3999]] = True
    assert allow.sum() < K
    for name, o in _three(H, world.hg, world.labels, world.Q, allow).items():
        assert (o[3] == 0).all(), "%s out_nhops" % name
        assert (o[2] == allow.sum()).all(), "%s out_ndist" % name
        assert (o[4] == EXACT).all(), "%s out_stage" % name
        want = np.concatenate([np.flatnonzero(allow) + world.hg.id_base, np.full(K - allow.sum(), -1)])
        np.testing.assert_array_equal(np.sort(o[0], axis=1), np.broadcast_to(np.sort(want), o[0].shape), err_msg="%s ids" % name)


def test_half_rows_give_each_call_its_float32_rows_and_stages(H, world):
    w = world
    w.hg.export()               # the twin: the same vectors under the same graph
    hg = H.Hgraph(w.X, w.hg.deg0, w.hg.nbr0, w.hg.upper, entry_point=w.hg.entry_point, id_base=w.hg.id_base, max_degree=w.hg.max_degree)
    hg.set_option("half_rows", 1)
    assert hg.info().row_format == ROWS_HALF
    labels = hg.labels(np.arange(N, dtype=np.int32), N)
    try:
        got = _three(H, hg, labels, w.Q, _sparse_mask())
    finally:
        labels.release()
        hg.release()
    for name, want in _sparse_calls(H, w).items():
        o = got[name]
        np.testing.assert_array_equal(o[0], want[0], err_msg="%s ids" % name)
        np.testing.assert_array_equal(o[1].view(np.uint32), want[1].view(np.uint32), err_msg="%s distances" % name)
        np.testing.assert_array_equal(o[4], want[4], err_msg="%s out_stage" % name)
