"""The sharded index (ocaml-hnsw_amd/csrc/hnsw_sharded.hip) against the header's definition, which is in terms of public calls: a
shard is hnsw_build of its slice, a sharded row is the merge of the rows hnsw_search_batch / hnsw_brute_force_batch give on the
borrowed shard handles.  The merge reference is numpy everywhere: np.lexsort((global id, distance)) over the real entries, compared
bit for bit.  Device 0 is listed several times, so one GPU is enough."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, NQ, M, EFC, SEED = 5003, 24, 70, 8, 40, 11
N_IP, D_IP = 3001, 100
EF, K = 32, 10


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, ctx=""):
    assert len(got) == len(want), ctx
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.asarray(a).dtype == np.asarray(b).dtype, "%s [%d] dtype" % (ctx, i)
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="%s [%d]" % (ctx, i))


def np_merge(ids, dist, first_row, k_out, id_base, fill):
    """the definition: per query the first k_out real entries of all lists under (distance, first_row[list] + id), then the fill"""
    ids, dist = np.asarray(ids), np.asarray(dist)
    n_lists, nq, _ = ids.shape
    gid_all = np.asarray(first_row, np.int64)[:, None, None] + ids.astype(np.int64)
    out_i = np.full((nq, k_out), -1, np.int64)
    out_d = np.full((nq, k_out), np.nan if fill == 0 else np.inf, np.float32)
    for q in range(nq):
        real = ids[:, q, :] >= id_base
        gid, dd = gid_all[:, q, :][real], dist[:, q, :][real]
        order = np.lexsort((gid, dd))[:k_out]
        out_i[q, :len(order)] = gid[order]
        out_d[q, :len(order)] = dd[order]
    return out_i, out_d


def _shard_rows(H, s, Q, ef, k, fill, sem):
    """hnsw_search_batch on every borrowed shard handle -> (ids [G][nq][k], dist, first_row [G], ndist summed, nhops summed)"""
    ids, dist, first, nd, nh = [], [], [], 0, 0
    for g in range(s.num_shards()):
        hg, lo = s.shard(g)
        i, d, a, b = H._search(hg, Q, ef, k, fill, counters=True, sem=sem)
        ids.append(i); dist.append(d); first.append(lo)
        nd, nh = nd + a, nh + b                                 # (uint32 arrays: the sum wraps as the kernel's does)
    return np.stack(ids), np.stack(dist), first, nd, nh


def _check_search(H, s, Q, ef, k, fill=0, sem=0, ctx=""):
    got = s.knn_batch(Q, ef, k, fill=fill, sem=sem, counters=True)
    ids, dist, first, nd, nh = _shard_rows(H, s, Q, ef, k, fill, sem)
    want = np_merge(ids, dist, first, k, s.id_base, fill)
    _same(got, want + (nd, nh), ctx)
    return got


class World:
    pass


@pytest.fixture(scope="module")
def world(H):
    w = World()
    rng = np.random.default_rng(5)
    w.X = rng.normal(size=(N, D)).astype(np.float32)
    w.Q = rng.normal(size=(NQ, D)).astype(np.float32)
    Xi = rng.normal(size=(N_IP, D_IP)).astype(np.float32)
    w.X_ip = (Xi / np.linalg.norm(Xi, axis=1, keepdims=True)).astype(np.float32)          # unit rows
    w.Q_ip = rng.normal(size=(NQ, D_IP)).astype(np.float32)
    cache = {}

    def sharded(G, metric=0):
        if (G, metric) not in cache:
            X = w.X if metric == 0 else w.X_ip
            cache[(G, metric)] = H.ShardedHgraph.build(X, M, EFC, [0] * G, seed=SEED, metric=metric)
        return cache[(G, metric)]

    w.sharded = sharded
    yield w
    for s in cache.values():
        s.release()


# ---- 1. the merge operator alone ------------------------------------------------------------------------------------------------

def _lists(rng, n_lists, nq, k_in, id_base):
    """lists with few distinct distances (negative ones too), ragged, some all padding; padding carries junk below id_base"""
    values = np.array([-2.5, -1.0, -0.125, 0.0, 0.5, 0.5000001, 3.0, 1e30], np.float32)
    dist = np.sort(rng.choice(values, size=(n_lists, nq, k_in)), axis=-1)
    ids = (np.cumsum(rng.integers(1, 4, size=(n_lists, nq, k_in)), axis=-1) - 1 + id_base).astype(np.int32)   # ascending, distinct
    kind = rng.integers(0, 4, size=(n_lists, nq))               # 0: all padding, 1: full, else ragged
    cnt = np.where(kind == 0, 0, np.where(kind == 1, k_in, rng.integers(0, k_in + 1, size=(n_lists, nq))))
    pad = np.arange(k_in)[None, None, :] >= cnt[:, :, None]
    ids[pad] = rng.choice(np.array([id_base - 1, -7, -2 ** 31], np.int32), size=int(pad.sum()))
    dist[pad] = rng.choice(np.array([np.nan, -np.inf, 0.0], np.float32), size=int(pad.sum()))
    # lists far apart, the upper half beyond 2^33: global ids need their 64 bits
    first = np.arange(n_lists, dtype=np.int64) * 5000 + np.where(np.arange(n_lists) >= (n_lists + 1) // 2, 2 ** 33, 0)
    return ids, dist, first


@pytest.mark.parametrize("nq", [70, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 10, 10), (3, 7, 10), (64, 16, 1024), (64, 1024, 1024), (5, 33, 20)])
def test_merge_operator(H, shape, nq):
    n_lists, k_in, k_out = shape
    rng = np.random.default_rng(1000 * n_lists + k_in + nq)
    for fill, id_base in ((H.FILL_OHNSW, 0), (H.FILL_BA, 1)):
        ids, dist, first = _lists(rng, n_lists, nq, k_in, id_base)
        want = np_merge(ids, dist, first, k_out, id_base, fill)
        got = H.merge_lists(ids, dist, first, k_out, id_base=id_base, fill=fill)
        _same(got, want, "merge %s nq %d fill %d" % (shape, nq, fill))
    if shape == (3, 7, 10) and nq == 70:
        assert (want[0][:, -1] < 0).any() and (want[0][:, -1] >= 0).any()     # the real entries run out for some queries only


def test_merge_operator_equal_distances_across_and_inside_lists(H):
    # every distance equal: the order is the global ids', whatever list they come from; first_row may repeat
    ids = np.array([[[0, 2, 4]], [[1, 3, 5]], [[0, 1, -1]]], np.int32)
    dist = np.full(ids.shape, -1.5, np.float32)
    got = H.merge_lists(ids, dist, [0, 0, 6], 9, fill=H.FILL_BA)
    np.testing.assert_array_equal(got[0], [[0, 1, 2, 3, 4, 5, 6, 7, -1]])
    got = H.merge_lists(ids, dist, [0, 2 ** 33, 2 ** 33 + 6], 9, fill=H.FILL_BA)          # global ids beyond 32 bits
    np.testing.assert_array_equal(got[0], [[0, 2, 4, 2 ** 33 + 1, 2 ** 33 + 3, 2 ** 33 + 5, 2 ** 33 + 6, 2 ** 33 + 7, -1]])
    np.testing.assert_array_equal(got[1], np.array([[-1.5] * 8 + [np.inf]], np.float32))


# ---- 2. build ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2, 3, 5])
def test_build_is_hnsw_build_of_each_slice(H, world, G):
    s = world.sharded(G)
    assert s.num_shards() == G
    total_bytes = 0
    for g in range(G):
        lo, hi = N * g // G, N * (g + 1) // G
        hg, first = s.shard(g)
        assert first == lo
        assert hg.info().n == hi - lo
        alone = H.Ohnsw.build_batch_bigarray(world.X[lo:hi], M, EFC, seed=SEED + g)
        a, b = hg.export(), alone.export()
        np.testing.assert_array_equal(a.deg0, b.deg0)
        np.testing.assert_array_equal(a.nbr0, b.nbr0)
        assert a.max_layer == b.max_layer and a.entry_point == b.entry_point
        total_bytes += hg.info().device_bytes
        alone.release()
    assert s.info() == (N, D, H.METRIC_L2, 0, total_bytes)


# ---- 3. search --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 3])
def test_search_is_the_merge_of_the_shards_rows(H, world, G):
    s = world.sharded(G)
    for sem, fill in ((H.SEM_OHNSW, H.FILL_OHNSW), (H.SEM_FUNCTOR, H.FILL_BA)):
        ids, dist, nd, nh = _check_search(H, s, world.Q, EF, K, fill, sem, "L2 G %d sem %d" % (G, sem))
        assert ids.dtype == np.int64 and (ids >= 0).all() and (ids < N).all() and (np.diff(dist, axis=1) >= 0).all()
        assert (nd > 0).all() and (nh > 0).all()


def test_search_inner_product(H, world):
    s = world.sharded(3, H.METRIC_IP)
    assert s.info()[:4] == (N_IP, D_IP, H.METRIC_IP, 0)
    for sem, fill in ((H.SEM_OHNSW, H.FILL_OHNSW), (H.SEM_FUNCTOR, H.FILL_BA)):
        _check_search(H, s, world.Q_ip, EF, K, fill, sem, "IP sem %d" % sem)


def test_search_over_half_rows_with_refine(H, world):
    s = world.sharded(3)
    plain = s.knn_batch(world.Q, EF, K)
    try:
        s.set_option("half_rows", 1)
        s.set_option("refine", 16)
        for g in range(3):
            assert s.shard(g)[0].info().row_format == H.ROWS_HALF
        for sem, fill in ((H.SEM_OHNSW, H.FILL_OHNSW), (H.SEM_FUNCTOR, H.FILL_BA)):
            _check_search(H, s, world.Q, EF, K, fill, sem, "half rows sem %d" % sem)
    finally:
        s.set_option("half_rows", 0)
        s.set_option("refine", 0)
    _same(s.knn_batch(world.Q, EF, K), plain, "options off again")


def test_set_option_is_all_or_nothing(H, world):
    s = world.sharded(3)
    L = H.load()
    hg1 = s.shard(1)[0]
    # shard 1 searches its sq8 rows, so it alone refuses half_rows: shard 0, which accepted, is set back
    hg1.set_option("sq8_rows", 1)
    try:
        with pytest.raises(H.InvalidArgument, match="sq8_rows"):
            s.set_option("half_rows", 1)
        assert [s.shard(g)[0].info().row_format for g in range(3)] == [H.ROWS_F32, H.ROWS_SQ8, H.ROWS_F32]
    finally:
        hg1.set_option("sq8_rows", -1)
    with pytest.raises(H.InvalidArgument):
        s.set_option("no_such_option", 1)
    assert L.hnsw_sharded_set_option(s.handle, None, 1) == H.ERR_BAD_ARG


# ---- 4. ties across shards ----------------------------------------------------------------------------------------------------------

def test_ties_across_shards(H):
    rng = np.random.default_rng(7)
    X = rng.integers(0, 4, size=(600, 8)).astype(np.float32)    # integer grid: equal distances everywhere; squared sums <= 72
    Q = rng.integers(0, 4, size=(NQ, 8)).astype(np.float32)
    s = H.ShardedHgraph.build(X, M, EFC, [0] * 4, seed=SEED)
    flat = H.Hgraph.flat(X)
    try:
        ids, dist, _, _ = _check_search(H, s, Q, 64, 20, ctx="grid")
        assert (np.diff(dist, axis=1) == 0).mean() > 0.3        # the rows are full of equal distances
        for q in range(NQ):                                     # ... ordered by global id inside each run
            for j in range(19):
                assert dist[q, j] < dist[q, j + 1] or ids[q, j] < ids[q, j + 1]
        bi, bd = s.brute_force_knn(20, Q)
        fi, fd = H.Ohnsw.brute_force_knn(flat, 20, Q)
        _same((bi, bd), (fi.astype(np.int64), fd), "grid brute force")
    finally:
        s.release()
        flat.release()


# ---- 5. brute force on float data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1])
def test_brute_force_matches_the_unsharded_scan(H, world, metric):
    X, Q = (world.X, world.Q) if metric == 0 else (world.X_ip, world.Q_ip)
    s = world.sharded(3, metric)
    flat = H.Hgraph.flat(X, metric=metric)
    try:
        for fill in (H.FILL_OHNSW, H.FILL_BA):
            bi, bd = s.brute_force_knn(K, Q, fill=fill)
            fi, fd = H.Ohnsw.brute_force_knn(flat, K + 1, Q, fill=fill)
            assert bi.dtype == np.int64
            np.testing.assert_array_equal(_bits(bd), _bits(fd[:, :K]))          # distances: every query, bit for bit
            distinct = (np.diff(fd, axis=1) > 0).all(axis=1)                    # the 11 nearest reference distances pairwise distinct
            print("metric %d fill %d: %d of %d queries have 11 distinct nearest distances" % (metric, fill, int(distinct.sum()), NQ))
            assert distinct.mean() >= 0.95
            np.testing.assert_array_equal(bi[distinct], fi[distinct, :K].astype(np.int64))
    finally:
        flat.release()


# ---- 6. small shards ----------------------------------------------------------------------------------------------------------------

def test_small_shards(H, world):
    L = H.load()
    X, Q = world.X[:23], world.Q
    s = H.ShardedHgraph.build(X, M, EFC, [0] * 3, seed=SEED)
    try:                                                        # k = 10 > n_g = 7, 8, 8: fills inside a shard's list
        ids, _, _, _ = _check_search(H, s, Q, 16, 10, ctx="n 23")
        assert (ids >= 0).all()                                 # ... and the merged row still has 10 real entries
        bi, bd = s.brute_force_knn(10, Q)
        flat = H.Hgraph.flat(X)
        fi, fd = H.Ohnsw.brute_force_knn(flat, 10, Q)
        flat.release()
        np.testing.assert_array_equal(_bits(bd), _bits(fd))
        p = H._SearchParams(16, 10, 0, H.SEM_FUNCTOR_NEAREST_K)  # "the k farthest of W" has no merged meaning
        out_i, out_d = np.zeros((NQ, 10), np.int64), np.zeros((NQ, 10), np.float32)
        assert L.hnsw_sharded_search_batch(s.handle, H._ptr(Q), NQ, D, ctypes.byref(p), H._ptr(out_i), H._ptr(out_d), None, None) == H.ERR_BAD_ARG
        p = H._SearchParams(8, 10, 0, 0)                        # k > ef
        assert L.hnsw_sharded_search_batch(s.handle, H._ptr(Q), NQ, D, ctypes.byref(p), H._ptr(out_i), H._ptr(out_d), None, None) == H.ERR_BAD_ARG
        p = H._SearchParams(16, 10, 0, 0)
        assert L.hnsw_sharded_search_batch(s.handle, None, 0, D, ctypes.byref(p), None, None, None, None) == H.OK      # nq == 0
        assert L.hnsw_sharded_search_batch(s.handle, None, 1, D, ctypes.byref(p), None, None, None, None) == H.ERR_BAD_ARG
    finally:
        s.release()
    s = H.ShardedHgraph.build(world.X[:5], M, EFC, [0] * 5, seed=SEED)
    try:                                                        # five shards of one row: 5 real entries, then the fill
        for fill in (H.FILL_OHNSW, H.FILL_BA):
            ids, dist, _, _ = _check_search(H, s, Q, 8, 8, fill=fill, sem=H.SEM_FUNCTOR, ctx="n 5")
            assert (np.sort(ids[:, :5], axis=1) == np.arange(5)).all() and (ids[:, 5:] == -1).all()
            assert (np.isnan(dist[:, 5:]) if fill == H.FILL_OHNSW else np.isposinf(dist[:, 5:])).all()
            bi, bd = s.brute_force_knn(8, Q, fill=fill)
            _same((bi, bd), (ids, dist), "n 5 brute force")
    finally:
        s.release()
    out = ctypes.c_void_p(1)
    pb = H._BuildParams(M, EFC, 0, 0, SEED, 0, 0, 0, 0)
    dev = (ctypes.c_int32 * 65)()
    for n, G in ((2, 3), (23, 0), (230, 65)):
        out.value = 1
        assert L.hnsw_sharded_build(H._ptr(world.X), n, D, D, ctypes.byref(pb), dev, G, ctypes.byref(out)) == H.ERR_BAD_ARG
        assert out.value is None


# ---- 7. shard handles: borrowed, read-only; save / load; create -----------------------------------------------------------------------

def test_shard_handles_are_read_only_but_searchable(H, world):
    L = H.load()
    s = world.sharded(3)
    hg, lo = s.shard(1)
    n1 = hg.info().n
    pb = H._BuildParams(M, EFC, 0, 0, SEED, 0, 0, 0, 0)
    one = np.array([3], np.int64)
    assert L.hnsw_index_insert(hg.handle, H._ptr(world.X), 1, D, ctypes.byref(pb)) == H.ERR_BAD_ARG
    assert L.hnsw_index_remove(hg.handle, H._ptr(one), 1, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_mark_deleted(hg.handle, H._ptr(one), 1) == H.ERR_BAD_ARG
    assert hg.info().n == n1 and hg.deleted_count() == 0
    allow = np.arange(n1) % 3 == 0
    fi, fd = H.Ohnsw.knn_batch_filtered(hg, K, world.Q, allow, ef=EF)
    assert (fi >= 0).all() and allow[fi].all() and (np.diff(fd, axis=1) >= 0).all()
    _, bd = H.Ohnsw.brute_force_knn(hg, K, world.Q)
    radius = float(bd[:, 4].mean())
    lims, ri, rd = H.Ohnsw.range_search(hg, radius, world.Q, ef=EF)
    assert lims[-1] == len(ri) > 0 and (rd <= radius).all() and (ri < n1).all()


def test_save_then_load(H, world, tmp_path):
    s = world.sharded(3)
    before = s.knn_batch(world.Q, EF, K, counters=True)
    paths = [str(tmp_path / ("shard%d.hnsw" % g)) for g in range(3)]
    s.save(paths)
    t = H.ShardedHgraph.load(paths, [0] * 3)
    try:
        assert t.info()[:4] == s.info()[:4] and [t.shard(g)[1] for g in range(3)] == [s.shard(g)[1] for g in range(3)]
        _same(t.knn_batch(world.Q, EF, K, counters=True), before, "loaded")
        hg = t.shard(2)[0]
        assert H.load().hnsw_index_mark_deleted(hg.handle, H._ptr(np.array([0], np.int64)), 1) == H.ERR_BAD_ARG
    finally:
        t.release()
    with pytest.raises((H.Failure, H.InvalidArgument)):
        H.ShardedHgraph.load([paths[0], str(tmp_path / "missing.hnsw")], [0, 0])


def test_create_adopts_graphs_of_unequal_size(H, world):
    bounds = [0, 700, 2801, N]
    parts = [H.Ohnsw.build_batch_bigarray(world.X[a:b], M, EFC, seed=3).export() for a, b in zip(bounds, bounds[1:])]
    s = H.ShardedHgraph.create(parts, [0] * 3)
    try:
        assert s.info()[:4] == (N, D, H.METRIC_L2, 0)
        assert [s.shard(g)[1] for g in range(3)] == bounds[:3]
        rows = [H._search(p, world.Q, EF, K, 0, counters=True) for p in parts]
        want = np_merge(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), bounds[:3], K, 0, 0)
        got = s.knn_batch(world.Q, EF, K, counters=True)
        _same(got, want + (sum(r[2] for r in rows), sum(r[3] for r in rows)), "created")
        other = H.Hgraph.flat(world.X_ip[:50])                  # another d: the shards must agree
        with pytest.raises(H.InvalidArgument, match="does not agree"):
            H.ShardedHgraph.create([parts[0], other], [0, 0])
    finally:
        s.release()
        for p in parts:
            p.release()


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------------

def test_a_row_depends_on_its_own_query_only(H, world):
    s = world.sharded(3)
    Q = world.Q
    whole = s.knn_batch(Q, EF, K, counters=True)
    a, b = s.knn_batch(Q[:33], EF, K, counters=True), s.knn_batch(Q[33:], EF, K, counters=True)
    _same([np.concatenate(p) for p in zip(a, b)], whole, "two calls")
    back = s.knn_batch(np.ascontiguousarray(Q[::-1]), EF, K, counters=True)
    _same([x[::-1] for x in back], whole, "reversed")
    bf = s.brute_force_knn(K, Q)
    _same([x[::-1] for x in s.brute_force_knn(K, np.ascontiguousarray(Q[::-1]))], bf, "brute force reversed")


def test_cpp_front_end_sharded(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_sharded")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sharded front-end ok" in out.stdout, out.stdout + out.stderr


# ---- 9. the device group's lifetime ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("released_first", ["sharded", "multi"])
def test_two_device_groups_side_by_side_and_released_in_either_order(H, released_first):
    """A sharded and a replicated handle on one device (three shards, two replicas: each a device group with streams, events and
    buffers of its own), called alternately: every round gives round one's bits -- the multi rows hnsw_search_batch's on the
    unsharded graph (7 queries over 2 replicas: the unequal-shard copies), the sharded rows the merge of the shards' own rows --
    and after either handle is released, once or twice, the other still does."""
    rng = np.random.default_rng(23)
    X = rng.random((300, 8), dtype=np.float32)
    Q = rng.random((7, 8), dtype=np.float32)
    ef, k = 16, 5
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=SEED).export()
    s = H.ShardedHgraph.build(X, M, EFC, [0, 0, 0], seed=SEED)
    m = H.MultiHgraph(hg, [0, 0])
    try:
        ids, dist, first_row, _, _ = _shard_rows(H, s, Q, ef, k, H.FILL_OHNSW, H.SEM_OHNSW)
        want = {"sharded": np_merge(ids, dist, first_row, k, s.id_base, H.FILL_OHNSW), "multi": H._search(hg, Q, ef, k, H.FILL_OHNSW)}
        call = {"sharded": lambda: s.knn_batch(Q, ef, k), "multi": lambda: m.knn_batch_bigarray(k, Q, ef=ef)}
        handle = {"sharded": s, "multi": m}
        round_one = {}
        for r in range(3):
            for name in ("sharded", "multi"):
                got = call[name]()
                _same(got, want[name], "%s round %d" % (name, r))
                _same(got, round_one.setdefault(name, got), "%s round %d against round one" % (name, r))
        survivor = "multi" if released_first == "sharded" else "sharded"
        for _ in range(2):                                      # (the second release finds nothing to do)
            handle[released_first].release()
            _same(call[survivor](), round_one[survivor], "%s after the other's release" % survivor)
        for _ in range(2):
            handle[survivor].release()
    finally:
        s.release()
        m.release()
        hg.release()
