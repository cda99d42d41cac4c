"""hnsw_index_insert (Ohnsw.insert, lib/ohnsw.ml:766-837, for m vectors into an index the library holds): the grown graph
equals the reference's sequential build link for link, and the batched build where the split falls on one of its batch
boundaries; everything the handle derived from its graph (byte / split rows, locality codes, the fallback slab, prepared
shapes) follows it; every refusal leaves the index exactly as it was."""
import os
import tempfile

import numpy as np
import pytest
from device_bytes import base_bytes, expected

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT = 0, 2, 3


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1
    return H


def _data(kind, n, d, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    if kind == "levels":
        return rng.integers(0, 4, size=(n, d)).astype(np.float32)
    if kind == "unit":
        X = rng.normal(size=(n, d))
        return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    centres = rng.integers(20, 200, size=(32, d))
    return np.clip(np.rint(centres[rng.integers(0, 32, n)] + rng.normal(0, 25, size=(n, d))), 0, 218).astype(np.float32)


def _space(oracle, X, metric):
    return (oracle.Space.ip if metric else oracle.Space.l2)(X, arith=oracle.TREE16)


def _same_graph(hg, want, base=0):
    """exported device graph == oracle graph (0-based) shifted by `base`: entry point, max layer, layer-0 rows in iteration
    order, upper-layer nodes / degrees / rows"""
    sh = lambda a: np.where(a >= 0, a + base, -1)
    assert hg.entry_point == want.entry_point + base
    assert hg.max_layer == want.max_layer
    np.testing.assert_array_equal(hg.deg0, want.deg0)
    np.testing.assert_array_equal(hg.nbr0, sh(want.nbr0))
    assert len(hg.upper) == len(want.upper)
    for (nodes, deg, nbr), (wn, wd, wb) in zip(hg.upper, want.upper):
        np.testing.assert_array_equal(nodes, wn + base)
        np.testing.assert_array_equal(deg, wd)
        np.testing.assert_array_equal(nbr, sh(wb))


def _same_export(a, b):
    assert (a.entry_point, a.max_layer, a.n) == (b.entry_point, b.max_layer, b.n)
    np.testing.assert_array_equal(a.deg0, b.deg0)
    np.testing.assert_array_equal(a.nbr0, b.nbr0)
    for (n1, d1, r1), (n2, d2, r2) in zip(a.upper, b.upper):
        np.testing.assert_array_equal(n1, n2)
        np.testing.assert_array_equal(d1, d2)
        np.testing.assert_array_equal(r1, r2)


def _invariants(hg, M):
    """Graph.Test.invariant (lib/ohnsw.ml:217-225) and the degree caps: symmetric links, no self links, no duplicates"""
    n = hg.n
    assert hg.deg0.max(initial=0) <= 2 * M
    sets = []
    for i in range(n):
        row = hg.nbr0[i, :hg.deg0[i]].tolist()
        assert len(set(row)) == len(row) and i + hg.id_base not in row, i
        sets.append(set(row))
    assert all(i + hg.id_base in sets[j - hg.id_base] for i in range(n) for j in sets[i])
    for nodes, deg, nbr in hg.upper:
        assert deg.max(initial=0) <= M
        slot = {int(v): s for s, v in enumerate(nodes)}
        for s, v in enumerate(nodes):
            row = nbr[s, :deg[s]].tolist()
            assert len(set(row)) == len(row) and int(v) not in row
            for u in row:
                assert int(v) in nbr[slot[int(u)], :deg[slot[int(u)]]]


def _levels(hg):
    lvl = np.zeros(hg.n, np.int64)
    for l, (nodes, _, _) in enumerate(hg.upper):
        lvl[nodes - hg.id_base] = l + 1
    return lvl


def _boundaries(lvl, max_batch=8192, batch_div=16):
    """the batch ends of hnsw_build's schedule (a node that raises max_layer ends its batch)"""
    out, pos, cur = [], 1, 0
    while pos < len(lvl):
        end = min(len(lvl), pos + max(1, min(max_batch, pos // batch_div)))
        for j in range(pos, end):
            if lvl[j] > cur:
                end = j + 1
                break
        cur = max(cur, int(lvl[end - 1]))
        out.append(end)
        pos = end
    return out


def _oracle_graph(oracle, hg):
    return oracle.Graph(hg.n, hg.entry_point - hg.id_base, hg.deg0,
                        np.where(hg.nbr0 >= 0, hg.nbr0 - hg.id_base, -1),
                        [(nodes - hg.id_base, deg, np.where(nbr >= 0, nbr - hg.id_base, -1)) for nodes, deg, nbr in hg.upper])


def _search_bits(H, hg, Q, k, ef):
    ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
    return ids, dist.view(np.uint32), nh, H.Ba.knn_batch(hg, Q, ef, k).view(np.uint32)


def _check_search(H, oracle, hg, X, metric, Q, efs=(64, 200, 512), k=10):
    """Ohnsw.knn_batch_bigarray (ids, distance bits, hops) and Hnsw.Ba.knn_batch against the oracle on the exported graph"""
    hg.export()
    g = _oracle_graph(oracle, hg)
    sp = _space(oracle, X, metric)
    for ef in efs:
        ids, dist, nh, fd = _search_bits(H, hg, Q, k, ef)
        oi, od, ond, onh = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=k, ef=ef, ties=oracle.TIES_CANONICAL, counters=True)
        np.testing.assert_array_equal(ids, oi, err_msg="ef %d" % ef)
        np.testing.assert_array_equal(dist, od.view(np.uint32), err_msg="ef %d" % ef)
        np.testing.assert_array_equal(nh, onh, err_msg="ef %d" % ef)
        ofd = oracle.Functor.knn_batch(g, sp, Q, ef, k, ties=oracle.TIES_CANONICAL)
        np.testing.assert_array_equal(fd, ofd.view(np.uint32), err_msg="ef %d" % ef)
    return g, sp


# ---- link-for-link identities ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,metric,n,d,M,efc", [
    ("uniform", 0, 3000, 16, 6, 40),
    ("levels", 0, 2500, 6, 8, 60),
    ("unit", 1, 3000, 24, 8, 50),
    ("sift", 0, 2000, 128, 16, 100),
    ("sift", 0, 2500, 32, 32, 80),
    ("levels", 0, 2500, 6, 32, 80),
])
def test_sequential_inserts_equal_the_reference_insert_link_for_link(H, oracle, kind, metric, n, d, M, efc):
    """build(X[:n1]) then inserts of one vector, of X[n1+1:n2] and of X[n2:], all max_batch = 1: Ohnsw.insert node by node,
    so the result is the oracle's sequential build of all of X however the inserts were split"""
    X = _data(kind, n, d)
    want = oracle.build_ohnsw(_space(oracle, X, metric), M, efc, seed=5, ties=oracle.TIES_CANONICAL)
    n1, n2 = n // 3, (2 * n) // 3
    hg = H.Ohnsw.build_batch_bigarray(X[:n1], M, efc, seed=5, metric=metric, max_batch=1)
    for a, b in ((n1, n1 + 1), (n1 + 1, n2), (n2, n)):
        ids = H.Ohnsw.insert_batch(hg, X[a:b], M, efc, seed=5, max_batch=1)
        np.testing.assert_array_equal(ids, np.arange(a, b, dtype=np.int64))
        assert ids.dtype == np.int64
        assert hg.n == b and hg.deg0 is None and hg.nbr0 is None and hg.upper is None
    assert hg.vectors.shape == (n, d)
    np.testing.assert_array_equal(hg.vectors, X)
    _same_graph(hg.export(), want)


def test_insert_into_a_graph_the_library_did_not_build(H, oracle):
    """hnsw_index_create from the oracle's sequential build of a prefix (id_base 1, rows sliced to their longest list as the
    OCaml flatten does: narrower than 2M / M, so the widening path runs), then the rest inserted one by one: the oracle's
    sequential build of the whole set"""
    X = _data("uniform", 1500, 16, seed=3)
    M, efc, n1 = 8, 40, 12
    sp = _space(oracle, X, 0)
    pre = oracle.build_ohnsw(sp, M, efc, seed=5, ties=oracle.TIES_CANONICAL, n=n1)
    w0 = int(pre.deg0.max())
    assert w0 < 2 * M
    upper = []
    wu = max([int(deg.max(initial=1)) for _, deg, _ in pre.upper] + [1])
    for nodes, deg, nbr in pre.upper:
        upper.append((nodes + 1, deg, np.where(nbr[:, :wu] >= 0, nbr[:, :wu] + 1, -1)))
    hg = H.Hgraph(X[:n1], pre.deg0, np.where(pre.nbr0[:, :w0] >= 0, pre.nbr0[:, :w0] + 1, -1), upper,
                  entry_point=pre.entry_point + 1, id_base=1, max_degree=wu)
    assert hg.info().max_degree0 == w0
    ids = H.Ohnsw.insert_batch(hg, X[n1:], M, efc, seed=5, max_batch=1)
    np.testing.assert_array_equal(ids, np.arange(n1 + 1, 1500 + 1))
    inf = hg.info()
    assert (inf.n, inf.max_degree0, inf.max_degree) == (1500, 2 * M, M)
    assert (hg.max_degree0, hg.max_degree) == (2 * M, M)
    want = oracle.build_ohnsw(sp, M, efc, seed=5, ties=oracle.TIES_CANONICAL)
    _same_graph(hg.export(), want, base=1)


def test_batched_insert_at_a_batch_boundary_equals_the_batched_build(H, oracle):
    """build(X[:n1]) + insert(X[n1:]) == build(X) with default batching when n1 is a batch boundary of build(X)'s schedule;
    an empty index grown by one insert of X == build(X); off a boundary the graph keeps the reference's invariants"""
    M, efc, n, d = 8, 40, 20000, 16
    X = _data("uniform", n, d, seed=4)
    full = H.Ohnsw.build_batch_bigarray(X, M, efc, seed=9).export()
    bounds = _boundaries(_levels(full))
    n1 = next(b for b in bounds if b >= n // 2)
    assert n1 < n
    grown = H.Ohnsw.build_batch_bigarray(X[:n1], M, efc, seed=9)
    H.Ohnsw.insert_batch(grown, X[n1:], M, efc, seed=9)
    _same_export(grown.export(), full)
    empty = H.Hgraph(np.zeros((0, d), np.float32), np.zeros(0, np.int32), np.zeros((0, 2 * M), np.int32))
    H.Ohnsw.insert_batch(empty, X, M, efc, seed=9)
    _same_export(empty.export(), full)
    off = H.Ohnsw.build_batch_bigarray(X[:n1 + 37], M, efc, seed=9)
    H.Ohnsw.insert_batch(off, X[n1 + 37:n1 + 2000], M, efc, seed=9)
    H.Ohnsw.insert_batch(off, X[n1 + 2000:], M, efc, seed=9, max_batch=300)
    off.export()
    assert off.n == n
    _invariants(off, M)


# ---- searches on grown indices -----------------------------------------------------------------------------------------

def _queries(X, nq, seed, jitter=True):
    rng = np.random.default_rng(seed)
    Q = X[rng.integers(0, len(X), nq)].copy()
    if jitter:
        Q += rng.integers(0, 2, size=Q.shape).astype(np.float32)
    return Q


@pytest.mark.parametrize("case", ["l2", "ip", "bytes", "bytes_then_float", "split", "split_freed"])
def test_search_on_a_grown_index_matches_the_oracle(H, oracle, case):
    metric = 1 if case == "ip" else 0
    if case == "ip":
        X, M = _data("unit", 4000, 24), 8
    elif case.startswith("bytes"):
        X, M = _data("sift", 4000, 128), 16
        if case == "bytes_then_float":
            X[3000:] += np.float32(0.5)
    elif case.startswith("split"):
        X, M = _data("uniform", 4000, 100), 12
    else:
        X, M = _data("uniform", 4000, 32), 8
    hg = H.Ohnsw.build_batch_bigarray(X[:3000], M, 60, seed=1, metric=metric)
    fmt0 = hg.info().row_format
    if case.startswith("bytes"):
        assert fmt0 == ROWS_BYTES
    if case.startswith("split"):
        assert fmt0 == ROWS_SPLIT
    if case == "split_freed":
        bytes0 = hg.info().device_bytes
        hg.set_option("split_rows", -1)
        assert hg.info().device_bytes < bytes0 and hg.info().row_format == ROWS_F32
        assert hg.info().device_bytes == base_bytes(hg.export())
    assert hg.info().device_bytes == expected(hg.export(), X.shape[1])
    H.Ohnsw.insert_batch(hg, X[3000:3400], M, 60, seed=1)
    assert hg.info().device_bytes == expected(hg.export(), X.shape[1])          # the grown tables and row copies, exactly
    H.Ohnsw.insert_batch(hg, X[3400:], M, 60, seed=1)
    assert hg.info().device_bytes == expected(hg.export(), X.shape[1])
    inf = hg.info()
    assert inf.n == 4000 and hg.n == 4000
    want_fmt = {"bytes": ROWS_BYTES, "bytes_then_float": ROWS_F32, "split": ROWS_SPLIT, "split_freed": ROWS_F32}.get(case, ROWS_F32)
    assert inf.row_format == want_fmt
    assert hg.row_bytes() == (128 if want_fmt == ROWS_BYTES else 4 * X.shape[1])
    Q = X[np.random.default_rng(2).integers(0, 4000, 150)] if metric else _queries(X, 150, 2, jitter=case != "bytes_then_float")
    _check_search(H, oracle, hg, X, metric, Q)
    if case == "split":
        # the grown split rows against the plain float32 rows: same bits
        a = _search_bits(H, hg, Q, 10, 128)
        hg.set_option("split_rows", 0)
        assert hg.info().row_format == ROWS_F32
        b = _search_bits(H, hg, Q, 10, 128)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
        H.Ohnsw.insert_batch(hg, _data("uniform", 50, 100, seed=8), M, 60, seed=1)      # split_rows 0 keeps its effect
        assert hg.info().row_format == ROWS_F32


def test_grown_index_derived_state(H, oracle):
    """visited_blocks 1 with the per-slot codes materialised by a search BEFORE the insert, byte_rows 0 and the device
    fallback slab set before it; afterwards: codes a permutation, stats == export, save -> load same bits, layer operators on
    the upper layers == oracle, prepared shapes still prepared"""
    import torch
    X = _data("sift", 6000, 64, seed=5)
    M = 8
    hg = H.Ohnsw.build_batch_bigarray(X[:4000], M, 60, seed=3, expected_ef=200)
    hg.set_option("visited_blocks", 1)
    hg.set_option("byte_rows", 0)
    Q = _queries(X, 100, 6)
    H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=200)
    assert hg.visited_blocks(200) > 0
    hg.set_option("device_fallback_slab_bytes", 4 * 4000 * 3)                # three queries of the old n, two of the new
    H.Ohnsw.insert_batch(hg, X[4000:], M, 60, seed=3)
    assert hg.info().row_format == ROWS_F32 and hg.row_bytes() == 4 * 64     # byte_rows 0 kept its effect
    assert hg.visited_blocks(200) > 0
    g, sp = _check_search(H, oracle, hg, X, 0, Q, efs=(200, 512))
    codes = hg.locality_codes()
    assert sorted(codes.tolist()) == list(range(6000))
    np.testing.assert_array_equal(codes[4000:], np.arange(4000, 6000))
    # the device entry point with its fallback slab
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    ids = torch.empty((100, 10), dtype=torch.int32, device=dev)
    dd = torch.empty((100, 10), dtype=torch.float32, device=dev)
    st = torch.zeros(100, dtype=torch.int32, device=dev)
    H.search_batch_device(hg, Qd.data_ptr(), 100, 64, 200, 10, ids.data_ptr(), dd.data_ptr(), 0, 0, st.data_ptr(), 0)
    torch.cuda.synchronize()
    oi, od = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=10, ef=200, ties=oracle.TIES_CANONICAL)
    assert ((st.cpu().numpy() & 1) == 0).all()
    np.testing.assert_array_equal(ids.cpu().numpy(), oi)
    np.testing.assert_array_equal(dd.cpu().numpy().view(np.uint32), od.view(np.uint32))
    # a slab that holds no query of the grown index refuses the insert
    hg.set_option("device_fallback_slab_bytes", 4 * 6000)
    with pytest.raises(H.InvalidArgument, match="holds no query"):
        H.Ohnsw.insert_batch(hg, X[:1], M, 60, seed=3)
    hg.set_option("device_fallback_slab_bytes", 0)
    # Hgraph.Stats against the export
    st_ = hg.stats()
    assert st_["num_nodes"] == 6000
    assert st_["layer_sizes"][0] == 6000
    for l, (nodes, deg, nbr) in enumerate(hg.upper):
        assert st_["layer_sizes"][l + 1] == len(nodes)
        c = st_["layer_connectivity"][l + 1]
        assert (c["min"], c["max"]) == (int(deg.min()), int(deg.max()))
    c0 = st_["layer_connectivity"][0]
    assert (c0["min"], c0["max"]) == (int(hg.deg0.min()), int(hg.deg0.max()))
    assert c0["mean"] == hg.deg0.sum() / 6000
    # save -> load: same graph, same bits
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "grown.hnsw")
        hg.save(path)
        again = H.Hgraph.load(path)
    _same_export(again.export(), hg)
    for u, v in zip(_search_bits(H, hg, Q, 10, 128), _search_bits(H, again, Q, 10, 128)):
        np.testing.assert_array_equal(u, v)
    # layer operators on the upper layers
    rng = np.random.default_rng(9)
    for layer in range(1, g.max_layer + 1):
        nodes = g.upper[layer - 1][0]
        T = _queries(X, 16, 10 + layer)
        starts = [rng.choice(nodes, size=min(3, len(nodes)), replace=False).tolist() for _ in range(16)]
        got = H.Ohnsw.search_k(hg, layer, starts, T, 5, ef=16)
        start1 = rng.choice(nodes, size=16)
        one = H.Ohnsw.search_one(hg, layer, start1, T)
        for j in range(16):
            want = oracle.Ohnsw.search_k(g, sp, starts[j], T[j], 16, layer=layer, ties=oracle.TIES_CANONICAL)
            assert [n for n, _ in got[j]] == [n for n, _ in want[:5]], (layer, j)
            assert int(one[j]) == oracle.Ohnsw.search_one(g, sp, int(start1[j]), T[j], layer=layer), (layer, j)


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_index_untouched(H):
    import ctypes
    X = _data("uniform", 2000, 16, seed=12)
    M = 8
    hg = H.Ohnsw.build_batch_bigarray(X[:1500], M, 40, seed=2).export()
    Q = _queries(X, 50, 13)
    before = (hg.info().n, hg.info().entry_point, hg.info().max_layer, hg.info().device_bytes, hg.info().max_degree0)
    bits = _search_bits(H, hg, Q, 10, 64)
    snap = H.Hgraph.__new__(H.Hgraph)
    snap.deg0, snap.nbr0, snap.upper = hg.deg0.copy(), hg.nbr0.copy(), [tuple(a.copy() for a in u) for u in hg.upper]
    snap.n, snap.entry_point, snap.max_layer = hg.n, hg.entry_point, hg.max_layer
    L = H.load()
    B = X[1500:]

    def raw(p, stride=16, m=len(B)):
        return L.hnsw_index_insert(hg.handle, B.ctypes.data_as(ctypes.c_void_p), m, stride, ctypes.byref(p))

    def params(**kw):
        a = dict(num_connections=M, num_nodes_search_construction=40, metric=0, id_base=0, seed=2, max_batch=0, batch_div=0,
                 expected_ef=0, expected_semantics=0)
        a.update(kw)
        return H._BuildParams(*a.values())

    cases = [(params(metric=1), H.ERR_BAD_ARG, "metric"), (params(id_base=1), H.ERR_BAD_ARG, "id_base"),
             (params(num_connections=4), H.ERR_BAD_ARG, "max_degree0=16"),
             (params(num_nodes_search_construction=513), H.ERR_UNSUPPORTED, "513"), (params(), H.ERR_BAD_ARG, "row_stride")]
    for i, (p, code, msg) in enumerate(cases):
        rc = raw(p, stride=15) if msg == "row_stride" else raw(p)
        assert rc == code, (i, rc)
        assert msg in L.hnsw_last_error().decode(), (i, L.hnsw_last_error())
    # a pending submit
    req = H.submit(hg, Q, 64, 10)
    assert raw(params()) == H.ERR_BAD_ARG and "submitted" in L.hnsw_last_error().decode()
    req.wait()
    # every refusal: same graph, same info, same bits
    hg.export()
    _same_export(hg, snap)
    assert (hg.info().n, hg.info().entry_point, hg.info().max_layer, hg.info().device_bytes, hg.info().max_degree0) == before
    for u, v in zip(_search_bits(H, hg, Q, 10, 64), bits):
        np.testing.assert_array_equal(u, v)
    # a replica of an hnsw_multi
    multi = H.MultiHgraph(hg, [0])
    rep = ctypes.c_void_p()
    assert L.hnsw_multi_replica(multi._h, 0, ctypes.byref(rep)) == H.OK
    assert L.hnsw_index_insert(rep, B.ctypes.data_as(ctypes.c_void_p), len(B), 16, ctypes.byref(params())) == H.ERR_BAD_ARG
    assert "replica" in L.hnsw_last_error().decode()
    ids, dist = multi.knn_batch_bigarray(10, Q, ef=64)
    np.testing.assert_array_equal(ids, bits[0])
    multi.release()
    # m == 0 is a no-op; the index still grows afterwards
    assert raw(params(), m=0) == H.OK and hg.info().n == 1500
    H.Ohnsw.insert_batch(hg, B, M, 40, seed=2)
    assert hg.info().n == 2000
