"""Search by stored item (ocaml-hnsw_amd/csrc/hnsw_by_id.hip): hnsw_index_get_rows_device, hnsw_search_batch_by_id / _by_key,
hnsw_brute_force_batch_by_id and hnsw_knn_graph against the ONE definition the header gives -- the public host call over the gathered
rows, and for exclude_self = 1 that call k + 1 wide with position p deleted, restated in numpy below -- on the world of
tests/test_gpu_range.py (2003 x 20 Gaussian vectors, the oracle's graph with M 8, efC 40, seed 1; ef 16, k 10).

Every comparison is exact: ids (keys) equal element for element, distances and counters compared as bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, EF, K = 2003, 20, 16, 10
M, EFC = 8, 40
I64 = np.iinfo(np.int64)
MISSING = -(2 ** 62) - 12345            # no stored key: see nasty_keys
UNSUPPORTED = -7


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def nasty_keys(n, seed=7):
    """n distinct int64 keys in a shuffled order (tests/test_gpu_keys.py): the extremes, -1, 0, pairs that differ only in bit 32 and
    above and pairs that differ only in the low word first, random ones behind"""
    x, y = 0x0000123400005678, -0x0000432100008765
    special = [I64.min, I64.max, -1, 0, 1, x, x + 2 ** 32, x + 2 ** 33, x + 2 ** 63 - 2 ** 62, y, y - 2 ** 32, y + 2 ** 32,
               x + 1, x + 2, y + 1, 2 ** 32, 2 ** 32 - 1, -2 ** 32, -2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31 - 1,
               2 ** 62, -2 ** 62, I64.min + 1, I64.max - 1]
    rng = np.random.default_rng(seed)
    rest = rng.integers(I64.min // 2, I64.max // 2, size=n + 64, dtype=np.int64).tolist()
    seen, out = set(), []
    for k in special + rest:
        if k not in seen and k != MISSING and I64.min <= k <= I64.max:
            seen.add(k)
            out.append(k)
        if len(out) == n:
            break
    out = np.array(out, dtype=np.int64)
    assert len(out) == n and len(np.unique(out)) == n
    return out[rng.permutation(n)]


def _translate(keys, ids, base=0, missing=MISSING):
    """the definition of hnsw_index_keys_of in numpy"""
    ids = np.asarray(ids, np.int64) - base
    ok = (ids >= 0) & (ids < len(keys))
    return np.where(ok, keys[np.where(ok, ids, 0)], missing).astype(np.int64)


def drop_self(R, self_ids, k):
    """THE DEFINITION of exclude_self = 1 over R = the public call's (ids [nq][k + 1], distances, counters...): per query p = the
    smallest j in [0, k] with R.ids[q][j] == ids[q], or k; the row with position p deleted -> ((ids, distances, counters...), p)"""
    ri, rd = R[0], R[1]
    nq = len(self_ids)
    assert ri.shape == (nq, k + 1) and rd.shape == (nq, k + 1)
    oi, od, ps = np.empty((nq, k), ri.dtype), np.empty((nq, k), np.float32), np.empty(nq, np.int64)
    for q in range(nq):
        hits = np.nonzero(ri[q] == self_ids[q])[0]
        p = int(hits[0]) if len(hits) else k
        keep = [j for j in range(k + 1) if j != p]
        oi[q], od[q], ps[q] = ri[q][keep], rd[q][keep], p
    return (oi, od) + tuple(R[2:]), ps


def _same(got, want, ctx=""):
    assert len(got) == len(want), ctx
    np.testing.assert_array_equal(got[0], want[0], err_msg=ctx + " ids")
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg=ctx + " distance bits")
    for a, b in zip(got[2:], want[2:]):
        np.testing.assert_array_equal(a, b, err_msg=ctx + " counters")


def _want(H, hg, ids, ef, k, fill, sem, exclude_self):
    """what the definition gives for the stored rows `ids` of hg, through the PUBLIC call over hg.rows(ids) -> (rows, p or None)"""
    Q = hg.rows(ids)
    if not exclude_self:
        return H._search(hg, Q, ef, k, fill, True, sem), None
    return drop_self(H._search(hg, Q, max(ef, k + 1), k + 1, fill, True, sem), ids, k)


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """the index of the issue; fresh(base, metric) uploads the same graph again as a handle of its own"""
    w = World()
    w.X = _floats(N, D, 1)
    w.space = oracle.Space.l2(w.X, arith=oracle.TREE16)
    w.g = oracle.build_ohnsw(w.space, M, EFC, seed=1)

    def fresh(base=0, metric=0):
        up = [(nodes + base, deg, np.where(nbr >= 0, nbr + base, -1)) for nodes, deg, nbr in w.g.upper]
        return H.Hgraph(w.X, w.g.deg0, np.where(w.g.nbr0 >= 0, w.g.nbr0 + base, -1), up, entry_point=w.g.entry_point + base, id_base=base,
                        max_degree=M, metric=metric)
    w.fresh = fresh
    rng = np.random.default_rng(11)
    some = rng.choice(N, size=64, replace=False)
    w.nodes = np.concatenate([some, [0, N - 1, some[5]]]).astype(np.int32)     # 64 random, the first, the last, one repeated
    w.hg = fresh()                      # never changed by a test
    w.keys = nasty_keys(N)
    w.keyed = fresh()
    w.keyed.set_keys(w.keys)
    yield w
    w.hg.release()
    w.keyed.release()


# ---- 1. the gather -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3, 4, 20, 33, 100, 1024])
def test_rows_device(H, d):
    import torch
    dev = torch.device("cuda", 0)
    n = 70
    X = _floats(n, d, d)
    sentinel = np.float32(-12345.5)
    for base in (0, 1):
        hg = H.Hgraph.flat(X, id_base=base)
        rng = np.random.default_rng(d + base)
        ids = np.concatenate([[base, base + n - 1, base + 7, base + 7], [0] if base else [base + 1],         # id_base 1: id 0 lies below the base
                              rng.integers(base, base + n, size=60)]).astype(np.int32)
        valid = (ids >= base) & (ids < base + n)
        assert valid.all() == (base == 0)
        want = np.zeros((len(ids), d), np.float32)
        want[valid] = hg.rows(ids[valid])
        d_ids = torch.from_numpy(ids).to(dev)
        for m in (1, 15, 16, 17, 64, 65):                                   # the group and wave edges
            for stride in (d, d + 3, (d + 3) // 4 * 4 + 4):                 # d, an odd stride (value by value), a multiple of 4
                out = torch.full((m, stride), float(sentinel), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                H.rows_device(hg, d_ids.data_ptr(), m, out.data_ptr(), stride)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                ctx = "d %d base %d m %d stride %d" % (d, base, m, stride)
                np.testing.assert_array_equal(_bits(got[:, :d]), _bits(want[:m]), err_msg=ctx)
                assert (got[:, d:] == sentinel).all(), ctx + ": written past d"
        H.rows_device(hg, 0, 0, 0, d)                                       # m == 0: a no-op, whatever the arrays
        with pytest.raises(H.InvalidArgument):
            H.rows_device(hg, d_ids.data_ptr(), 1, 0, d)
        if d > 1:
            with pytest.raises(H.InvalidArgument, match="out_stride"):
                H.rows_device(hg, d_ids.data_ptr(), 1, d_ids.data_ptr(), d - 1)
        hg.release()


# ---- 2. exclude_self = 0: the public call over the gathered rows -----------------------------------------------------------------

@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("sem", [0, 1])
def test_keep_self(H, world, base, sem):
    w = world
    hg = w.fresh(base) if base else w.hg
    ids = w.nodes + base
    fill = H.FILL_BA if sem else H.FILL_OHNSW
    want, _ = _want(H, hg, ids, EF, K, fill, sem, False)
    if sem:
        got = H.Ba.knn_batch_by_id(hg, ids, EF, K, exclude_self=False, counters=True)
    else:
        got = H.Ohnsw.knn_batch_by_id(hg, K, ids, ef=EF, exclude_self=False, counters=True)
    _same(got, want, "base %d rule %d" % (base, sem))
    assert (got[0][:, 0] == ids).mean() > 0.5                            # (a stored vector mostly finds itself first)
    if base:
        hg.release()


# ---- 3. exclude_self = 1 against the numpy statement of the definition -----------------------------------------------------------

@pytest.mark.parametrize("ef,k", [(10, 10), (16, 10), (1, 1), (128, 100), (1024, 1023)])
def test_drop_self(H, world, ef, k):
    w = world
    for base, sem in ((0, 0), (1, 1)):
        hg = w.fresh(base) if base else w.hg
        ids = w.nodes + base
        fill = H.FILL_BA if sem else H.FILL_OHNSW
        want, p = _want(H, hg, ids, ef, k, fill, sem, True)
        assert (p == 0).mean() > 0.5, "self is not at position 0 for most queries: the branch is not exercised"
        got = H._search_by_id(hg, ids, ef, k, fill, True, True, sem)
        _same(got, want, "ef %d k %d base %d" % (ef, k, base))
        assert not (got[0] == ids[:, None])[p < k].any()
        if base:
            hg.release()


def test_k_1024_is_unsupported(H, world):
    with pytest.raises(H.Failure, match=r"\[%d\].*1025" % UNSUPPORTED):
        H.Ohnsw.knn_batch_by_id(world.hg, 1024, world.nodes, ef=1024)
    with pytest.raises(H.Failure, match=r"\[%d\]" % UNSUPPORTED):
        H.Ohnsw.brute_force_by_id(world.hg, 1024, world.nodes)
    ids, _ = H.Ohnsw.knn_batch_by_id(world.hg, 1024, world.nodes[:3], ef=1024, exclude_self=False)       # without the extra entry k = 1024 stands
    assert ids.shape == (3, 1024)


# ---- 4. self not first, self absent ------------------------------------------------------------------------------------------------

def test_self_not_first_under_the_inner_product(H, world):
    w = world
    hg = w.fresh(0, H.METRIC_IP)
    # (under the inner product a short vector is not its own nearest: the 16 shortest join the queries)
    ids = np.concatenate([w.nodes, np.argsort((w.X.astype(np.float64) ** 2).sum(axis=1))[:16]]).astype(np.int32)
    want, p = _want(H, hg, ids, EF, K, H.FILL_OHNSW, 0, True)
    assert (want[0] != ids[:, None]).all()
    assert ((p > 0) & (p < K)).any(), "no query has self at a position other than 0: the branch is not exercised"
    assert (p == 0).any()
    print("inner product: self at position", np.bincount(p, minlength=K + 1).tolist())
    _same(H.Ohnsw.knn_batch_by_id(hg, K, ids, ef=EF, counters=True), want, "inner product")
    hg.release()


def test_marked_nodes_are_legal_queries_and_never_in_their_row(H, world):
    w = world
    hg = w.fresh()
    hg.mark_deleted(np.unique(w.nodes))
    assert hg.deleted_count() == len(np.unique(w.nodes))
    for ex in (True, False):
        want, p = _want(H, hg, w.nodes, EF, K, H.FILL_OHNSW, 0, ex)     # the public call on the marked handle: the filtered ladder under the live mask
        if ex:
            assert (p == K).all()                                       # self can never be there
        got = H.Ohnsw.knn_batch_by_id(hg, K, w.nodes, ef=EF, exclude_self=ex, counters=True)
        _same(got, want, "marked, exclude_self %d" % ex)
        assert not np.isin(got[0], np.unique(w.nodes)).any()
    # the filtered ladder was reached: the rows are those of the filtered call under the live mask, stage and all
    live = np.ones(N, bool)
    live[w.nodes] = False
    fi = H.Ohnsw.knn_batch_filtered(hg, K, hg.rows(w.nodes), live, ef=EF, counters=True)
    _same(H.Ohnsw.knn_batch_by_id(hg, K, w.nodes, ef=EF, exclude_self=False, counters=True), fi[:4], "marked against the filtered call")
    hg.release()


# ---- 5. short rows: trailing fills survive the shift -------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0, 1])
def test_short_rows(H, fill):
    hg = H.Ohnsw.build_batch_bigarray(_floats(5, D, 5), M, EFC, seed=1)
    ids = np.arange(5, dtype=np.int32)
    want, p = _want(H, hg, ids, EF, K, fill, 0, True)
    got = H._search_by_id(hg, ids, EF, K, fill, True, True, 0)
    _same(got, want, "fill %d" % fill)
    assert (p == 0).all() and (got[0][:, 4:] == -1).all() and (got[0][:, :4] >= 0).all()
    tail = got[1][:, 4:]
    assert np.isinf(tail).all() if fill else np.isnan(tail).all()
    hg.release()


# ---- 6. inherited paths: one case each against the public call over the gathered rows ----------------------------------------------

@pytest.mark.parametrize("path", ["half_rows", "sq8_dim_rows+refine", "bit_rows+bit_query_bits", "cosine", "insert"])
def test_inherited_paths(H, world, path):
    w = world
    hg = w.fresh(0, H.METRIC_COSINE if path == "cosine" else H.METRIC_L2)
    ids = w.nodes
    if path == "half_rows":
        hg.set_option("half_rows", 1)
        assert hg.info().row_format == H.ROWS_HALF
    elif path == "sq8_dim_rows+refine":
        hg.set_option("sq8_dim_rows", 1)
        hg.set_option("refine", -1)
        assert hg.info().row_format == H.ROWS_SQ8_DIM
    elif path == "bit_rows+bit_query_bits":
        hg.set_option("bit_rows", 1)
        hg.set_option("bit_query_bits", 4)
        assert hg.info().row_format == H.ROWS_BITS
    elif path == "insert":
        new = H.Ohnsw.insert_batch(hg, _floats(37, D, 9), M, EFC, seed=3)
        ids = np.concatenate([w.nodes[:20], new[[0, 17, 36]]]).astype(np.int32)             # old nodes and new ones
    for ex in (False, True):
        want, _ = _want(H, hg, ids, EF, K, H.FILL_OHNSW, 0, ex)
        _same(H.Ohnsw.knn_batch_by_id(hg, K, ids, ef=EF, exclude_self=ex, counters=True), want, "%s, exclude_self %d" % (path, ex))
    hg.release()


# ---- 7. keys ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ex", [False, True])
def test_by_key(H, world, ex):
    w = world
    by_id = H.Ohnsw.knn_batch_by_id(w.keyed, K, w.nodes, ef=EF, exclude_self=ex, counters=True)
    _same(by_id, H.Ohnsw.knn_batch_by_id(w.hg, K, w.nodes, ef=EF, exclude_self=ex, counters=True), "keys change no by-id row")
    got = H.Ohnsw.knn_batch_by_key(w.keyed, K, w.keys[w.nodes], ef=EF, exclude_self=ex, counters=True, missing=MISSING)
    assert got[0].dtype == np.int64
    _same(got, (_translate(w.keys, by_id[0]),) + by_id[1:], "exclude_self %d" % ex)
    ba = H.Ba.knn_batch_by_key(w.keyed, w.keys[w.nodes], EF, K, exclude_self=ex, missing=MISSING)
    want = H.Ba.knn_batch_by_id(w.keyed, w.nodes, EF, K, exclude_self=ex)
    _same(ba, (_translate(w.keys, want[0]), want[1]), "functor rule, exclude_self %d" % ex)


def test_by_key_fills_are_the_missing_key(H):
    hg = H.Ohnsw.build_batch_bigarray(_floats(5, D, 5), M, EFC, seed=1)
    keys = nasty_keys(5)
    hg.set_keys(keys)
    got = H.Ohnsw.knn_batch_by_key(hg, K, keys, ef=EF, missing=MISSING)
    by_id = H.Ohnsw.knn_batch_by_id(hg, K, np.arange(5), ef=EF)
    _same(got, (_translate(keys, by_id[0]), by_id[1]))
    assert (got[0][:, 4:] == MISSING).all() and (got[0][:, :4] != MISSING).all()
    hg.release()


def test_by_key_refusals(H, world):
    w = world
    L = H.load()
    absent = MISSING + 1
    assert absent not in set(w.keys.tolist())
    keys = np.array([w.keys[3], absent, w.keys[4], absent - 1], np.int64)
    ok = np.full((4, K), 77, np.int64)
    od = np.full((4, K), 7.5, np.float32)
    nd = np.full(4, 77, np.uint32)
    p = H._SearchParams(EF, K, 0, 0)
    rc = L.hnsw_search_batch_by_key(w.keyed.handle, H._ptr(keys), 4, ctypes.byref(p), 1, MISSING, H._ptr(ok), H._ptr(od), H._ptr(nd), None)
    msg = L.hnsw_last_error().decode()
    assert rc == H.ERR_BAD_ARG and "keys[1]=%d" % absent in msg, msg                 # the first by position, named
    assert (ok == 77).all() and (od == 7.5).all() and (nd == 77).all()                 # nothing written
    with pytest.raises(H.InvalidArgument, match="no keys"):
        H.Ohnsw.knn_batch_by_key(w.hg, K, w.keys[:3], ef=EF)
    assert H.Ohnsw.knn_batch_by_key(w.keyed, K, np.zeros(0, np.int64), ef=EF)[0].shape == (0, K)


# ---- 8. the exact form -------------------------------------------------------------------------------------------------------------

def test_brute_force_by_id(H, world):
    w = world
    for hg in (w.hg, w.fresh(1)):
        ids = w.nodes + hg.id_base
        Q = hg.rows(ids)
        _same(H.Ohnsw.brute_force_by_id(hg, K, ids, exclude_self=False), H.Ohnsw.brute_force_knn(hg, K, Q), "base %d keep" % hg.id_base)
        for fill in (H.FILL_OHNSW, H.FILL_BA):
            want, p = drop_self(H.Ohnsw.brute_force_knn(hg, K + 1, Q, fill=fill), ids, K)
            assert (p == 0).all()                                           # distinct Gaussian vectors: self is the nearest
            _same(H.Ohnsw.brute_force_by_id(hg, K, ids, fill=fill), want, "base %d fill %d" % (hg.id_base, fill))
        if hg is not w.hg:
            hg.release()


def test_brute_force_by_id_among_duplicates(H):
    X = _floats(200, D, 21)
    copies = np.array([3, 17, 18, 40, 41, 42, 77, 90, 101, 120, 150, 151, 180, 190])
    X[copies] = X[3]                                                        # one vector stored 14 times
    hg = H.Hgraph.flat(X)
    ids, dist = H.Ohnsw.brute_force_by_id(hg, K, [190])
    np.testing.assert_array_equal(ids[0], copies[:K])                       # 13 lower copies precede self: the first 10, self absent
    assert (dist[0] == 0).all()
    # 8 queries, copies among them: the row = the (distance, id) order over hnsw_distance_batch's distances with self removed
    q = np.array([3, 41, 190, 0, 5, 100, 199, 151], np.int32)
    table = H.Ohnsw.distance_l2(hg, hg.rows(q), np.tile(np.arange(200, dtype=np.int32), (len(q), 1)))
    got, gd = H.Ohnsw.brute_force_by_id(hg, K, q)
    for i, v in enumerate(q):
        order = np.lexsort((np.arange(200), table[i]))
        want = order[order != v][:K]
        assert sorted(got[i].tolist()) == sorted(want.tolist()), (v, got[i], want)
        np.testing.assert_array_equal(_bits(gd[i]), _bits(table[i][got[i]]))
    hg.release()


# ---- 9. the k-NN graph ---------------------------------------------------------------------------------------------------------------

def test_knn_graph(H, world):
    w = world
    hg = w.fresh()
    everyone = np.arange(N, dtype=np.int32)
    want = H.Ohnsw.knn_batch_by_id(hg, K, everyone, ef=EF)
    _same(hg.knn_graph(K, ef=EF), want, "default chunk")
    for chunk in (500, 2003, 2004):                                          # boundaries at 500 .. 2000 and a last chunk of 3; one chunk either way
        hg.set_option("graph_chunk_rows", chunk)
        _same(hg.knn_graph(K, ef=EF), want, "chunk %d" % chunk)
    hg.set_option("graph_chunk_rows", 500)
    np.testing.assert_array_equal(hg.knn_graph(K, ef=EF, distances=False), want[0])
    _same(hg.knn_graph(K, exact=True), H.Ohnsw.brute_force_by_id(hg, K, everyone), "exact")
    _same(hg.knn_graph(K, ef=EF, sem=H.SEM_FUNCTOR, fill=H.FILL_BA), H.Ba.knn_batch_by_id(hg, everyone, EF, K), "functor rule")
    with pytest.raises(H.InvalidArgument, match="graph_chunk_rows"):
        hg.set_option("graph_chunk_rows", 0)
    with pytest.raises(H.Failure, match=r"\[%d\]" % UNSUPPORTED):
        hg.knn_graph(1024, ef=1024)
    hg.release()
    one = w.fresh(1)
    one.set_option("graph_chunk_rows", 700)
    _same(one.knn_graph(K, ef=EF), H.Ohnsw.knn_batch_by_id(one, K, everyone + 1, ef=EF), "id_base 1")
    one.release()
    empty = H.Hgraph.flat(np.zeros((0, 4), np.float32))
    ids, dist = empty.knn_graph(K)
    assert ids.shape == (0, K) and dist.shape == (0, K)                     # n == 0 is OK
    empty.release()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(H, world):
    w = world
    for base in (0, 1):
        hg = w.fresh(base) if base else w.hg
        bad = np.array([base + 5, base + N, base - 1, base + 6], np.int32)
        out = (np.full((4, K), 77, np.int32), np.full((4, K), 7.5, np.float32))
        for call in (lambda: H.Ohnsw.knn_batch_by_id(hg, K, bad, ef=EF, out=out), lambda: H.Ohnsw.brute_force_by_id(hg, K, bad)):
            with pytest.raises(H.InvalidArgument, match=r"ids\[1\]=%d" % (base + N)):       # the first by position, named
                call()
        assert (out[0] == 77).all() and (out[1] == 7.5).all()                               # nothing written
        if base:
            hg.release()
    with pytest.raises(H.InvalidArgument, match="exclude_self"):
        H._search_by_id(w.hg, w.nodes, EF, K, H.FILL_OHNSW, 2)
    with pytest.raises(H.InvalidArgument, match="exclude_self"):
        H._search_by_id(w.hg, w.nodes, EF, K, H.FILL_OHNSW, -1)
    with pytest.raises(H.InvalidArgument, match="NEAREST_K"):
        H._search_by_id(w.hg, w.nodes, EF, K, H.FILL_BA, True, sem=H.SEM_FUNCTOR_NEAREST_K)
    ids, dist = H._search_by_id(w.hg, w.nodes[:3], EF, K, H.FILL_BA, False, sem=H.SEM_FUNCTOR_NEAREST_K)      # ... which exclude_self = 0 inherits
    _same((ids, dist), H._search(w.hg, w.hg.rows(w.nodes[:3]), EF, K, H.FILL_BA, sem=H.SEM_FUNCTOR_NEAREST_K))
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_by_id(w.hg, 20, w.nodes, ef=EF, exclude_self=False)               # k > ef: the public call's own check
    for ex in (False, True):                                                                # nq == 0 is a no-op
        ids, dist = H.Ohnsw.knn_batch_by_id(w.hg, K, np.zeros(0, np.int32), ef=EF, exclude_self=ex)
        assert ids.shape == (0, K) and dist.shape == (0, K)
    assert H.Ohnsw.brute_force_by_id(w.hg, K, [])[0].shape == (0, K)


# ---- 11. page-locked outputs: the epilogue writes in place --------------------------------------------------------------------------

def test_page_locked_outputs(H, world):
    w = world
    nq = len(w.nodes)
    for ex in (True, False):
        want = H.Ohnsw.knn_batch_by_id(w.hg, K, w.nodes, ef=EF, exclude_self=ex, counters=True)
        out = (H.host_empty((nq, K), np.int32), H.host_empty((nq, K), np.float32))
        out[0][:] = 77
        out[1][:] = 7.5
        got = H.Ohnsw.knn_batch_by_id(w.hg, K, w.nodes, ef=EF, exclude_self=ex, counters=True, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _same(got, want, "page-locked, exclude_self %d" % ex)
    # ... and the keys of the keyed call
    L = H.load()
    want = H.Ohnsw.knn_batch_by_key(w.keyed, K, w.keys[w.nodes], ef=EF, counters=True, missing=MISSING)
    ok, od = H.host_empty((nq, K), np.int64), H.host_empty((nq, K), np.float32)
    nd, nh = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
    keys = np.ascontiguousarray(w.keys[w.nodes])
    p = H._SearchParams(EF, K, 0, 0)
    H._check(L.hnsw_search_batch_by_key(w.keyed.handle, H._ptr(keys), nq, ctypes.byref(p), 1, MISSING, H._ptr(ok), H._ptr(od), H._ptr(nd), H._ptr(nh)))
    _same((ok, od, nd, nh), want, "page-locked keys")


# ---- 12. the C++ front end -----------------------------------------------------------------------------------------------------------

def test_cpp_front_end_by_id(H, tmp_path):
    from conftest import ROOT
    exe = str(tmp_path / "test_front_by_id")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_by_id.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "by-id front-end ok" in out.stdout, out.stdout + out.stderr
