"""Soft deletion owned by the index (ocaml-hnsw_amd/csrc/hnsw_soft_delete.hip): hnsw_index_mark_deleted / unmark_deleted /
deleted_count / deleted_bits / compact, and every entry point that honours the marks, against the header's definition.

That definition is in terms of calls that exist, so every check is bit for bit: each case has a TWIN handle of the same graph that
is never marked and is searched under Hgraph.filter(live) -- the marked handle's plain calls must give the twin's filtered rows,
counters included.  The exact scans are held against the oracle's full order restricted to the live nodes.  The world is the one
of tests/test_gpu_range.py: 2003 Gaussian vectors of 20 dimensions, the oracle's graph (M 8, efC 40, seed 1), 64 queries, ef 16."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT = 0xFFFFFFFF
N, D, NQ, EF, K = 2003, 20, 64, 16, 10
SEVEN = (0, 31, 32, 1001, 1002, 1984, 2002)


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.space = oracle.Space.l2(w.X, arith=oracle.TREE16)
    w.g = oracle.build_ohnsw(w.space, 8, 40, seed=1)
    w.full_ids, w.full_dist = oracle.brute_force_knn(w.space, w.Q, N)           # every query's full order (distance, id)
    w.new = lambda: H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, id_base=0, max_degree=8)
    w.plain = w.new()                                                           # a handle never marked
    yield w
    w.plain.release()


def _marked_sets():
    rng = np.random.default_rng(123)
    sets = {"5 %": rng.permutation(N) < N // 20, "50 %": rng.permutation(N) < N // 2,
            "all but every 100th": np.arange(N) % 100 != 0, "all but seven": np.ones(N, bool), "every node": np.ones(N, bool)}
    sets["all but seven"][list(SEVEN)] = False
    return sets


MARKED = _marked_sets()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, ctx=""):
    assert len(got) == len(want), ctx
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)), err_msg="%s [%d]" % (ctx, i))


def _pair(w, marked):
    """(the marked handle, its never-marked twin, the twin's filter of the live nodes)"""
    hg, twin = w.new(), w.new()
    hg.mark_deleted(np.flatnonzero(marked))
    assert hg.deleted_count() == int(marked.sum())
    np.testing.assert_array_equal(hg.deleted_mask(), marked)
    assert hg.info().n == N                                     # n stays the stored count
    return hg, twin, twin.filter(~marked)


def _restricted(w, live, k, fill_nan=True):
    """the k smallest live nodes of every query under (distance, id), the rest filled: from the oracle's full order"""
    ids = np.full((NQ, k), -1, np.int32)
    dist = np.full((NQ, k), np.nan if fill_nan else np.inf, np.float32)
    for q in range(NQ):
        keep = live[w.full_ids[q]]
        c = min(k, int(keep.sum()))
        ids[q, :c], dist[q, :c] = w.full_ids[q][keep][:c], w.full_dist[q][keep][:c]
    return ids, dist


# ---- 1. the search calls under marks -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(MARKED))
def test_searches_answer_under_the_live_mask(H, world, case):
    w, marked = world, MARKED[case]
    live = ~marked
    hg, twin, flt = _pair(w, marked)
    L = H.load()
    for sem, fill in ((H.SEM_OHNSW, H.FILL_OHNSW), (H.SEM_FUNCTOR, H.FILL_BA)):
        want = H._search_filtered(twin, flt, w.Q, EF, K, fill, True, sem=sem)
        stage = want[4]
        got = H._search(hg, w.Q, EF, K, fill, True, sem=sem)
        _same(got, want[:4], "%s rule %d" % (case, sem))        # ids, distance bits, evaluations, hops
        print("%s rule %d: stages %s" % (case, sem, dict(zip(*[a.tolist() for a in np.unique(stage, return_counts=True)]))))
        # the classes each marked set is here for, on the twin's own output
        if case == "50 %":
            assert len(np.unique(stage)) >= 2
        if case == "all but every 100th":
            assert live.sum() == 21 and (stage == EXACT).any()
        if case in ("all but seven", "every node"):             # n_allowed < k: no walk, filled rows
            assert (stage == EXACT).all() and (want[3] == 0).all() and (want[2] == live.sum()).all()
            real = int(live.sum())
            assert (got[0][:, real:] == -1).all()
            tail = got[1][:, real:]
            assert np.isnan(tail).all() if fill == H.FILL_OHNSW else np.isposinf(tail).all()
        assert not marked[got[0][got[0] >= 0]].any()
    # hnsw_knn: the same row, *out_count = the real entries
    p = H._SearchParams(EF, K, H.FILL_OHNSW, H.SEM_OHNSW)
    want = H._search_filtered(twin, flt, w.Q, EF, K, H.FILL_OHNSW)
    for q in (0, 17, 63):
        ids, dist, cnt = np.zeros(K, np.int32), np.zeros(K, np.float32), ctypes.c_int32(-5)
        assert L.hnsw_knn(hg.handle, w.Q[q].ctypes.data, ctypes.byref(p), ids.ctypes.data, dist.ctypes.data, ctypes.byref(cnt)) == H.OK
        _same((ids, dist), (want[0][q], want[1][q]), "%s knn %d" % (case, q))
        assert cnt.value == int((want[0][q] >= 0).sum()) == min(K, int(live.sum()))
    # the k farthest of W have no filtered meaning
    p = H._SearchParams(EF, K, H.FILL_BA, H.SEM_FUNCTOR_NEAREST_K)
    ids, dist = np.zeros((NQ, K), np.int32), np.zeros((NQ, K), np.float32)
    assert L.hnsw_search_batch(hg.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(p), ids.ctypes.data, dist.ctypes.data, None, None) == H.ERR_BAD_ARG
    flt.release()
    twin.release()
    hg.release()


@pytest.mark.parametrize("case", list(MARKED))
def test_exact_scans_are_over_the_live_nodes(H, world, case):
    import torch
    w, marked = world, MARKED[case]
    hg = w.new()
    hg.mark_deleted(np.flatnonzero(marked))
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(w.Q).to(dev)
    for k in (10, 1024):
        for fill in (H.FILL_OHNSW, H.FILL_BA):
            want = _restricted(w, ~marked, k, fill == H.FILL_OHNSW)
            _same(H.Ohnsw.brute_force_knn(hg, k, w.Q, fill=fill), want, "%s scan k %d" % (case, k))
            ids = torch.empty((NQ, k), dtype=torch.int32, device=dev)
            dd = torch.empty((NQ, k), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            H.brute_force_device(hg, Qd.data_ptr(), NQ, D, k, ids.data_ptr(), dd.data_ptr(), fill=fill)
            torch.cuda.synchronize()
            _same((ids.cpu().numpy(), dd.cpu().numpy()), want, "%s device scan k %d" % (case, k))
    hg.release()


@pytest.mark.parametrize("case", list(MARKED))
def test_range_calls_are_the_filtered_forms(H, world, case):
    w, marked = world, MARKED[case]
    hg, twin, flt = _pair(w, marked)
    for radius in (4.5, 6.0):
        for sem in (H.SEM_OHNSW, H.SEM_FUNCTOR):
            _same(H._range_search(hg, w.Q, radius, EF, sem, True), H._range_search(twin, w.Q, radius, EF, sem, True, filter=flt),
                  "%s range radius %g rule %d" % (case, radius, sem))
        _same(H.Ohnsw.brute_force_range(hg, radius, w.Q, counters=True), H.Ohnsw.brute_force_range(twin, radius, w.Q, counters=True, filter=flt),
              "%s range scan radius %g" % (case, radius))
    got = H.Ohnsw.brute_force_range(hg, float("inf"), w.Q, counters=True)
    assert (np.diff(got[0]) == (~marked).sum()).all() and not marked[got[1]].any()
    if case == "every node":                                    # empty segments, not HNSW_ERR_EMPTY_INDEX
        got = H.Ohnsw.range_search(hg, 6.0, w.Q, ef=EF, counters=True)
        assert (got[0] == 0).all() and (got[5] == EXACT).all() and (got[3] == 0).all() and (got[4] == 0).all()
    flt.release()
    twin.release()
    hg.release()


def test_new_filters_are_anded_with_the_live_mask(H, world):
    w, marked = world, MARKED["50 %"]
    hg, twin, flt = _pair(w, marked)
    allow = np.random.default_rng(9).permutation(N) < N // 3
    f, tf = hg.filter(allow), twin.filter(allow & ~marked)
    assert f.count() == tf.count() == int((allow & ~marked).sum())
    np.testing.assert_array_equal(f.bits(), tf.bits())
    np.testing.assert_array_equal(f.bits(), H.pack_allow(allow & ~marked, N))
    _same(H._search_filtered(hg, f, w.Q, EF, K, H.FILL_OHNSW, True), H._search_filtered(twin, tf, w.Q, EF, K, H.FILL_OHNSW, True), "ANDed filter")
    _same(H._range_search(hg, w.Q, 4.5, EF, 0, True, filter=f), H._range_search(twin, w.Q, 4.5, EF, 0, True, filter=tf), "ANDed filter, range")
    # seven labels, one unused (label 5); a marked node's label counts as -1
    labels = (np.arange(N) % 7).astype(np.int32)
    labels[labels == 5] = 6
    labels[::11] = -1
    fs = hg.filters_by_label(labels, 7)
    for l, fl in enumerate(fs):
        want = (labels == l) & ~marked
        assert fl.count() == int(want.sum()), l
        np.testing.assert_array_equal(fl.bits(), H.pack_allow(want, N), err_msg="label %d" % l)
    assert fs[5].count() == 0
    which = (np.arange(NQ) % 7).astype(np.int32)
    tfs = [twin.filter((labels == l) & ~marked) for l in range(7)]
    _same(H._search_filtered_each(hg, fs, which, w.Q, EF, K, H.FILL_OHNSW, True), H._search_filtered_each(twin, tfs, which, w.Q, EF, K, H.FILL_OHNSW, True),
          "label filters")
    for x in fs + tfs + [f, tf, flt]:
        x.release()
    twin.release()
    hg.release()


# ---- 2. the graph-changing calls under marks -----------------------------------------------------------------------------------

def _same_graph(a, b):
    a.export()
    b.export()
    assert (a.entry_point, a.max_layer, a.n) == (b.entry_point, b.max_layer, b.n)
    np.testing.assert_array_equal(a.deg0, b.deg0)
    np.testing.assert_array_equal(a.nbr0, b.nbr0)
    assert len(a.upper) == len(b.upper)
    for u, v in zip(a.upper, b.upper):
        for x, y in zip(u, v):
            np.testing.assert_array_equal(x, y)


def test_insert_keeps_the_marks_and_the_new_nodes_are_live(H, world):
    w, marked = world, MARKED["5 %"]
    hg, twin, flt = _pair(w, marked)
    flt.release()
    extra = _floats(100, D, 3)
    for h in (hg, twin):
        H.Ohnsw.insert_batch(h, extra, 8, 40, seed=1)
    grown = np.concatenate([marked, np.zeros(100, bool)])
    np.testing.assert_array_equal(hg.deleted_mask(), grown)
    assert hg.deleted_count() == int(marked.sum()) and hg.info().n == N + 100
    flt = twin.filter(~grown)
    _same(H._search(hg, w.Q, EF, K, H.FILL_OHNSW, True), H._search_filtered(twin, flt, w.Q, EF, K, H.FILL_OHNSW, True)[:4], "after insert")
    _same(H._range_search(hg, w.Q, 4.5, EF, 0, True), H._range_search(twin, w.Q, 4.5, EF, 0, True, filter=flt), "after insert, range")
    near = H.Ohnsw.brute_force_knn(hg, 1, extra[:5] + np.float32(1e-4))[0][:, 0]
    np.testing.assert_array_equal(near, N + np.arange(5))          # the new nodes are live: the masked scan returns them
    flt.release()
    twin.release()
    hg.release()


def test_remove_moves_the_marks_with_their_nodes(H, world):
    w, marked = world, MARKED["5 %"]
    hg, twin, flt = _pair(w, marked)
    flt.release()
    rng = np.random.default_rng(5)
    gone = np.concatenate([rng.choice(np.flatnonzero(marked), 10, replace=False), rng.choice(np.flatnonzero(~marked), 40, replace=False)])
    new_id = H.Ohnsw.remove_batch(hg, gone)
    np.testing.assert_array_equal(H.Ohnsw.remove_batch(twin, gone), new_id)
    want = np.zeros(N - 50, bool)
    want[new_id[marked & (new_id >= 0)]] = True
    np.testing.assert_array_equal(hg.deleted_mask(), want)
    assert hg.deleted_count() == int(marked.sum()) - 10 == int(want.sum())
    flt = twin.filter(~want)
    _same(H._search(hg, w.Q, EF, K, H.FILL_OHNSW, True), H._search_filtered(twin, flt, w.Q, EF, K, H.FILL_OHNSW, True)[:4], "after remove")
    flt.release()
    twin.release()
    hg.release()


def test_compact_is_remove_of_the_marked_nodes(H, world):
    import torch
    w, marked = world, MARKED["5 %"]
    hg, twin, flt = _pair(w, marked)
    flt.release()
    new_id = hg.compact()
    np.testing.assert_array_equal(new_id, H.Ohnsw.remove_batch(twin, np.flatnonzero(marked)))
    assert hg.deleted_count() == 0 and not hg.deleted_mask().any() and hg.info().n == N - int(marked.sum())
    _same_graph(hg, twin)                                       # layer 0 and every upper layer, link for link
    _same(H._search(hg, w.Q, EF, K, H.FILL_OHNSW, True), H._search(twin, w.Q, EF, K, H.FILL_OHNSW, True), "after compact")
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(w.Q).to(dev)
    out = []
    for h in (hg, twin):                                        # the device form is accepted again
        ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        H.search_batch_device(h, Qd.data_ptr(), NQ, D, EF, K, ids.data_ptr(), dd.data_ptr())
        torch.cuda.synchronize()
        out.append((ids.cpu().numpy(), dd.cpu().numpy()))
    _same(out[0], out[1], "device form after compact")
    np.testing.assert_array_equal(hg.compact(), np.arange(hg.info().n))         # nothing marked: the identity
    twin.release()
    hg.release()


def test_unmarking_everything_gives_the_plain_paths_back(H, world):
    import torch
    w, marked = world, MARKED["50 %"]
    hg = w.new()
    hg.mark_deleted(np.flatnonzero(marked))
    hg.unmark_deleted(np.flatnonzero(marked)[::2])
    assert hg.deleted_count() == int(marked.sum()) - len(np.flatnonzero(marked)[::2])
    hg.unmark_deleted(np.arange(N))                             # unmarking a live node is allowed and does nothing
    assert hg.deleted_count() == 0 and not hg.deleted_mask().any()
    _same(H._search(hg, w.Q, EF, K, H.FILL_OHNSW, True), H._search(w.plain, w.Q, EF, K, H.FILL_OHNSW, True), "search")
    _same(H._range_search(hg, w.Q, 4.5, EF, 0, True), H._range_search(w.plain, w.Q, 4.5, EF, 0, True), "range")
    _same(H.Ohnsw.brute_force_knn(hg, K, w.Q), H.Ohnsw.brute_force_knn(w.plain, K, w.Q), "scan")
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(w.Q).to(dev)
    out = []
    for h in (hg, w.plain):
        ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        H.search_batch_device(h, Qd.data_ptr(), NQ, D, EF, K, ids.data_ptr(), dd.data_ptr())
        torch.cuda.synchronize()
        out.append((ids.cpu().numpy(), dd.cpu().numpy()))
    _same(out[0], out[1], "device form")
    hg.release()


# ---- 3. refusals and their lifting ---------------------------------------------------------------------------------------------

def test_refusals_while_marked_and_their_lifting(H, world):
    import torch
    w = world
    L = H.load()
    hg = w.new()
    old = hg.filter(np.arange(N) % 2 == 0)                      # made before the first mark
    H.Ohnsw.knn_batch_filtered(hg, K, w.Q, old, ef=EF)
    hg.mark_deleted([5, 6, 7])
    with pytest.raises(H.InvalidArgument, match="filter"):      # ... and refused after it: HNSW_ERR_BAD_ARG
        H.Ohnsw.knn_batch_filtered(hg, K, w.Q, old, ef=EF)
    old.release()
    cur = hg.filter(np.arange(N) % 2 == 0)
    hg.mark_deleted([5, 6])                                     # marked already: no bit changes, the filter stays current
    H.Ohnsw.knn_batch_filtered(hg, K, w.Q, cur, ef=EF)
    hg.unmark_deleted([7])                                      # a bit changed
    with pytest.raises(H.InvalidArgument, match="filter"):
        H.Ohnsw.knn_batch_filtered(hg, K, w.Q, cur, ef=EF)
    cur.release()
    assert hg.deleted_count() == 2

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(w.Q).to(dev)
    ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    dd = torch.empty((NQ, K), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def forms():
        p = H._SearchParams(EF, K, H.FILL_OHNSW, H.SEM_OHNSW)
        rcs = [L.hnsw_search_batch_device(hg.handle, Qd.data_ptr(), NQ, D, ctypes.byref(p), ids.data_ptr(), dd.data_ptr(), None, None, None, None)]
        msgs = [L.hnsw_last_error().decode()]
        rcs.append(L.hnsw_search_batch_h2d(hg.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(p), ids.data_ptr(), dd.data_ptr(), None, None, None, None))
        msgs.append(L.hnsw_last_error().decode())
        torch.cuda.synchronize()
        req = ctypes.c_void_p()
        rcs.append(L.hnsw_search_submit(hg.handle, w.Q.ctypes.data, NQ, D, ctypes.byref(p), ctypes.byref(req)))
        msgs.append(L.hnsw_last_error().decode())
        if rcs[-1] == H.OK:
            a, b = np.zeros((NQ, K), np.int32), np.zeros((NQ, K), np.float32)
            assert L.hnsw_search_wait(req, a.ctypes.data, b.ctypes.data, None, None) == H.OK
        with tempfile.TemporaryDirectory() as tmp:
            rcs.append(L.hnsw_index_save(hg.handle, os.path.join(tmp, "marked.hnsw").encode()))
            msgs.append(L.hnsw_last_error().decode())
        return rcs, msgs

    rcs, msgs = forms()
    assert rcs == [H.ERR_UNSUPPORTED] * 3 + [H.ERR_BAD_ARG], rcs
    assert all("compact or unmark first" in m for m in msgs), msgs
    hg.unmark_deleted([5, 6])                                   # the count is back at 0: all accepted again
    assert forms()[0] == [H.OK] * 4

    # bad arguments: refused on the host, the mask unchanged
    hg.mark_deleted([100, 200])
    before = hg.deleted_mask()

    def raw(fn, ids, m=None, handle=None):
        ids = np.asarray(ids, np.int64)
        return fn(hg.handle if handle is None else handle, ids.ctypes.data_as(ctypes.c_void_p), len(ids) if m is None else m)

    for fn in (L.hnsw_index_mark_deleted, L.hnsw_index_unmark_deleted):
        for bad, m, msg in (([3, 5, 3], None, "twice"), ([3, N], None, "not a stored node"), ([-1], None, "not a stored node"), ([1], -1, "m=-1")):
            assert raw(fn, bad, m) == H.ERR_BAD_ARG and msg in L.hnsw_last_error().decode(), msg
        assert fn(hg.handle, None, 2) == H.ERR_BAD_ARG
        assert fn(hg.handle, None, 0) == H.OK                   # m == 0 is a no-op
    np.testing.assert_array_equal(hg.deleted_mask(), before)
    assert hg.deleted_count() == 2
    multi = H.MultiHgraph(w.plain, [0])                         # a replica of an hnsw_multi
    rep = ctypes.c_void_p()
    assert L.hnsw_multi_replica(multi._h, 0, ctypes.byref(rep)) == H.OK
    assert raw(L.hnsw_index_mark_deleted, [1, 2], handle=rep) == H.ERR_BAD_ARG and "replica" in L.hnsw_last_error().decode()
    c = ctypes.c_int64(-1)
    assert L.hnsw_index_deleted_count(rep, ctypes.byref(c)) == H.OK and c.value == 0
    multi.release()
    hg.release()


def test_cpp_front_end_soft_delete(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_soft_delete")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "soft delete front-end ok" in out.stdout, out.stdout + out.stderr
