"""Option "head_queries" (hnsw_search_batch, csrc/hnsw_capi.hip): a host call that reads its page-locked query matrix in place and
would order its batch searches rows [0, H) in a plain launch on a second stream and orders only the rows behind them; the two
parts join at the end of the call.  Nothing a caller sees may depend on H: ids, distance bits, evaluation and hop counts are
compared with those of head_queries = 0 bit for bit -- byte rows (the hand-scheduled loop) and 24-dimensional float rows (the C++
loop), L2 and inner product, both accept rules, results in place with the counters staged and in place, flagged queries on both
sides of the split, the time_kernels record -- and a call that must not split (pageable queries, order_queries 0) ignores it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EF, K = 32, 10
NQS = (2, 65, 700)


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1
    return H


def _heads(nq):
    return sorted({1, 64, nq - 1, nq // 2})


@pytest.fixture(scope="module")
def indices(H):
    """name -> (index, 700 pageable queries): byte-valued d = 128 under L2 and under the inner product, float d = 24 under L2"""
    rng = np.random.default_rng(11)
    n = 4000
    Xb = rng.integers(0, 219, size=(n, 128)).astype(np.float32)
    Qb = rng.integers(0, 219, size=(max(NQS), 128)).astype(np.float32)
    Xf = rng.standard_normal((n, 24)).astype(np.float32)
    Qf = rng.standard_normal((max(NQS), 24)).astype(np.float32)
    out = {}
    for name, X, Q, metric in (("bytes", Xb, Qb, 0), ("bytes_ip", Xb, Qb, 1), ("float", Xf, Qf, 0)):
        hg = H.Ohnsw.build_batch_bigarray(X, 12, 60, seed=1, metric=metric)
        assert hg.row_bytes() == (128 if name != "float" else 96)
        hg.set_option("order_queries", 1)
        out[name] = (hg, Q)
    yield out
    for hg, _ in out.values():
        hg.release()


def _pinned(H, a):
    p = H.host_empty(a.shape, a.dtype)
    p[:] = a
    return p


def _call(H, hg, Q, head, sem=0, pinned_counters=False, ef=EF, k=K):
    """one hnsw_search_batch with head_queries = head: results into fresh page-locked matrices, the counters into pageable arrays
    (staged: their download has to come behind the join) or page-locked ones -> (ids, distance bits, ndist, nhops)"""
    C = H._C
    nq = Q.shape[0]
    oi, od = H.host_empty((nq, k), np.int32), H.host_empty((nq, k), np.float32)
    oi[:] = -7
    od[:] = np.nan
    nd, nh = (H.host_empty(nq, np.uint32), H.host_empty(nq, np.uint32)) if pinned_counters else (np.zeros(nq, np.uint32), np.zeros(nq, np.uint32))
    nd[:] = 0
    nh[:] = 0
    hg.set_option("head_queries", head)
    p = H._SearchParams(ef, k, H.FILL_BA if sem else H.FILL_OHNSW, sem)
    H._check(H.load().hnsw_search_batch(hg.handle, H._ptr(Q), nq, Q.shape[1], C.byref(p), H._ptr(oi), H._ptr(od), H._ptr(nd), H._ptr(nh)))
    hg.set_option("head_queries", -1)
    return oi.copy(), od.view(np.uint32).copy(), np.array(nd), np.array(nh)


def _same(want, got, ctx):
    for name, a, b in zip(("ids", "distance bits", "ndist", "nhops"), want, got):
        np.testing.assert_array_equal(a, b, err_msg="%s: %s" % (ctx, name))


@pytest.mark.parametrize("sem", [0, 1], ids=["ohnsw", "functor"])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", ["bytes", "bytes_ip", "float"])
def test_any_head_gives_the_unsplit_call(H, indices, name, nq, sem):
    hg, Q = indices[name]
    Qp = _pinned(H, Q[:nq])
    sem = H.SEM_FUNCTOR if sem else H.SEM_OHNSW
    want = _call(H, hg, Qp, 0, sem)
    assert (want[0] != -7).all()                                           # every row was written (_call pre-fills with -7)
    assert (want[2] > 0).all()
    for head in _heads(nq):
        _same(want, _call(H, hg, Qp, head, sem), "%s nq %d head %d" % (name, nq, head))
    # the counters written in place as well
    _same(want, _call(H, hg, Qp, nq // 2, sem, pinned_counters=True), "%s nq %d head %d, counters in place" % (name, nq, nq // 2))
    # and the automatic choice
    _same(want, _call(H, hg, Qp, -1, sem), "%s nq %d automatic" % (name, nq))


def test_calls_that_do_not_split_ignore_the_option(H, indices):
    hg, Q = indices["bytes"]
    Qp = _pinned(H, Q)
    want = _call(H, hg, Qp, 0)
    # a pageable query matrix is staged by a copy: no head, whatever the option says
    for head in (1, 350, 699, 10 ** 12):
        _same(want, _call(H, hg, Q, head), "pageable queries, head %d" % head)
    hg.set_option("order_queries", 0)
    try:
        for head in (1, 350, 699):
            _same(want, _call(H, hg, Qp, head), "order_queries 0, head %d" % head)
    finally:
        hg.set_option("order_queries", 1)


def test_time_kernels_records_one_call_per_call(H, indices):
    hg, Q = indices["bytes"]
    Qp = _pinned(H, Q)
    hg.set_option("time_kernels", 1)
    try:
        hg.kernel_times()
        for head in (0, 350):
            _call(H, hg, Qp, head)
            search_ms, prepass_ms, calls = hg.kernel_times()
            assert calls == 1 and search_ms > 0 and prepass_ms > 0, (head, search_ms, prepass_ms, calls)
    finally:
        hg.set_option("time_kernels", 0)


def test_flagged_queries_on_both_sides_of_the_split_are_repaired(H):
    """The graph of test_tie_list_overflow_through_the_loops at ef 128: ef - 1 identical shell points fill W behind the far entry
    node and a chain of ever closer points evicts them while they are unexpanded and tied with the new maximum -- more than the 64
    LDS slots of the tie list, so every query is flagged and searched again by the host call, after the join, over the whole batch."""
    import torch
    ef = 128
    shells, chain = ef - 1, 100
    n = 1 + shells + chain + 1
    pos = np.zeros(n, np.float32)
    pos[0] = 250.0
    pos[1:1 + shells] = 150.0
    pos[1 + shells:1 + shells + chain] = 149.0 - np.arange(chain)
    z = n - 1
    pos[z] = 1.0
    rows = [[] for _ in range(n)]
    width = 64
    first = list(range(1, 1 + shells))
    rows[0] = first[:width]
    rest = first[width:]
    hub = 1
    while rest:
        rows[hub] = rest[:width - 1]
        rest = rest[width - 1:]
        hub += 1
    rows[1] = rows[1][:width - 1] + [1 + shells]
    for i in range(chain - 1):
        rows[1 + shells + i] = [2 + shells + i]
    late = 1 + (shells * 2) // 3
    rows[late] = (rows[late] + [z])[:width]
    deg0 = np.array([len(r) for r in rows], np.int32)
    nbr0 = np.full((n, width), -1, np.int32)
    for i, r in enumerate(rows):
        nbr0[i, :len(r)] = r
    X = np.zeros((n, 128), np.float32)
    X[:, 0] = pos
    hg = H.Hgraph(X, deg0, nbr0, entry_point=0, max_degree=32)
    hg.to_device(0)
    hg.set_option("order_queries", 1)
    nq = 9
    Q = np.zeros((nq, 128), np.float32)
    Q[:, 1] = np.arange(nq) % 3                                            # (the same walk, three different distance offsets)
    # every query is flagged by a launch without the fallback
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    ids = torch.empty((nq, 10), dtype=torch.int32, device=dev)
    dd = torch.empty((nq, 10), dtype=torch.float32, device=dev)
    st = torch.zeros(nq, dtype=torch.int32, device=dev)
    H.search_batch_device(hg, Qd.data_ptr(), nq, 128, ef, 10, ids.data_ptr(), dd.data_ptr(), 0, 0, st.data_ptr(), 0)
    torch.cuda.synchronize()
    assert (st & 1).cpu().numpy().astype(bool).all()
    Qp = _pinned(H, Q)
    want = _call(H, hg, Qp, 0, ef=ef)
    assert (want[0][:, 0] == z).all()                                      # the point behind the late shell: found by the repair only
    for head in (1, 4, 8):
        _same(want, _call(H, hg, Qp, head, ef=ef), "flagged queries, head %d" % head)
    hg.release()


def test_the_option_takes_any_value(H, indices):
    hg, Q = indices["float"]
    for v in (-1, 0, 1, 64, 10 ** 12, -5, -1):
        hg.set_option("head_queries", v)
    with pytest.raises(Exception):
        hg.set_option("head_querie", 1)
    # a sharded index reads every shard's current value (get_option) before it sets the new one
    sh = H.ShardedHgraph.build(Q, 8, 40, devices=[0, 0], seed=1)
    try:
        for v in (5, 0, -1):
            sh.set_option("head_queries", v)
    finally:
        sh.release()
