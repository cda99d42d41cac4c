"""Option "filter_collect" (hnsw_search_collect_kernel, ocaml-hnsw_amd/csrc/hnsw_device.hip.h): filtered k-NN answered from EVERY
node the layer-0 walk evaluates, against the definition the header gives (WITH OPTION filter_collect), restated in Python below
over the exported graph.

The restatement: the greedy descent (the oracle's search_one per upper layer), then the search_k loop with a (key, id) min-heap C
and a max-heap W -- accept iff |W| < e or key < max(W).key, stop when the popped candidate is beyond max(W).  It records the
evaluated set E_e(q) = {entry node} + every neighbour of every expanded node; R_e(q) is the first k allowed members of E_e(q) under
(key, id); the ladder e = ef, 2 ef, ... 1024 serves a query at the first stage with |R| >= k.  Keys are the oracle's TREE16
pre-square-root values (ordering by the square-rooted float32 can swap two keys that round to one distance).  Before it is
trusted, the restatement's W and hop count of every query are held against the oracle's knn_batch_bigarray(k = e, ef = e,
TIES_CANONICAL, counters=True) (`_self_check`).  The exact stage is unchanged by the option: its rows are the option-off rows.

Every query is compared, ids equal and distance bits equal."""
import heapq

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT = 0, 2, 3
EXACT = 0xFFFFFFFF
N, NQ, K = 2003, 64, 10            # n is no multiple of 32: the mask's last word is partial
M, EFC, SEED = 8, 40, 7
# the masks: np.random.default_rng(MASK_SEED).random(N) < s.  With this seed the d 20 world has queries served at stage 0, at a
# later stage and by the exact stage over the grid below (test_parity_d20 asserts it)
MASK_SEED = 20
SELECTIVITIES = (1, 0.5, 0.1, 0.03, 0.01, 0.003, 0)
EFS = (16, 64, 128, 200)           # W in 1, 2, 2 and 4 key registers


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _ladder(ef):
    out = [ef]
    while out[-1] < 1024:
        out.append(min(1024, 2 * out[-1]))
    return out


def _mask(s, n=N, seed=MASK_SEED):
    return np.random.default_rng(seed).random(n) < s


def _fill_value(fill):
    return np.float32(np.nan) if fill == 0 else np.float32(np.inf)


class World:
    """an index, its exported graph, the keys of every (query, node) pair and the restatement's walks (computed once, cached)"""

    def __init__(self, H, oracle, X, Q, metric, row_format, hg=None):
        """hg: an index uploaded from host arrays (its graph is then the host copy); None: the device builder's, exported"""
        self.H, self.o, self.X, self.Q, self.metric = H, oracle, X, Q, metric
        self.hg = hg or H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=SEED, metric=metric)
        assert self.hg.info().row_format == row_format, self.hg.info().row_format
        if hg is None:
            self.hg.export()
        self.g = oracle.Graph(self.hg.n, self.hg.entry_point, self.hg.deg0, self.hg.nbr0, self.hg.upper)
        self.adj0 = [row[row >= 0].tolist() for row in self.hg.nbr0]
        if metric == H.METRIC_L2:
            self.space = oracle.Space.l2(X, arith=oracle.TREE16)
            self.key = np.array([[oracle.l2sq_tree16(x, q) for x in X] for q in Q], np.float32)
            self.dist = np.sqrt(self.key.astype(np.float64)).astype(np.float32)
        else:
            self.space = oracle.Space.ip(X, arith=oracle.TREE16)
            dot = np.array([[oracle.dot_tree16(x, q) for x in X] for q in Q], np.float32)
            self.key = self.dist = np.float32(1.0) - dot
        self.entry0 = []
        for q in Q:                                              # the layer-0 entry node: the greedy descent
            cur = self.hg.entry_point
            for layer in range(self.hg.max_layer, 0, -1):
                cur = oracle.Ohnsw.search_one(self.g, self.space, cur, q, layer)
            self.entry0.append(int(cur))
        self._walks, self._checked = {}, set()

    def walk(self, q, e):
        """-> (W ascending under (key, id), hops, E: every node the layer-0 search evaluates, in evaluation order)"""
        if (q, e) in self._walks:
            return self._walks[(q, e)]
        key = self.key[q].tolist()
        cur = self.entry0[q]
        seen = bytearray(len(key))
        seen[cur] = 1
        E, C, W, hops = [cur], [(key[cur], cur)], [(-key[cur], -cur)], 0
        while C:
            kc, c = heapq.heappop(C)
            if kc > -W[0][0]:
                break
            hops += 1
            for nb in self.adj0[c]:
                if seen[nb]:
                    continue
                seen[nb] = 1
                E.append(nb)
                kn = key[nb]
                if len(W) < e or kn < -W[0][0]:
                    heapq.heappush(C, (kn, nb))
                    heapq.heappush(W, (-kn, -nb))
                    if len(W) > e:
                        heapq.heappop(W)
        ids = [v for _, v in sorted((-a, -b) for a, b in W)]
        self._walks[(q, e)] = (np.array(ids, np.int64), hops, np.array(E, np.int64))
        return self._walks[(q, e)]

    def self_check(self, e):
        """the restatement is the oracle's walk: W and hops of every query at (k = e, ef = e), canonical ties"""
        if e in self._checked:
            return
        o = self.o
        W, _, _, hops = o.Ohnsw.knn_batch_bigarray(self.g, self.space, self.Q, k=e, ef=e, ties=o.TIES_CANONICAL, counters=True)
        for q in range(len(self.Q)):
            ids, h, _ = self.walk(q, e)
            want = W[q][W[q] >= 0]
            np.testing.assert_array_equal(ids, want, err_msg="restatement: W of query %d at e %d" % (q, e))
            assert h == hops[q], "restatement: hops of query %d at e %d: %d, the oracle %d" % (q, e, h, hops[q])
        self._checked.add(e)

    def restate(self, mask, ef, k, fill):
        """the definition -> ids (0-based, -1 filled), distances, stages, hops summed, |E| summed (a lower bound of out_ndist);
        exact-stage rows are left filled: the caller takes them from the option-off call"""
        nq = len(self.Q)
        ids = np.full((nq, k), -1, np.int32)
        dist = np.full((nq, k), _fill_value(fill), np.float32)
        stage = np.full(nq, EXACT, np.uint32)
        hops, evals = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
        if mask.sum() < k:
            return ids, dist, stage, hops, evals + np.uint32(mask.sum())
        for q in range(nq):
            for j, e in enumerate(_ladder(ef)):
                _, h, E = self.walk(q, e)
                hops[q] += h
                evals[q] += len(E)
                A = E[mask[E]]
                if len(A) >= k:
                    order = np.lexsort((A, self.key[q][A]))[:k]
                    ids[q], dist[q], stage[q] = A[order], self.dist[q][A[order]], j
                    break
            else:
                evals[q] += mask.sum()
        return ids, dist, stage, hops, evals

    def release(self):
        self.hg.release()


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


@pytest.fixture(scope="module")
def w20(H, oracle):
    """d 20: ragged rows, NCH 1"""
    rng = np.random.default_rng(1)
    X = rng.normal(size=(N, 20)).astype(np.float32)
    Q = rng.normal(size=(NQ, 20)).astype(np.float32)
    w = World(H, oracle, X, Q, H.METRIC_L2, ROWS_F32)
    yield w
    w.release()


@pytest.fixture(scope="module")
def w20ip(H, oracle):
    w = World(H, oracle, _floats(N, 20, 3), _floats(NQ, 20, 4), H.METRIC_IP, ROWS_F32)
    yield w
    w.release()


@pytest.fixture(scope="module")
def w128(H, oracle):
    """d 128 float: full rows, NCH 2"""
    w = World(H, oracle, _floats(N, 128, 5), _floats(NQ, 128, 6), H.METRIC_L2, ROWS_F32)
    yield w
    w.release()


@pytest.fixture(scope="module")
def wbytes(H, oracle):
    """d 128, byte-valued in 0..7: byte rows, equal distances are frequent.  Three quarters of the queries are byte-valued too
    (the kernel's integer path), the others are not (its float path over the same rows)."""
    rng = np.random.default_rng(7)
    X = rng.integers(0, 8, size=(N, 128)).astype(np.float32)
    Q = rng.integers(0, 8, size=(NQ, 128)).astype(np.float32)
    Q[48:] += np.float32(0.5)
    w = World(H, oracle, X, Q, H.METRIC_L2, ROWS_BYTES)
    yield w
    w.release()


@pytest.fixture(scope="module")
def w100(H, oracle):
    """d 100: split rows (400 bytes = three lines + 16 bytes)"""
    w = World(H, oracle, _floats(N, 100, 8), _floats(NQ, 100, 9), H.METRIC_L2, ROWS_SPLIT)
    yield w
    w.release()


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_rows(got, want, ctx):
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="%s [%d]" % (ctx, i))


def _both(H, w, mask, ef, k, fill, sem, flt=None):
    """the filtered call with the option off and on, on the same handle -> (off, on), each (ids, dist, ndist, nhops, stage)"""
    own = flt or w.hg.filter(mask)
    try:
        w.hg.set_option("filter_collect", 0)
        off = H._search_filtered(w.hg, own, w.Q, ef, k, fill, True, sem=sem)
        w.hg.set_option("filter_collect", 1)
        try:
            on = H._search_filtered(w.hg, own, w.Q, ef, k, fill, True, sem=sem)
        finally:
            w.hg.set_option("filter_collect", 0)
    finally:
        if flt is None:
            own.release()
    return off, on


def _check(H, w, mask, ef, k=K, fill=0, sem=0, ctx=""):
    """parity with the restatement for every query -> (stages, off, on)"""
    want = w.restate(mask, ef, k, fill)
    ladder = _ladder(ef)
    if mask.sum() >= k:                                          # every stage some query walked
        last = max(len(ladder) - 1 if st == EXACT else int(st) for st in want[2])
        for e in ladder[:last + 1]:
            w.self_check(e)
    off, on = _both(H, w, mask, ef, k, fill, sem)
    exact = want[2] == EXACT
    print("%s: stages with the option %s, without %s" % (ctx, dict(zip(*np.unique(want[2], return_counts=True))),
                                                           dict(zip(*np.unique(off[4], return_counts=True)))))
    np.testing.assert_array_equal(on[4], want[2], err_msg=ctx + " out_stage")
    ids = np.where(exact[:, None], off[0], want[0])              # (the exact stage is the unchanged one)
    dist = np.where(exact[:, None], off[1], want[1])
    np.testing.assert_array_equal(on[0], ids, err_msg=ctx + " ids")
    np.testing.assert_array_equal(on[1].view(np.uint32), dist.view(np.uint32), err_msg=ctx + " distance bits")
    assert (off[4][exact] == EXACT).all(), ctx                   # W is a subset of E: short with E, short with W
    real = on[0] >= 0
    assert mask[on[0][real]].all(), ctx
    if sem == 0:
        np.testing.assert_array_equal(on[3], want[3], err_msg=ctx + " out_nhops")
    assert (on[2] >= want[4]).all(), ctx + " out_ndist"
    if mask.sum() < k:
        assert (on[3] == 0).all() and (on[2] == mask.sum()).all(), ctx          # no walk
    return want[2], off, on


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ef", EFS)
def test_parity_d20(H, w20, ef):
    seen = set()
    for s in SELECTIVITIES:
        mask = _mask(s)
        for sem, fill in ((0, 0), (1, 1), (0, 1)) if s in (0.1, 0.003) else ((0, 0), (1, 1)):
            stages, off, on = _check(H, w20, mask, ef, K, fill, sem, "d 20 ef %d s %g rule %d fill %d" % (ef, s, sem, fill))
            seen |= set(np.where(stages == EXACT, -1, np.minimum(stages.astype(np.int64), 1)).tolist())
            if s == 1:
                assert (stages == 0).all()
            if s in (0.1, 0.03) and ef == 16:
                assert (on[4] < off[4]).any()                    # the option serves earlier what W alone could not
    assert seen == {0, 1, -1}, seen                              # served at stage 0, at a later stage, by the exact stage


@pytest.mark.parametrize("ef", [16, 128])
def test_parity_inner_product(H, w20ip, ef):
    negative = False
    for s in (0.5, 0.03, 0.003):
        for sem, fill in ((0, 0), (1, 1)):
            _, _, on = _check(H, w20ip, _mask(s), ef, K, fill, sem, "IP ef %d s %g rule %d" % (ef, s, sem))
            negative = negative or bool((on[1][on[0] >= 0] < 0).any())
    assert negative                                              # negative distances: the order-preserving key is exercised


@pytest.mark.parametrize("shape", ["w128", "wbytes", "w100"])
def test_parity_row_formats(H, request, shape):
    w = request.getfixturevalue(shape)
    for ef in (64, 200):
        for s in (0.5, 0.03, 0.003):
            for sem, fill in ((0, 0),) if shape == "wbytes" else ((0, 0), (1, 1)):     # (equal distances: the two rules differ there)
                _check(H, w, _mask(s), ef, K, fill, sem, "%s ef %d s %g rule %d" % (shape, ef, s, sem))


def test_tie_overflow_is_repaired(H, oracle):
    """More than 64 entries evicted from W while tied with max(W) and still unexpanded: the collect launch flags the query as the
    plain one does, and the re-run with the global slab, in collect mode too, rewrites its row -- a node evaluated only through
    such an entry (Z) is in R.  (The graph of tests/test_gpu_parity.py::test_tie_overflow_beyond_lds_stack.)"""
    n = 229
    pos = np.zeros(n, np.float32)                 # 1-D positions, the queries at 0: E far, 127 identical "shell" points at 10,
    pos[0] = 20.0                                 # a chain approaching, Z close
    pos[1:128] = 10.0
    pos[128:228] = 9.0 - 0.01 * np.arange(100)
    pos[228] = 0.1
    rows = [[] for _ in range(n)]
    rows[0] = [1] + list(range(2, 65))            # E -> H + 63 shells
    rows[1] = list(range(65, 128)) + [128]        # H -> 63 shells + head of the chain
    for i in range(99):
        rows[128 + i] = [129 + i]
    rows[40] = [228]                              # a shell evicted late is the only way to Z
    deg0 = np.array([len(r) for r in rows], np.int32)
    nbr0 = np.full((n, 64), -1, np.int32)
    for i, r in enumerate(rows):
        nbr0[i, :len(r)] = r
    X = pos[:, None]
    hg = H.Hgraph(X, deg0, nbr0, entry_point=0, max_degree=32)
    w = World(H, oracle, X, np.zeros((3, 1), np.float32), H.METRIC_L2, ROWS_F32, hg=hg)
    try:
        assert 228 in w.walk(0, 128)[2] and 228 in w.walk(0, 128)[0]
        mask = np.zeros(n, bool)
        mask[[5, 70, 228] + list(range(128, 141))] = True
        for order in (0, 1):
            hg.set_option("order_queries", order)
            stages, _, on = _check(H, w, mask, 128, K, 0, 0, "tie overflow, order_queries %d" % order)
            assert (stages == 0).all() and (on[0][:, 0] == 228).all()
    finally:
        w.release()


# ---- 2. k boundaries ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_k_boundaries(H, w20, wbytes, k):
    for w, name in ((w20, "d 20"), (wbytes, "bytes")):
        for s in (0.5, 0.1):
            stages, _, _ = _check(H, w, _mask(s), 128, k, 0, 0, "%s k %d s %g" % (name, k, s))
            assert (stages != EXACT).all()


def test_k_129_is_the_ladder_over_w(H, w20):
    for s in (0.5, 0.1):
        off, on = _both(H, w20, _mask(s), 200, 129, 0, 0)
        _same_rows(on, off, "k 129 s %g" % s)


# ---- 3. consistency ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["w20", "wbytes"])
def test_stage0_rows_are_the_same(H, request, shape):
    w = request.getfixturevalue(shape)
    checked = 0
    for ef, s in ((16, 0.5), (64, 0.5), (64, 0.1), (128, 0.1), (200, 0.03)):
        mask = _mask(s)
        off, on = _both(H, w, mask, ef, K, 0, 0)
        for q in np.flatnonzero(off[4] == 0):
            assert on[4][q] == 0
            checked += 1
            if (on[0][q] == off[0][q]).all():
                assert (on[1][q].view(np.uint32) == off[1][q].view(np.uint32)).all()
                continue
            # the one exception: a node outside the final W tied with max(W) at the k-th place, where (key, id) decides
            assert w.key[q][on[0][q][K - 1]] == w.key[q][off[0][q][K - 1]], "%s ef %d s %g query %d" % (shape, ef, s, q)
            assert shape == "wbytes"                             # continuous data has no such tie
            want = w.restate(mask, ef, K, 0)
            np.testing.assert_array_equal(on[0][q], want[0][q])
    assert checked > 64


def test_option_off_restores_the_results(H, w20):
    mask = _mask(0.1)
    flt = w20.hg.filter(mask)
    before = H._search_filtered(w20.hg, flt, w20.Q, 16, K, 0, True)
    off, on = _both(H, w20, mask, 16, K, 0, 0, flt=flt)
    after = H._search_filtered(w20.hg, flt, w20.Q, 16, K, 0, True)
    flt.release()
    _same_rows(off, before, "off")
    _same_rows(after, before, "after")
    assert (on[4] != before[4]).any()


# ---- 4. per-query filters ----------------------------------------------------------------------------------------------------------

def test_filtered_each_rows_are_the_single_filter_rows(H, w20):
    w = w20
    masks = [_mask(0.5), _mask(0.03), _mask(0.003), _mask(0.1, seed=21)]
    assert masks[2].sum() < K                                    # one filter allows fewer than k nodes: no walk for its queries
    filters = [w.hg.filter(m) for m in masks]
    which = (np.arange(NQ) % len(masks)).astype(np.int32)
    w.hg.set_option("filter_collect", 1)
    try:
        for ef, sem, fill in ((16, 0, 0), (64, 1, 1)):
            each = H._search_filtered_each(w.hg, filters, which, w.Q, ef, K, fill, True, sem=sem)
            for f in range(len(masks)):
                one = H._search_filtered(w.hg, filters[f], w.Q, ef, K, fill, True, sem=sem)
                sel = which == f
                _same_rows([a[sel] for a in each], [a[sel] for a in one], "ef %d filter %d" % (ef, f))
            if sem == 0:                                         # ... which are the definition's
                for f in (0, 1, 3):
                    want = w.restate(masks[f], ef, K, fill)
                    sel = (which == f) & (want[2] != EXACT)
                    np.testing.assert_array_equal(each[0][sel], want[0][sel])
                    np.testing.assert_array_equal(each[4][sel], want[2][sel])
            assert (each[4][which == 2] == EXACT).all() and (each[3][which == 2] == 0).all()
    finally:
        w.hg.set_option("filter_collect", 0)
        for f in filters:
            f.release()


# ---- 5. other entry points ---------------------------------------------------------------------------------------------------------

def np_merge(ids, dist, first_row, k_out, fill):
    """the sharded call's definition: per query the first k_out real entries of all shards' rows under (distance, global id)"""
    n_lists, nq, _ = ids.shape
    gid_all = np.asarray(first_row, np.int64)[:, None, None] + ids.astype(np.int64)
    out_i = np.full((nq, k_out), -1, np.int64)
    out_d = np.full((nq, k_out), _fill_value(fill), np.float32)
    for q in range(nq):
        real = ids[:, q, :] >= 0
        gid, dd = gid_all[:, q, :][real], dist[:, q, :][real]
        order = np.lexsort((gid, dd))[:k_out]
        out_i[q, :len(order)] = gid[order]
        out_d[q, :len(order)] = dd[order]
    return out_i, out_d


def test_plain_calls_under_marks(H, w20):
    w = w20
    hg = H.Hgraph(w.X, w.hg.deg0, w.hg.nbr0, w.hg.upper, entry_point=w.hg.entry_point, max_degree=w.hg.max_degree)   # the same graph, a handle of its own
    live = _mask(0.1)
    try:
        hg.mark_deleted(np.flatnonzero(~live))
        hg.set_option("filter_collect", 1)
        for ef in (16, 64):
            want = w.restate(live, ef, K, 0)
            plain = H._search(hg, w.Q, ef, K, H.FILL_OHNSW, True)
            filt = H._search_filtered(hg, np.ones(N, bool), w.Q, ef, K, H.FILL_OHNSW, True)   # (a current filter never allows a marked node: LIVE)
            _same_rows(plain, filt[:4], "marks ef %d" % ef)
            served = want[2] != EXACT
            np.testing.assert_array_equal(plain[0][served], want[0][served])
            np.testing.assert_array_equal(plain[1][served].view(np.uint32), want[1][served].view(np.uint32))
            np.testing.assert_array_equal(filt[4], want[2])
            for q in (0, 17, 63):                                # hnsw_knn
                one = H.Ohnsw.knn(hg, K, w.Q[q], ef=ef)
                assert [v for v, _ in one] == plain[0][q].tolist()
                assert np.array([d for _, d in one], np.float32).view(np.uint32).tolist() == plain[1][q].view(np.uint32).tolist()
        hg.set_option("filter_collect", 0)                       # (the option did something: W alone walks more stages)
        off = H._search(hg, w.Q, 64, K, H.FILL_OHNSW, True)
        assert (off[3] >= plain[3]).all() and (off[3] > plain[3]).any()
    finally:
        hg.release()


def test_sharded_filtered_call(H, w20):
    s = H.ShardedHgraph.build(w20.X, M, EFC, [0] * 3, seed=SEED)
    try:
        lo = [s.shard(g)[1] for g in range(3)] + [s.n]
        mask = _mask(0.1)
        before = s.knn_batch_filtered(w20.Q, 16, K, mask, counters=True)
        s.set_option("filter_collect", 1)
        for sem, fill in ((0, 0), (1, 1)):
            rows = [H._search_filtered(s.shard(g)[0], mask[lo[g]:lo[g + 1]], w20.Q, 16, K, fill, True, sem=sem) for g in range(3)]
            want = np_merge(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), lo[:-1], K, fill)
            got = s.knn_batch_filtered(w20.Q, 16, K, mask, fill=fill, sem=sem, counters=True)
            _same_rows(got, want + (sum(r[2] for r in rows), sum(r[3] for r in rows), np.stack([r[4] for r in rows]).max(axis=0)),
                       "sharded rule %d" % sem)
            if sem == 0:
                assert (got[4] < before[4]).any()                # the option reached the shards
        with pytest.raises(H.InvalidArgument):
            s.set_option("filter_collect", 2)
        s.set_option("filter_collect", 0)
        _same_rows(s.knn_batch_filtered(w20.Q, 16, K, mask, counters=True), before, "sharded, option off again")
    finally:
        s.release()


@pytest.mark.parametrize("option", ["order_queries", "visited_blocks"])
def test_launch_options_do_not_change_the_rows(H, w20, w128, option):
    for w, ef in ((w20, 16), (w128, 200)):
        mask = _mask(0.03)
        flt = w.hg.filter(mask)
        w.hg.set_option("filter_collect", 1)
        try:
            got = []
            for v in (0, 1):
                w.hg.set_option(option, v)
                got.append(H._search_filtered(w.hg, flt, w.Q, ef, K, 0, True))
            _same_rows(got[1], got[0], "%s 0 / 1, ef %d" % (option, ef))
        finally:
            w.hg.set_option(option, -1)
            w.hg.set_option("filter_collect", 0)
            flt.release()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(H, w20):
    w, L = w20, H.load()
    mask = _mask(0.1)
    flt = w.hg.filter(mask)
    off = H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True)
    try:
        for v in (2, -1):
            assert L.hnsw_index_set_option(w.hg.handle, b"filter_collect", v) == H.ERR_BAD_ARG
            _same_rows(H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True), off, "refused value %d" % v)     # still off
        w.hg.set_option("filter_collect", 1)
        on = H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True)
        assert (on[4] != off[4]).any()
        for v in (2, -1):
            assert L.hnsw_index_set_option(w.hg.handle, b"filter_collect", v) == H.ERR_BAD_ARG
            _same_rows(H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True), on, "refused value %d" % v)      # still on
        # the inexact rows are refused while it is on, the index unchanged ...
        for rows in ("half_rows", "sq8_rows"):
            assert L.hnsw_index_set_option(w.hg.handle, rows.encode(), 1) == H.ERR_BAD_ARG
            assert "filter_collect" in L.hnsw_last_error().decode()
            assert w.hg.info().row_format == ROWS_F32
            _same_rows(H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True), on, rows)
        # ... and it is refused while they are read
        w.hg.set_option("filter_collect", 0)
        for rows in ("half_rows", "sq8_rows"):
            w.hg.set_option(rows, 1)
            inexact = H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True)
            assert L.hnsw_index_set_option(w.hg.handle, b"filter_collect", 1) == H.ERR_BAD_ARG
            assert rows in L.hnsw_last_error().decode()
            _same_rows(H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True), inexact, rows + " read")
            w.hg.set_option(rows, -1)
        assert w.hg.info().row_format == ROWS_F32
        _same_rows(H._search_filtered(w.hg, flt, w.Q, 16, K, 0, True), off, "at the end")
    finally:
        for rows in ("half_rows", "sq8_rows"):
            w.hg.set_option(rows, -1)
        w.hg.set_option("filter_collect", 0)
        flt.release()
