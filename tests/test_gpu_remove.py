"""hnsw_index_remove (hard deletion, ocaml-hnsw_amd/csrc/hnsw_remove.hip): the repaired graph equals, link for link and in row
order, the graph the header's definition gives -- NUMBERING, PROPOSE, OFFER, AGREE restated here from Hgraph.export() before the
call and from public calls only (hnsw_select_neighbours_batch with cand_degree, hnsw_distance_batch, numpy); everything the
handle derives from its graph follows it; every refusal leaves the index as it was; filters made before are refused."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
from conftest import ROOT
from device_bytes import expected as expected_bytes

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8 = 0, 2, 3, 4, 5
M, EFC = 8, 64


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
    X = rng.normal(size=(n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


# ---- the definition, restated ------------------------------------------------------------------------------------------------

def _layers(hg):
    """[(cap, {node: row})] per layer, 0-based ids, rows in row order"""
    b = hg.id_base
    out = [(hg.max_degree0, {v: (hg.nbr0[v, :hg.deg0[v]] - b).tolist() for v in range(hg.n)})]
    for nodes, deg, nbr in hg.upper:
        out.append((hg.max_degree, {int(v) - b: (nbr[s, :deg[s]] - b).tolist() for s, v in enumerate(nodes)}))
    return out


class Want:
    """the graph hnsw_index_remove must leave, from the exported graph `hg` (still on the device: the operators run on it), its
    vectors X and the removed 0-based ids"""

    def __init__(self, H, hg, X, dead):
        b, n = hg.id_base, hg.n
        deadm = np.zeros(n, bool)
        deadm[np.asarray(sorted(dead), np.int64)] = True
        self.new_id = np.where(deadm, -1, np.cumsum(~deadm) - 1).astype(np.int64)       # NUMBERING
        self.n = int((~deadm).sum())
        self.touched, self.rows = [], []
        for cap, rows in _layers(hg):
            touched = [u for u in sorted(rows) if not deadm[u] and any(deadm[w] for w in rows[u])]
            live, C = {}, {}
            for u in touched:
                lv = [w for w in rows[u] if not deadm[w]]
                seen, c = set(lv) | {u}, []
                for r in rows[u]:
                    if not deadm[r]:
                        continue
                    for w in rows[r]:
                        if len(lv) + len(c) >= 1024:                    # the stop
                            break
                        if deadm[w] or w in seen:
                            continue
                        seen.add(w)
                        c.append(w)
                live[u], C[u] = lv, c
            S = {}
            if touched:                                                 # PROPOSE
                sel = H.Ohnsw.select_neighbours(hg, X[touched], [[w + b for w in live[u] + C[u]] for u in touched], cap,
                                                keep_all_if_few=False, degrees=[[0] * len(live[u]) + [2] * len(C[u]) for u in touched])
                for u, s in zip(touched, sel):
                    assert [w - b for w in s[:len(live[u])]] == live[u]  # the forced entries, kept in order
                    S[u] = [w - b for w in s[len(live[u]):]]
            U = {u: list(S[u]) for u in touched}                        # OFFER
            for w in touched:
                for u in S[w]:
                    if u in U and w not in live[u] and w not in S[u]:
                        U[u].append(w)
            T = {}
            if touched:
                width = max(max(len(U[u]) for u in touched), 1)
                ids = np.full((len(touched), width), b, np.int32)
                for i, u in enumerate(touched):
                    ids[i, :len(U[u])] = np.asarray(U[u], np.int32) + b
                dist = H.Ohnsw.distance_l2(hg, X[touched], ids)
                for i, u in enumerate(touched):
                    order = sorted(range(len(U[u])), key=lambda j: (dist[i, j], U[u][j]))
                    T[u] = [U[u][j] for j in order][:cap - len(live[u])]
            new_rows = {}
            for u in rows:
                if deadm[u]:
                    continue
                row = [w for w in rows[u] if not deadm[w]]
                if u in T:
                    row += [w for w in T[u] if w in T and u in T[w]]    # AGREE
                assert len(row) <= cap
                new_rows[int(self.new_id[u])] = [int(self.new_id[w]) for w in row]
            self.touched.append(touched)
            self.rows.append((cap, new_rows))
        while len(self.rows) > 1 and not self.rows[-1][1]:              # LEVELS, TOP, ENTRY
            self.rows.pop()
        self.max_layer = len(self.rows) - 1 if self.n else 0
        old_entry = None if hg.entry_point is None else hg.entry_point - b
        if self.n == 0:
            self.entry = None
        elif old_entry is not None and not deadm[old_entry]:
            self.entry = int(self.new_id[old_entry])
        else:
            self.entry = min(self.rows[self.max_layer][1])
        self.base = b

    def check(self, hg, new_id):
        """hg: the handle after the call, exported"""
        b = self.base
        np.testing.assert_array_equal(new_id, np.where(self.new_id >= 0, self.new_id + b, b - 1))
        assert new_id.dtype == np.int32
        assert hg.n == self.n and hg.info().n == self.n
        assert hg.entry_point == (None if self.entry is None else self.entry + b)
        assert hg.max_layer == self.max_layer
        cap0, rows0 = self.rows[0]
        assert hg.nbr0.shape == (self.n, cap0)
        for v in range(self.n):
            assert (hg.nbr0[v, :hg.deg0[v]] - b).tolist() == rows0[v], ("layer 0", v)
            assert (hg.nbr0[v, hg.deg0[v]:] == -1).all()
        assert len(hg.upper) == self.max_layer
        for l, (nodes, deg, nbr) in enumerate(hg.upper, 1):
            cap, rows = self.rows[l]
            assert (nodes - b).tolist() == sorted(rows), ("layer", l)
            for s, v in enumerate(nodes):
                assert (nbr[s, :deg[s]] - b).tolist() == rows[int(v) - b], ("layer", l, int(v))


def _invariants(before, after, new_id, symmetric=True):
    """no removed id, no self link, no duplicate, degrees within the caps, every live link kept (as the row's prefix, in order),
    a symmetric graph still symmetric.  before / after: exported graphs; new_id as returned (id_base-based)."""
    b = after.id_base
    assert (new_id[new_id >= b] == np.arange(after.n) + b).all()
    old_layers, new_layers = _layers(before), _layers(after)
    for l, (cap, rows) in enumerate(new_layers):
        for v, row in rows.items():
            assert len(row) <= cap and len(set(row)) == len(row) and v not in row, (l, v)
            assert all(0 <= w < after.n and w in rows for w in row), (l, v)
            if symmetric:
                assert all(v in rows[w] for w in row), (l, v)
    for l, (_, rows) in enumerate(old_layers):
        for u, row in rows.items():
            if new_id[u] < b:
                continue
            kept = [int(new_id[w]) - b for w in row if new_id[w] >= b]
            got = new_layers[l][1][int(new_id[u]) - b] if l < len(new_layers) else []
            assert got[:len(kept)] == kept, (l, u)


def _shift(hg, X, base, metric, H):
    """the exported graph `hg` (id_base 0) as a new index with ids from `base`, made through hnsw_index_create"""
    sh = lambda a: np.where(a >= 0, a + base, -1).astype(np.int32)
    return H.Hgraph(X, hg.deg0.copy(), sh(hg.nbr0), [(nodes + base, deg.copy(), sh(nbr)) for nodes, deg, nbr in hg.upper],
                    entry_point=hg.entry_point + base, id_base=base, max_degree=hg.max_degree, metric=metric)


_built = {}


def _base_graph(H, d, metric):
    """the base shape, built once per (d, metric): (X, exported graph)"""
    if (d, metric) not in _built:
        X = _data("unit" if metric else "uniform", 600, d, seed=20 + d)
        _built[(d, metric)] = (X, H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=3, metric=metric).export())
    return _built[(d, metric)]


def _removal_set(kind, hg):
    """0-based ids"""
    n = hg.n
    rng = np.random.default_rng(5)
    if kind == "one":
        return [n // 2]
    if kind == "random20":
        return rng.choice(n, size=n // 5, replace=False).tolist()
    if kind == "block":
        return list(range(n // 3, n // 3 + n // 6))
    if kind == "entry":
        return [hg.entry_point - hg.id_base]
    if kind == "top":
        return (hg.upper[-1][0] - hg.id_base).tolist()
    if kind == "all_but_three":
        keep = set(rng.choice(n, size=3, replace=False).tolist())
        return [v for v in range(n) if v not in keep]
    raise ValueError(kind)


# ---- 1. link-for-link equality on built graphs -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["one", "random20", "block", "entry", "top", "all_but_three"])
@pytest.mark.parametrize("d,metric,base", [(16, 0, 0), (16, 1, 1), (16, 0, 1), (100, 0, 1), (100, 1, 0), (130, 0, 0), (130, 1, 1)])
def test_repaired_graph_equals_the_definition_link_for_link(H, d, metric, base, kind):
    X, g0 = _base_graph(H, d, metric)
    assert g0.max_layer >= 1
    hg = _shift(g0, X, base, metric, H).to_device().export()
    before = _shift(g0, X, base, metric, H)                             # a host copy that stays as it was
    dead = _removal_set(kind, hg)
    want = Want(H, hg, X, dead)
    assert len(want.touched[0]) > 0
    new_id = H.Ohnsw.remove_batch(hg, np.asarray(dead, np.int64) + base)
    assert hg.deg0 is None and hg.vectors.shape == (600 - len(dead), d)
    np.testing.assert_array_equal(hg.vectors, X[new_id >= base])
    hg.export()
    want.check(hg, new_id)
    if kind == "top":
        assert hg.max_layer < g0.max_layer
    if kind == "entry":
        assert new_id[g0.entry_point] == base - 1 and hg.entry_point == want.entry + base
    _invariants(before, hg, new_id)
    hg.release()


# ---- 2. hand-made graphs through hnsw_index_create -------------------------------------------------------------------------------

def _from_lists(H, X, rows, cap, entry=0):
    n = len(rows)
    deg0 = np.array([len(r) for r in rows], np.int32)
    nbr0 = np.full((n, cap), -1, np.int32)
    for v, r in enumerate(rows):
        nbr0[v, :len(r)] = r
    return H.Hgraph(X, deg0, nbr0, entry_point=entry, id_base=0, max_degree=max(1, cap // 2))


def test_a_hub_crosses_the_candidate_stop(H):
    """node 0 has 20 removed neighbours (1..20), each listing 60 live nodes of its own: 1200 distinct live candidates, so the walk
    over the removed neighbours' rows stops at |live(u)| + |C(u)| = 1024; the links are symmetric"""
    n = 1 + 20 + 1200 + 2
    X = _data("uniform", n, 8, seed=31)
    rows = [[] for _ in range(n)]
    rows[0] = [1221] + list(range(1, 21)) + [1222]                      # live entries before and after the removed ones
    rows[1221], rows[1222] = [0], [0]
    for r in range(1, 21):
        mine = list(range(21 + 60 * (r - 1), 21 + 60 * r))
        rows[r] = mine[:30] + [0] + mine[30:]
        for w in mine:
            rows[w] = [r]
    hg = _from_lists(H, X, rows, 64).to_device().export()
    before = _from_lists(H, X, rows, 64)
    dead = list(range(1, 21))
    want = Want(H, hg, X, dead)
    assert 0 in want.touched[0] and len(want.touched[0]) == 1201
    new_id = H.Ohnsw.remove_batch(hg, dead)
    hg.export()
    want.check(hg, new_id)
    _invariants(before, hg, new_id)
    assert hg.deg0[0] > 2                                               # the hub found new neighbours
    hg.release()


def test_an_asymmetric_graph_is_repaired_by_the_same_rule(H):
    n, cap = 300, 8
    rng = np.random.default_rng(32)
    X = _data("uniform", n, 12, seed=33)
    rows = [rng.choice([w for w in range(n) if w != v], size=int(rng.integers(1, 7)), replace=False).tolist() for v in range(n)]
    hg = _from_lists(H, X, rows, cap).to_device().export()
    before = _from_lists(H, X, rows, cap)
    dead = rng.choice(np.arange(1, n), size=90, replace=False).tolist()
    want = Want(H, hg, X, dead)
    new_id = H.Ohnsw.remove_batch(hg, dead)
    hg.export()
    want.check(hg, new_id)
    _invariants(before, hg, new_id, symmetric=False)
    hg.release()


def test_a_node_whose_neighbours_all_die_is_left_isolated(H):
    """a ring of 40 nodes and, apart from it, the pair 40 - 41: node 41 leaves and node 40 keeps no link"""
    n = 42
    X = np.zeros((n, 4), np.float32)
    X[:, 0] = np.arange(n)                                              # on a line: 6 and 8 are nearer to each other than to 5 and 9
    rows = [[(v - 1) % 40, (v + 1) % 40] for v in range(40)] + [[41], [40]]
    hg = _from_lists(H, X, rows, 4).to_device().export()
    want = Want(H, hg, X, [41, 7])
    new_id = H.Ohnsw.remove_batch(hg, [41, 7])
    hg.export()
    want.check(hg, new_id)
    assert new_id[40] == 39 and hg.deg0[39] == 0
    assert hg.stats()["layer_connectivity"][0]["isolated"] == [39]
    assert hg.nbr0[6, :hg.deg0[6]].tolist() == [5, 7] and hg.nbr0[7, :hg.deg0[7]].tolist() == [8, 6]     # 6 - 8 linked (8 is now 7)
    hg.release()


# ---- 3. invariants at a larger size --------------------------------------------------------------------------------------------

def test_invariants_after_a_large_removal(H):
    X = _data("uniform", 4000, 16, seed=35)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=4).export()
    before = _shift(hg, X, 0, 0, H)
    dead = np.random.default_rng(36).choice(4000, size=1600, replace=False)
    new_id = H.Ohnsw.remove_batch(hg, dead)
    hg.export()
    assert hg.n == 2400
    _invariants(before, hg, new_id)
    for l in range(hg.max_layer + 1):
        assert hg.stats()["layer_connectivity"][l]["max"] <= (2 * M if l == 0 else M)
    hg.release()


# ---- 4. the tables agree with the graph ----------------------------------------------------------------------------------------

def _oracle_graph(oracle, hg):
    return oracle.Graph(hg.n, hg.entry_point - hg.id_base, hg.deg0, np.where(hg.nbr0 >= 0, hg.nbr0 - hg.id_base, -1),
                        [(nodes - hg.id_base, deg, np.where(nbr >= 0, nbr - hg.id_base, -1)) for nodes, deg, nbr in hg.upper])


def _queries(X, nq, seed):
    rng = np.random.default_rng(seed)
    return (X[rng.integers(0, len(X), nq)] + rng.integers(0, 2, size=(nq, X.shape[1]))).astype(np.float32)


def _half(X):
    return np.asarray(X, np.float32).astype(np.float16).astype(np.float32)


def _quantise(X):
    """the sq8 quantiser (include/hnsw_mi355x.h, option "sq8_rows"): float32 operations, round to nearest even"""
    X = np.asarray(X, np.float32)
    zero = np.float32(0)
    lo, hi = np.float32(X.min()) + zero, np.float32(X.max()) + zero
    s = np.float32(1) if hi == lo else np.float32(np.float32(hi - lo) / np.float32(255))
    return np.minimum(np.float32(255), np.maximum(zero, np.rint((X - lo) / s))).astype(np.uint8), lo, s


def _check_walk(H, oracle, hg, Xwalk, Q, efs=(32, 200), k=10):
    """ids, distance bits and hops of the device search == the oracle's search over the exported graph and the rows Xwalk"""
    g = _oracle_graph(oracle, hg)
    sp = oracle.Space.l2(Xwalk, arith=oracle.TREE16)
    for ef in efs:
        ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, k, Q, ef=ef, counters=True)
        oi, od, ond, onh = oracle.Ohnsw.knn_batch_bigarray(g, sp, Q, k=k, ef=ef, ties=oracle.TIES_CANONICAL, counters=True)
        np.testing.assert_array_equal(ids, oi, err_msg="ef %d" % ef)
        np.testing.assert_array_equal(dist.view(np.uint32), od.view(np.uint32), err_msg="ef %d" % ef)
        np.testing.assert_array_equal(nh, onh, err_msg="ef %d" % ef)


@pytest.mark.parametrize("case", ["f32", "bytes", "split", "half", "sq8"])
def test_search_after_a_removal_matches_the_oracle(H, oracle, case):
    n, d = 1500, {"bytes": 6, "split": 100}.get(case, 24)
    X = _data("levels" if case == "bytes" else "uniform", n, d, seed=40)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=6)
    if case in ("half", "sq8"):
        hg.set_option(case + "_rows", 1)
    fmt = {"f32": ROWS_F32, "bytes": ROWS_BYTES, "split": ROWS_SPLIT, "half": ROWS_HALF, "sq8": ROWS_SQ8}[case]
    assert hg.info().row_format == fmt
    dead = np.random.default_rng(41).choice(n, size=n // 4, replace=False)
    if case == "sq8":
        dead = np.union1d(dead, [int(X.min(axis=1).argmin()), int(X.max(axis=1).argmax())])       # the range's ends leave: lo and scale change
    new_id = H.Ohnsw.remove_batch(hg, dead)
    live = new_id >= 0
    Xl = X[live]
    hg.export()
    assert hg.n == len(Xl) and hg.info().row_format == fmt
    Q = _queries(Xl, 100, 42)
    fresh = H.Hgraph(Xl, hg.deg0, hg.nbr0, hg.upper, entry_point=hg.entry_point, max_degree=hg.max_degree)
    if case in ("f32", "bytes", "split"):
        assert hg.info().device_bytes == expected_bytes(hg, d)
        _check_walk(H, oracle, hg, Xl, Q)
    elif case == "half":
        _check_walk(H, oracle, hg, _half(Xl), Q)
    else:
        # the codes are those of a fresh index over X[live]; the walk runs over them in code space (k members of W), which are
        # then ordered by (float32 distance key, id) over X[live]
        fresh.set_option("sq8_rows", 1)
        B, lo, s = _quantise(Xl)
        assert hg.sq8_params() == fresh.sq8_params() == (lo, s)
        assert hg.sq8_params() != _quantise(X)[1:]
        np.testing.assert_array_equal(hg.sq8_codes(), B)
        g = _oracle_graph(oracle, hg)
        sp = oracle.Space.l2(B.astype(np.float32), arith=oracle.TREE16)
        for ef in (32, 200):
            ids, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=ef, counters=True)
            W, _, _, hops = oracle.Ohnsw.knn_batch_bigarray(g, sp, ((Q - lo) / s).astype(np.float32), k=10, ef=ef, ties=oracle.TIES_CANONICAL,
                                                            counters=True)
            np.testing.assert_array_equal(nh, hops)
            for q in range(len(Q)):
                w = W[q][W[q] >= 0].astype(np.int64)
                sq = np.array([oracle.l2sq_tree16(Xl[j], Q[q]) for j in w], np.float32)
                o = np.lexsort((w, sq))
                np.testing.assert_array_equal(ids[q, :len(o)], w[o])
                np.testing.assert_array_equal(dist[q, :len(o)].view(np.uint32), np.sqrt(sq[o].astype(np.float64)).astype(np.float32).view(np.uint32))
    # the exact scan reads the shrunk table
    for a, b in zip(H.Ohnsw.brute_force_knn(hg, 10, Q), H.Ohnsw.brute_force_knn(fresh, 10, Q)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    fresh.release()
    hg.release()


def test_byte_rows_appear_when_only_byte_valued_vectors_are_left(H, oracle):
    X = _data("levels", 800, 6, seed=43)
    X[::4] += np.float32(0.5)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=6)
    assert hg.info().row_format == ROWS_F32
    new_id = H.Ohnsw.remove_batch(hg, np.arange(0, 800, 4))
    hg.export()
    assert hg.info().row_format == ROWS_BYTES and hg.info().device_bytes == expected_bytes(hg, 6)
    _check_walk(H, oracle, hg, X[new_id >= 0], _queries(X[new_id >= 0], 50, 44), efs=(64,))
    hg.release()


# ---- 5. insert after remove, save / load ---------------------------------------------------------------------------------------

def _same_export(a, b):
    assert (a.entry_point, a.max_layer, a.n) == (b.entry_point, b.max_layer, b.n)
    np.testing.assert_array_equal(a.deg0, b.deg0)
    np.testing.assert_array_equal(a.nbr0, b.nbr0)
    assert len(a.upper) == len(b.upper)
    for u, v in zip(a.upper, b.upper):
        for x, y in zip(u, v):
            np.testing.assert_array_equal(x, y)


def _graph_invariants(hg, m):
    """Graph.Test.invariant (lib/ohnsw.ml:217-225) and the degree caps, as tests/test_gpu_insert.py holds a grown index to"""
    for l, (cap, rows) in enumerate(_layers(hg)):
        assert cap <= (2 * m if l == 0 else m)
        for v, row in rows.items():
            assert len(set(row)) == len(row) and v not in row
            assert all(v in rows[w] for w in row), (l, v)


def test_insert_after_remove_and_save_load(H, oracle):
    X = _data("uniform", 2000, 16, seed=45)
    hg = H.Ohnsw.build_batch_bigarray(X[:1500], M, EFC, seed=7)
    new_id = H.Ohnsw.remove_batch(hg, np.random.default_rng(46).choice(1500, size=400, replace=False))
    with tempfile.TemporaryDirectory() as tmp:                          # save / load round-trips the repaired graph
        path = os.path.join(tmp, "shrunk.hnsw")
        hg.save(path)
        again = H.Hgraph.load(path)
    _same_export(again.export(), hg.export())
    again.release()
    ids = H.Ohnsw.insert_batch(hg, X[1500:], M, EFC, seed=7)
    np.testing.assert_array_equal(ids, np.arange(1100, 1600))           # numbering continues from the shrunk n
    hg.export()
    assert hg.n == 1600
    _graph_invariants(hg, M)
    Xn = np.concatenate([X[:1500][new_id >= 0], X[1500:]])
    np.testing.assert_array_equal(hg.vectors, Xn)
    _check_walk(H, oracle, hg, Xn, _queries(Xn, 60, 47), efs=(64,))
    hg.release()


def test_remove_everything_then_insert_equals_a_build(H):
    X = _data("uniform", 1200, 16, seed=48)
    full = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=8).export()
    hg = H.Ohnsw.build_batch_bigarray(X[:300], M, EFC, seed=8)
    new_id = H.Ohnsw.remove_batch(hg, np.arange(300))
    assert (new_id == -1).all() and hg.n == 0 and hg.info().n == 0 and hg.entry_point is None
    with pytest.raises(H.InvalidArgument):                              # HNSW_ERR_EMPTY_INDEX
        H.Ohnsw.knn_batch_bigarray(hg, 5, X[:3], ef=16)
    H.Ohnsw.insert_batch(hg, X, M, EFC, seed=8)
    _same_export(hg.export(), full)
    hg.release()
    full.release()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_index_untouched(H):
    X = _data("uniform", 900, 16, seed=49)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=9).export()
    snap = _shift(hg, X, 0, 0, H)
    Q = _queries(X, 40, 50)
    state = lambda: tuple(getattr(hg.info(), f) for f in ("n", "entry_point", "max_layer", "device_bytes", "max_degree0", "row_format"))
    before, bits = state(), H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64, counters=True)
    L = H.load()
    out = np.full(900, 77, np.int32)

    def raw(ids, m=None, handle=None):
        ids = np.asarray(ids, np.int64)
        return L.hnsw_index_remove(hg.handle if handle is None else handle, ids.ctypes.data_as(ctypes.c_void_p), len(ids) if m is None else m,
                                   out.ctypes.data_as(ctypes.c_void_p))

    for ids, m, msg in (([3, 5, 3], None, "twice"), ([3, 900], None, "not a stored node"), ([-1], None, "not a stored node"), ([1], -1, "m=-1")):
        assert raw(ids, m) == H.ERR_BAD_ARG and msg in L.hnsw_last_error().decode(), msg
    assert L.hnsw_index_remove(hg.handle, None, 2, None) == H.ERR_BAD_ARG
    req = H.submit(hg, Q, 64, 10)                                       # a pending request
    assert raw([1, 2]) == H.ERR_BAD_ARG and "submitted" in L.hnsw_last_error().decode()
    req.wait()
    assert (out == 77).all()
    multi = H.MultiHgraph(hg, [0])                                      # a replica of an hnsw_multi
    rep = ctypes.c_void_p()
    assert L.hnsw_multi_replica(multi._h, 0, ctypes.byref(rep)) == H.OK
    assert raw([1, 2], handle=rep) == H.ERR_BAD_ARG and "replica" in L.hnsw_last_error().decode()
    np.testing.assert_array_equal(multi.knn_batch_bigarray(10, Q, ef=64)[0], bits[0])
    multi.release()
    # a graph that lists a node on a layer it is not on
    bad = _shift(snap, X, 0, 0, H)
    nodes, deg, nbr = bad.upper[0]
    outsider = next(v for v in range(900) if v not in set(nodes.tolist()))
    nbr[0, 0], deg[0] = outsider, max(deg[0], 1)
    assert L.hnsw_index_remove(bad.handle, np.array([5], np.int64).ctypes.data_as(ctypes.c_void_p), 1, None) == H.ERR_BAD_ARG
    assert "not on" in L.hnsw_last_error().decode() and bad.info().n == 900
    bad.release()
    # every refusal: same graph, same info, same bits
    hg.export()
    _same_export(hg, snap)
    assert state() == before
    for a, b in zip(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=64, counters=True), bits):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # m == 0 is a no-op that fills the identity
    assert raw([], 0) == H.OK and (out == np.arange(900)).all() and state() == before
    np.testing.assert_array_equal(H.Ohnsw.remove_batch(hg, []), np.arange(900))
    assert len(H.Ohnsw.remove_batch(hg, [899])) == 900 and hg.info().n == 899
    hg.release()


# ---- 7. stale filters ------------------------------------------------------------------------------------------------------------

def test_filters_made_before_the_graph_changed_are_refused(H):
    X = _data("uniform", 800, 16, seed=51)
    hg = H.Ohnsw.build_batch_bigarray(X[:700], M, EFC, seed=10)
    Q = _queries(X, 20, 52)
    f0 = hg.filter(np.arange(700) % 2 == 0)
    H.Ohnsw.knn_batch_filtered(hg, 5, Q, f0, ef=32)
    H.Ohnsw.remove_batch(hg, [1, 2, 3, 4, 5])
    with pytest.raises(H.InvalidArgument, match="filter"):              # made before a removal
        H.Ohnsw.knn_batch_filtered(hg, 5, Q, f0, ef=32)
    f1 = hg.filter(np.arange(695) % 2 == 0)
    ids = H.Ohnsw.knn_batch_filtered(hg, 5, Q, f1, ef=32)[0]
    assert (ids % 2 == 0).all()
    H.Ohnsw.remove_batch(hg, [10, 11, 12, 13, 14])
    H.Ohnsw.insert_batch(hg, X[700:705], M, EFC, seed=10)
    assert hg.info().n == 695                                           # remove 5, insert 5: the same n, another graph
    with pytest.raises(H.InvalidArgument, match="stale"):
        H.Ohnsw.knn_batch_filtered(hg, 5, Q, f1, ef=32)
    f2 = hg.filter(np.arange(695) % 2 == 1)
    ids = H.Ohnsw.knn_batch_filtered(hg, 5, Q, f2, ef=32)[0]
    assert (ids % 2 == 1).all()
    for f in (f0, f1, f2):
        f.release()
    hg.release()


# ---- 8. quality ------------------------------------------------------------------------------------------------------------------

def test_recall_after_a_removal_against_rebuilds(H):
    """Uniform data, n 3000, d 16, M 8, efConstruction 64, a random 20 % removed: recall@10 at ef 32 of 300 queries against the
    exact scan of the shrunk index.  The reference: hnsw_build over X[live] with seeds 1..5.  The repaired index must reach
    min(reference) - margin, margin = the reference's own spread (max - min) but at least 0.002 (six of the 3000 (query, neighbour)
    pairs: the resolution of the measurement)."""
    n, d, nq, k, ef = 3000, 16, 300, 10, 32
    rng = np.random.default_rng(60)
    X = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    Q = rng.uniform(-1, 1, size=(nq, d)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=1)
    new_id = H.Ohnsw.remove_batch(hg, rng.choice(n, size=n // 5, replace=False))
    Xl = X[new_id >= 0]
    truth = H.Ohnsw.brute_force_knn(hg, k, Q)[0]

    def recall(g):
        ids = H.Ohnsw.knn_batch_bigarray(g, k, Q, ef=ef)[0]
        return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / float(nq * k)

    got = recall(hg)
    ref = []
    for seed in (1, 2, 3, 4, 5):
        g = H.Ohnsw.build_batch_bigarray(Xl, M, EFC, seed=seed)
        ref.append(recall(g))
        g.release()
    margin = max(max(ref) - min(ref), 0.002)
    print("recall@10 ef 32 after removing 20 %%: repaired %.4f; rebuilt, seeds 1..5: %s; floor %.4f"
          % (got, " ".join("%.4f" % r for r in ref), min(ref) - margin))
    assert got >= min(ref) - margin, (got, ref)
    hg.release()


# ---- 9. the C++ front end ------------------------------------------------------------------------------------------------------

def test_cpp_front_end_remove(H, tmp_path):
    exe = str(tmp_path / "test_front_remove")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_remove.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "remove front-end ok" in out.stdout, out.stdout + out.stderr
