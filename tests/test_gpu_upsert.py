"""hnsw_index_upsert_keyed / hnsw_index_update (ocaml-hnsw_amd/csrc/hnsw_upsert.hip) against THE DEFINITION: two twin handles are built
from the same data and seed; handle A gets the one call, handle B gets remove_keys(P) followed by insert_batch_keyed(all), P being the
call's keys that are stored.  Afterwards the two must be equal bit for bit: the exported graph on every layer, the stored rows, the
keys, the info, the marks, every derived row copy with its parameters, the keyed search (ids as keys, distances, both counters) and the
exact scan.  The atomicity tests snapshot one handle, make calls that must be refused, and ask for the snapshot again -- with a filter
made BEFORE the refused call still accepted, which proves that the epoch did not move.

The base shape is n 3000, d 24, L2, M 8, efC 48, default batching: several build batches, an upper layer, touched rows on layer 1.
Keys are a random permutation of spread-out int64 values, negatives included.

The level law (splitmix64, hnsw_build.hip: node i draws the mix of seed + i * 0x9E3779B97F4A7C15, level = round(-ln(u) / ln M)) is
evaluated on the CPU below: with seed 113 and M 8 the positions 0..2999 draw levels up to 3 and position 3131 draws 4, so an upsert
of 250 stored + 150 new keys (new positions 2750..3149) holds a node that raises max_layer and ends its batch (row 381 of the call)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M, EFC = 3000, 24, 8, 48
NQ, EF, K = 64, 32, 10
SEED = 5
RAISING_SEED, RAISING_POSITION = 113, 3131
MISSING = -(2 ** 62) - 12345


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _keys(n, seed):
    """n distinct spread-out int64 keys, about half of them negative, in a random order"""
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(-2 ** 62, 2 ** 62, size=2 * n + 16, dtype=np.int64))
    k = k[k != MISSING]
    assert len(k) >= n
    k = k[rng.permutation(len(k))[:n]]
    assert (k < 0).any() and (k > 0).any()
    return k


def levels(seed, lo, hi, m):
    """the documented level law for positions [lo, hi)"""
    g = np.uint64(0x9E3779B97F4A7C15)
    i = np.arange(lo, hi, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + i * g
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    lv = np.minimum(np.floor(-np.log(u) * (1.0 / math.log(m)) + 0.5).astype(np.int64), 15)
    lv[i == 0] = 0
    return lv


def setup_module(module):
    old, new = levels(RAISING_SEED, 0, N, M), levels(RAISING_SEED, N, N + 150, M)
    assert new.max() > old.max() and N + int(new.argmax()) == RAISING_POSITION, (old.max(), new.max(), int(new.argmax()))


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.keys = _keys(N + 1000, 3)                 # [:N] stored, [N:] fresh keys for new rows
    w.new = _floats(1000, D, 4)                 # replacement and new vectors
    return w


def _twins(H, X, keys, seed=SEED, metric=None, m=M, efc=EFC, keyed=True):
    out = []
    for _ in range(2):
        hg = H.Ohnsw.build_batch_bigarray(X, m, efc, seed=seed, **({} if metric is None else {"metric": metric}))
        if keyed:
            hg.set_keys(keys)
        out.append(hg)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _snapshot(H, hg, Q, keyed=True, searches=True):
    """everything the definition names, as a dict of arrays"""
    inf = hg.info()
    s = {"info": np.array([inf.n, inf.max_degree, inf.max_degree0, inf.max_layer, inf.entry_point, inf.row_format, inf.metric, inf.id_base], np.int64)}
    hg._adopt(inf)
    hg.export()
    s["deg0"], s["nbr0"] = hg.deg0.copy(), hg.nbr0.copy()
    s["n_upper"] = np.array([len(hg.upper)])
    for l, (nodes, deg, nbr) in enumerate(hg.upper):
        s["up%d_nodes" % l], s["up%d_deg" % l], s["up%d_nbr" % l] = nodes.copy(), deg.copy(), nbr.copy()
    s["rows"] = _bits(hg.rows())
    if keyed:
        s["keys"] = hg.keys()
    s["deleted"] = hg.deleted_mask()
    s["n_deleted"] = np.array([hg.deleted_count()])
    if searches and inf.n > 0:
        if keyed:
            kk, dist, nd, nh, stage = H.Ohnsw.knn_batch_keyed(hg, K, Q, ef=EF, counters=True, missing=MISSING)
            s["s_keys"], s["s_stage"] = kk, stage
        else:
            kk, dist, nd, nh = H.Ohnsw.knn_batch_bigarray(hg, K, Q, ef=EF, counters=True)
            s["s_ids"] = kk
        s["s_dist"], s["s_nd"], s["s_nh"] = _bits(dist), nd, nh
        bi, bd = H.Ohnsw.brute_force_knn(hg, K, Q)
        s["bf_ids"], s["bf_dist"] = bi, _bits(bd)
    return s


def _same(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def _by_definition(H, A, B, X, keys, Q, seed=SEED, **build):
    """A gets the one call, B the two; outputs checked against find_keys before and B's removal -> nothing; then A == B"""
    base = A.id_base
    found = A.find_keys(keys)
    stored = found >= base
    n_old = A.n
    replaced, new_id = H.Ohnsw.upsert_batch_keyed(A, X, keys, M, EFC, seed=seed, **build)
    np.testing.assert_array_equal(replaced, stored)
    assert new_id.shape == (n_old,) and new_id.dtype == np.int32
    b_new_id = B.remove_keys(keys[stored])
    np.testing.assert_array_equal(new_id, b_new_id)
    dead = np.zeros(n_old, bool)
    dead[found[stored] - base] = True
    assert (new_id[dead] == base - 1).all() and (new_id[~dead] == base + np.arange(n_old - dead.sum())).all()
    first = H.Ohnsw.insert_batch_keyed(B, X, keys, M, EFC, seed=seed, **build)
    assert A.info().n == n_old - stored.sum() + len(keys)
    if len(keys):
        assert first[0] == n_old - stored.sum() + base
        # the new nodes take the ids behind the kept ones, in the call's row order
        np.testing.assert_array_equal(A.find_keys(keys), base + n_old - stored.sum() + np.arange(len(keys)))
    _same(_snapshot(H, A, Q), _snapshot(H, B, Q))


def _mixed_call(w, n, n_stored, n_new, seed):
    """n_stored stored keys scattered through a call of n_stored + n_new rows"""
    rng = np.random.default_rng(seed)
    keys = np.concatenate([w.keys[rng.permutation(n)[:n_stored]], w.keys[N:N + n_new]])
    order = rng.permutation(len(keys))
    return w.new[:len(keys)][order].copy(), keys[order].copy()


# ---- 1. and 2.: the mixed call -----------------------------------------------------------------------------------------------------

def test_mixed_call_equals_remove_then_insert(H, world):
    w = world
    A, B = _twins(H, w.X, w.keys[:N])
    assert A.max_layer >= 2                                    # an upper layer above layer 1: rows on layer 1 are touched
    X, keys = _mixed_call(w, N, 250, 150, 10)
    _by_definition(H, A, B, X, keys, w.Q)
    A.release(), B.release()


def test_mixed_call_with_max_batch_1(H, world):
    w = world
    n = 600
    A, B = _twins(H, w.X[:n], w.keys[:n])
    X, keys = _mixed_call(w, n, 250, 150, 11)
    _by_definition(H, A, B, X, keys, w.Q, max_batch=1)
    A.release(), B.release()


# ---- 3. the entry point and the whole top layer are replaced -----------------------------------------------------------------------

def test_entry_point_and_top_layer_replaced(H, world):
    w = world
    A, B = _twins(H, w.X, w.keys[:N])
    A.export()
    top_nodes = A.upper[-1][0]
    gone = np.unique(np.concatenate([top_nodes, [A.entry_point], np.arange(100, 160)]))
    assert A.entry_point in gone and len(top_nodes) >= 1
    rng = np.random.default_rng(12)
    keys = np.concatenate([w.keys[gone], w.keys[N:N + 50]])
    order = rng.permutation(len(keys))
    top_before, entry_before = A.max_layer, A.entry_point
    _by_definition(H, A, B, w.new[:len(keys)][order], keys[order], w.Q)
    inf = A.info()
    assert (inf.max_layer, inf.entry_point) != (top_before, entry_before)
    A.release(), B.release()


# ---- 4. a new node that raises max_layer --------------------------------------------------------------------------------------------

def test_new_node_raises_max_layer(H, world):
    w = world
    A, B = _twins(H, w.X, w.keys[:N], seed=RAISING_SEED)
    top = A.max_layer
    assert top == int(levels(RAISING_SEED, 0, N, M).max())
    A.export()
    keep = np.ones(N, bool)
    for nodes, _, _ in A.upper[-1:]:
        keep[nodes] = False                                    # the top layer stays: the removal must not lower max_layer
    keep[A.entry_point] = False
    rng = np.random.default_rng(13)
    gone = rng.permutation(np.flatnonzero(keep))[:250]
    keys = np.concatenate([w.keys[gone], w.keys[N:N + 150]])   # stored first: row i of the call is position 2750 + i
    _by_definition(H, A, B, w.new[:400], keys, w.Q, seed=RAISING_SEED)
    inf = A.info()
    assert inf.max_layer == top + 1 and inf.entry_point == RAISING_POSITION
    A.release(), B.release()


# ---- 5. and 6.: none stored, all stored ---------------------------------------------------------------------------------------------

def test_none_stored_is_insert_keyed(H, world):
    w = world
    A, B = _twins(H, w.X[:600], w.keys[:600])
    _by_definition(H, A, B, w.new[:200], w.keys[N:N + 200], w.Q)
    A.release(), B.release()


def test_every_node_replaced_equals_a_build(H, world):
    w = world
    n = 300
    A, B = _twins(H, w.X[:n], w.keys[:n])
    order = np.random.default_rng(14).permutation(n)
    _by_definition(H, A, B, w.new[:n], w.keys[:n][order], w.Q)
    C = H.Ohnsw.build_batch_bigarray(w.new[:n], M, EFC, seed=SEED)
    C.set_keys(w.keys[:n][order])
    _same(_snapshot(H, A, w.Q), _snapshot(H, C, w.Q))
    A.release(), B.release(), C.release()


# ---- 7. split rows under inner product; COSINE with unnormalised input --------------------------------------------------------------

@pytest.mark.parametrize("metric,d", [("IP", 100), ("COSINE", 24)])
def test_other_metrics(H, world, metric, d):
    w = world
    n = 800
    X = _floats(n, d, 21) * np.float32(3.0)                    # not unit vectors
    new = _floats(200, d, 22) * np.float32(0.25)
    Q = _floats(NQ, d, 23)
    code = {"IP": H.METRIC_IP, "COSINE": H.METRIC_COSINE}[metric]
    A, B = _twins(H, X, w.keys[:n], metric=code)
    if metric == "IP":
        assert A.info().row_format == H.ROWS_SPLIT
    rng = np.random.default_rng(24)
    keys = np.concatenate([w.keys[rng.permutation(n)[:120]], w.keys[N:N + 80]])
    order = rng.permutation(200)
    _by_definition(H, A, B, new[order], keys[order], Q)
    if metric == "COSINE":                                     # the stored rows are N(X), the new ones included
        np.testing.assert_allclose(np.linalg.norm(A.rows(), axis=1), 1.0, rtol=1e-5)
    A.release(), B.release()


# ---- 8. byte rows disappear with one non-byte vector ---------------------------------------------------------------------------------

def test_byte_rows_disappear(H, world):
    w = world
    n = 800
    rng = np.random.default_rng(31)
    X = rng.integers(0, 256, size=(n, D)).astype(np.float32)
    new = rng.integers(0, 256, size=(100, D)).astype(np.float32)
    new[57, 3] = 0.5
    Q = rng.integers(0, 256, size=(NQ, D)).astype(np.float32)
    A, B = _twins(H, X, w.keys[:n])
    assert A.info().row_format == H.ROWS_BYTES
    keys = np.concatenate([w.keys[rng.permutation(n)[:60]], w.keys[N:N + 40]])
    _by_definition(H, A, B, new, keys, Q)
    assert A.info().row_format != H.ROWS_BYTES
    A.release(), B.release()


# ---- 9. the code options --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("option", ["sq8_rows", "sq8_dim_rows", "half_rows", "bit_rows"])
def test_code_options_follow(H, world, option):
    w = world
    n = 800
    d = 32
    X, Q = _floats(n, d, 41), _floats(NQ, d, 42)
    new = _floats(200, d, 43) * np.float32(2.5)                # a wider range: the affine maps and the means move
    A, B = _twins(H, X, w.keys[:n])
    for hg in (A, B):
        hg.set_option(option, 1)
    rng = np.random.default_rng(44)
    keys = np.concatenate([w.keys[rng.permutation(n)[:120]], w.keys[N:N + 80]])
    order = rng.permutation(200)
    _by_definition(H, A, B, new[order], keys[order], Q)
    want = {"sq8_rows": H.ROWS_SQ8, "sq8_dim_rows": H.ROWS_SQ8_DIM, "half_rows": H.ROWS_HALF, "bit_rows": H.ROWS_BITS}[option]
    assert A.info().row_format == B.info().row_format == want
    if option == "sq8_rows":
        assert A.sq8_params() == B.sq8_params()
        np.testing.assert_array_equal(A.sq8_codes(), B.sq8_codes())
        # the whole table is quantised again: the map reaches past the old data's range, to the new, wider values
        lo, scale = A.sq8_params()
        assert lo < X.min() and lo + scale * 255 > X.max()
    elif option == "sq8_dim_rows":
        for a, b in zip(A.sq8_dim_params(), B.sq8_dim_params()):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        np.testing.assert_array_equal(A.sq8_dim_codes(), B.sq8_dim_codes())
    elif option == "bit_rows":
        np.testing.assert_array_equal(_bits(A.bit_params()), _bits(B.bit_params()))
        np.testing.assert_array_equal(A.bit_codes(), B.bit_codes())
    A.release(), B.release()


# ---- 10. marks ---------------------------------------------------------------------------------------------------------------------------

def test_marks_move_and_replaced_nodes_come_back_live(H, world):
    w = world
    n = 1000
    A, B = _twins(H, w.X[:n], w.keys[:n])
    rng = np.random.default_rng(51)
    marked = rng.permutation(n)[:100]
    for hg in (A, B):
        hg.mark_deleted(marked)
    in_p = marked[:40]
    others = np.setdiff1d(np.arange(n), marked)
    p_nodes = np.concatenate([in_p, rng.permutation(others)[:110]])
    keys = np.concatenate([w.keys[p_nodes], w.keys[N:N + 50]])
    order = rng.permutation(len(keys))
    X, keys = w.new[:len(keys)][order].copy(), keys[order]
    _by_definition(H, A, B, X, keys, w.Q)
    assert A.deleted_count() == 60
    np.testing.assert_array_equal(A.deleted_mask(), B.deleted_mask())
    # the 40 replaced keys are found by a search for their new vectors
    rows = np.flatnonzero(np.isin(keys, w.keys[in_p]))
    assert len(rows) == 40
    got, dist = H.Ohnsw.knn_batch_keyed(A, 1, X[rows], ef=64)
    np.testing.assert_array_equal(got[:, 0], keys[rows])
    assert (dist[:, 0] == 0).all()
    A.release(), B.release()


# ---- 11. hnsw_index_update ---------------------------------------------------------------------------------------------------------------

def test_update_by_id_on_a_handle_without_keys(H, world):
    w = world
    n = 1000
    A, B = _twins(H, w.X[:n], None, keyed=False)
    rng = np.random.default_rng(61)
    ids = rng.permutation(n)[:150].astype(np.int64)
    new_id = H.Ohnsw.update_batch(A, ids, w.new[:150], M, EFC, seed=SEED)
    b_new_id = H.Ohnsw.remove_batch(B, ids)
    H.Ohnsw.insert_batch(B, w.new[:150], M, EFC, seed=SEED)
    np.testing.assert_array_equal(new_id, b_new_id)
    assert A.info().n == n and A.keys_info() == (False, 0)
    _same(_snapshot(H, A, w.Q, keyed=False), _snapshot(H, B, w.Q, keyed=False))
    # out of range, repeated, and the keyed handle
    before = _snapshot(H, A, w.Q, keyed=False)
    with pytest.raises(H.InvalidArgument, match="not a stored node"):
        H.Ohnsw.update_batch(A, [0, n], w.new[:2], M, EFC, seed=SEED)
    with pytest.raises(H.InvalidArgument, match="appears twice"):
        H.Ohnsw.update_batch(A, [5, 7, 5], w.new[:3], M, EFC, seed=SEED)
    _same(before, _snapshot(H, A, w.Q, keyed=False))
    A.set_keys(w.keys[:n])
    with pytest.raises(H.InvalidArgument, match="hnsw_index_upsert_keyed"):
        H.Ohnsw.update_batch(A, [1], w.new[:1], M, EFC, seed=SEED)
    # ... and the keyed call on a handle that has nodes and no keys
    with pytest.raises(H.InvalidArgument, match="no keys"):
        H.Ohnsw.upsert_batch_keyed(B, w.new[:1], [7], M, EFC, seed=SEED)
    A.release(), B.release()


def test_empty_call_is_a_no_op(H, world):
    w = world
    hg = H.Ohnsw.build_batch_bigarray(w.X[:300], M, EFC, seed=SEED)
    hg.set_keys(w.keys[:300])
    flt = hg.filter(np.arange(0, 300, 2))
    replaced, new_id = H.Ohnsw.upsert_batch_keyed(hg, np.zeros((0, D), np.float32), [], M, EFC, seed=SEED)
    assert replaced.shape == (0,)
    np.testing.assert_array_equal(new_id, np.arange(300))
    H.Ohnsw.knn_batch_filtered(hg, K, w.Q, flt, ef=EF)         # the epoch did not move
    hg.release()


# ---- atomicity -----------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_the_handle_exactly_as_before(H, world):
    w = world
    n = 800
    d = 32
    X, Q = _floats(n, d, 71), _floats(NQ, d, 72)
    new = _floats(100, d, 73)
    hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=SEED)
    hg.set_keys(w.keys[:n])
    rng = np.random.default_rng(74)
    keys = np.concatenate([w.keys[rng.permutation(n)[:60]], w.keys[N:N + 40]])

    def snap():
        s = _snapshot(H, hg, Q)
        ids, dist = H.Ohnsw.knn_batch_filtered(hg, K, Q, flt, ef=EF)      # the filter made before is STILL ACCEPTED
        s["f_ids"], s["f_dist"] = ids, _bits(dist)
        return s

    flt = hg.filter(np.arange(0, n, 3))
    before = snap()

    def refused(exc, match, X=new, keys=keys, **args):
        with pytest.raises(exc, match=match):
            H.Ohnsw.upsert_batch_keyed(hg, X, keys, M, EFC, seed=SEED, **args)
        _same(before, snap())

    # a duplicate key in the call: the smallest is named
    dup = keys.copy()
    small, big = np.sort(keys)[[3, 70]]
    dup[np.flatnonzero(keys == small)[0] - 1] = small
    dup[np.flatnonzero(keys == big)[0] - 1] = big
    refused(H.InvalidArgument, r"key %d appears twice" % small, keys=dup)
    # wrong metric, wrong id_base
    refused(H.InvalidArgument, "metric", metric=H.METRIC_IP)
    with pytest.raises(H.InvalidArgument, match="id_base"):
        p = H._BuildParams(M, EFC, H.METRIC_L2, 1, SEED, 0, 0, 0, 0)
        H._check(H.load().hnsw_index_upsert_keyed(hg.handle, H._ptr(new), H._ptr(keys), len(keys), d, H._C.byref(p), None, None))
    _same(before, snap())
    # a pending submitted request
    req = H.submit(hg, Q, EF, K)
    with pytest.raises(H.InvalidArgument, match="not waited for"):
        H.Ohnsw.upsert_batch_keyed(hg, new, keys, M, EFC, seed=SEED)
    req.wait()
    _same(before, snap())
    # a value of 1e6 under half_rows: refused when the half copy of the new table is made, after the graph was built
    hg.set_option("half_rows", 1)
    flt = hg.filter(np.arange(0, n, 3))
    before = snap()
    big_v = new.copy()
    big_v[-1, 5] = 1e6
    refused(H.Failure, "fp16 infinity", X=big_v)
    hg.set_option("half_rows", 0)
    # a NaN in the LAST new vector under sq8_rows: refused before anything is built
    hg.set_option("sq8_rows", 1)
    flt = hg.filter(np.arange(0, n, 3))
    before = snap()
    nan_v = new.copy()
    nan_v[-1, d - 1] = np.nan
    refused(H.Failure, "new vector %d is NaN" % (len(new) - 1), X=nan_v)
    # a successful upsert moves the epoch ONCE: the old filter is refused, a new one and a search work
    replaced, _ = H.Ohnsw.upsert_batch_keyed(hg, new, keys, M, EFC, seed=SEED)
    assert replaced.sum() == 60 and hg.info().n == n + 40
    with pytest.raises(H.InvalidArgument):
        H.Ohnsw.knn_batch_filtered(hg, K, Q, flt, ef=EF)
    flt2 = hg.filter(np.arange(0, n + 40, 3))
    ids, _ = H.Ohnsw.knn_batch_filtered(hg, K, Q, flt2, ef=EF)
    assert (ids % 3 == 0).all()
    got, _ = H.Ohnsw.knn_batch_keyed(hg, K, Q, ef=EF)
    assert got.shape == (NQ, K)
    hg.release()


# ---- the C++ front end -------------------------------------------------------------------------------------------------------------

def test_cpp_front_end_upsert(H, tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "test_front_upsert")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_upsert.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "upsert front-end ok" in out.stdout, out.stdout + out.stderr
