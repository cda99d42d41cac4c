"""Keys the index owns (ocaml-hnsw_amd/csrc/hnsw_keys.hip): set / clear / keys_of / find, the keyed search against the plain and the
filtered calls of the same handle, and the keys' way through remove, compact and insert against an unkeyed twin -- on the world of
tests/test_gpu_range.py (2003 x 20 Gaussian vectors, the oracle's graph with M 8, efC 40, seed 1; 64 queries, ef 16, k 10).

The keys are NASTY on purpose: INT64_MIN, INT64_MAX, -1, 0, pairs that differ only in bit 32 and above (x, x + 2**32) and pairs that
differ only in the low word -- what a 32-bit truncation, an unsigned compare or an unsigned sort gets wrong.  Every comparison is
exact: keys equal element for element, distances and counters compared as bits."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, NQ, EF, K = 2003, 20, 64, 16, 10
M, EFC = 8, 40
I64 = np.iinfo(np.int64)
MISSING = -(2 ** 62) - 12345            # no stored key: see nasty_keys


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def nasty_keys(n, seed=7, extremes=True):
    """n distinct int64 keys in a shuffled order: the special values first (so that small n hold them), random ones behind"""
    x, y = 0x0000123400005678, -0x0000432100008765
    special = ([I64.min, I64.max] if extremes else []) + [
        -1, 0, 1, x, x + 2 ** 32, x + 2 ** 33, x + 2 ** 63 - 2 ** 62, y, y - 2 ** 32, y + 2 ** 32,      # bit 32 and above only
        x + 1, x + 2, y + 1, 2 ** 32, 2 ** 32 - 1, -2 ** 32, -2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31 - 1,       # low word only / the word's edge
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


class World:
    pass


@pytest.fixture(scope="module")
def world(H, oracle):
    """the index of the issue; `fresh()` uploads the same graph again as a handle of its own"""
    w = World()
    w.X, w.Q = _floats(N, D, 1), _floats(NQ, D, 2)
    w.space = oracle.Space.l2(w.X, arith=oracle.TREE16)
    w.g = oracle.build_ohnsw(w.space, M, EFC, seed=1)
    w.keys = nasty_keys(N)
    w.fresh = lambda: H.Hgraph(w.X, w.g.deg0, w.g.nbr0, w.g.upper, entry_point=w.g.entry_point, id_base=0, max_degree=M)
    w.hg = w.fresh()                    # keyed, never changed by a test
    w.hg.set_keys(w.keys)
    w.plain = H._search(w.hg, w.Q, EF, K, H.FILL_OHNSW, True)
    yield w
    w.hg.release()


def _graph(hg):
    """the exported graph with the slots past each degree blanked"""
    hg.export()
    def blank(deg, nbr):
        nbr = nbr.copy()
        nbr[np.arange(nbr.shape[1])[None, :] >= deg[:, None]] = -1
        return nbr
    return (hg.n, hg.entry_point, hg.max_layer, hg.deg0.copy(), blank(hg.deg0, hg.nbr0),
            [(nodes.copy(), deg.copy(), blank(deg, nbr)) for nodes, deg, nbr in hg.upper])


def _same_graph(a, b):
    assert a[:3] == b[:3]
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[4], b[4])
    assert len(a[5]) == len(b[5])
    for la, lb in zip(a[5], b[5]):
        for xa, xb in zip(la, lb):
            np.testing.assert_array_equal(xa, xb)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _translate(keys, ids, base=0, missing=MISSING):
    """the definition of hnsw_index_keys_of in numpy"""
    ids = np.asarray(ids, np.int64) - base
    ok = (ids >= 0) & (ids < len(keys))
    return np.where(ok, keys[np.where(ok, ids, 0)] if len(keys) else missing, missing).astype(np.int64)


# ---- 1. round trip: set, keys(), find ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2003])
def test_round_trip(H, n, base):
    hg = H.Hgraph.flat(_floats(n, 4, 3), id_base=base)
    assert hg.keys_info() == (False, 0)
    with pytest.raises(H.InvalidArgument, match="no keys"):
        hg.keys()
    rng = np.random.default_rng(n)
    for extremes in (True, False):
        keys = nasty_keys(n, seed=n, extremes=extremes)
        hg.set_keys(keys)                                               # (the second round replaces the first round's keys)
        assert hg.keys_info() == (True, 20 * n)
        np.testing.assert_array_equal(hg.keys(), keys)
        perm = rng.permutation(n)
        np.testing.assert_array_equal(hg.find_keys(keys[perm]), perm + base)
        # keys_of for explicit ids: the fill id -1, the ids just outside [base, base + n), far outside; any shape
        ids = np.concatenate([perm[:7] + base, [-1, base - 1, base + n, 2 ** 31 - 1, -2 ** 31, base, base + n - 1]]).astype(np.int32)
        np.testing.assert_array_equal(hg.keys(ids, missing=MISSING), _translate(keys, ids, base))
        assert hg.keys(np.zeros((0, 3), np.int32)).shape == (0, 3)
        np.testing.assert_array_equal(hg.keys(ids[:6].reshape(2, 3), missing=5), _translate(keys, ids[:6], base, 5).reshape(2, 3))
        # absent keys: between two stored keys; below all and above all where the extremes are not stored
        s = np.sort(keys)
        stored = set(keys.tolist())
        absent = [int(k) + 1 for k in s[:-1] if int(k) + 1 not in stored][:40] + [MISSING]
        if not extremes:
            absent += [I64.min, int(s[0]) - 1, I64.max, int(s[-1]) + 1]
        else:
            assert s[0] == I64.min and (n == 1 or s[-1] == I64.max)
        absent = [k for k in absent if k not in stored]
        np.testing.assert_array_equal(hg.find_keys(absent), np.full(len(absent), base - 1))
        # m = 0, and a list with repeats (the last element of the table among them)
        assert hg.find_keys([]).shape == (0,)
        rep = np.array([s[-1], s[0], s[-1], MISSING, s[n // 2], s[-1]], np.int64)
        want = np.array([np.flatnonzero(keys == k)[0] + base if k in stored else base - 1 for k in rep.tolist()])
        np.testing.assert_array_equal(hg.find_keys(rep), want)
    with pytest.raises(H.InvalidArgument, match="keys, the index has"):
        hg.set_keys(np.arange(n + 1))
    np.testing.assert_array_equal(hg.keys(), keys)
    hg.clear_keys()
    assert hg.keys_info() == (False, 0)
    with pytest.raises(H.InvalidArgument, match="no keys"):
        hg.find_keys([1])
    hg.release()


# ---- 2. duplicates ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("previous", [False, True])
def test_duplicates_are_refused_naming_the_smallest(H, previous):
    hg = H.Hgraph.flat(_floats(N, 4, 3))
    before = nasty_keys(N, seed=11)
    if previous:
        hg.set_keys(before)
    keys = nasty_keys(N, seed=12)
    big, small = 2 ** 40 + 5, -2 ** 40 - 5                  # (2^40 + 5 and its low word 5 are different keys)
    assert big not in keys and small not in keys
    keys[100] = keys[1600] = big                            # two equal keys 1500 rows apart
    keys[1900] = keys[7] = small                            # ... and a second pair with a smaller key
    with pytest.raises(H.InvalidArgument, match=r"key %d is the smallest duplicated key" % small):
        hg.set_keys(keys)
    assert hg.keys_info() == ((True, 20 * N) if previous else (False, 0))
    if previous:
        np.testing.assert_array_equal(hg.keys(), before)
        np.testing.assert_array_equal(hg.find_keys(before[::-1]), np.arange(N)[::-1])
    hg.release()


# ---- 3. the keyed search -------------------------------------------------------------------------------------------------------

def test_keyed_search_is_the_plain_call_in_keys(H, world):
    w = world
    ids, dist, nd, nh = w.plain
    keys, kdist, knd, knh, stage = H.Ohnsw.knn_batch_keyed(w.hg, K, w.Q, ef=EF, counters=True, missing=MISSING)
    np.testing.assert_array_equal(keys, w.keys[ids])
    np.testing.assert_array_equal(keys, w.hg.keys(ids, missing=MISSING))
    np.testing.assert_array_equal(_bits(kdist), _bits(dist))
    np.testing.assert_array_equal(knd, nd)
    np.testing.assert_array_equal(knh, nh)
    assert (stage == 0).all()
    # one query (the plain call's small-block path) and the functor rule
    k1, d1 = H.Ohnsw.knn_batch_keyed(w.hg, K, w.Q[:1], ef=EF)
    np.testing.assert_array_equal(k1, keys[:1])
    np.testing.assert_array_equal(_bits(d1), _bits(dist[:1]))
    fi, fd = H._search(w.hg, w.Q, EF, K, H.FILL_BA, sem=H.SEM_FUNCTOR)
    bk, bd = H.Ba.knn_batch_keyed(w.hg, w.Q, EF, K)
    np.testing.assert_array_equal(bk, w.keys[fi])
    np.testing.assert_array_equal(_bits(bd), _bits(fd))
    # a handle without keys is refused, and the plain call on the keyed handle still answers in ids
    bare = w.fresh()
    with pytest.raises(H.InvalidArgument, match="no keys"):
        H.Ohnsw.knn_batch_keyed(bare, K, w.Q, ef=EF)
    bi, bdist = H._search(bare, w.Q, EF, K, H.FILL_OHNSW)
    np.testing.assert_array_equal(bi, ids)
    np.testing.assert_array_equal(_bits(bdist), _bits(dist))
    bare.release()


@pytest.mark.parametrize("case", ["half", "seven"])
def test_keyed_search_under_a_filter(H, world, case):
    w = world
    rng = np.random.default_rng(21)
    allow = rng.random(N) < 0.5 if case == "half" else np.isin(np.arange(N), rng.choice(N, size=7, replace=False))
    f = w.hg.filter(allow)
    ids, dist, nd, nh, stage = H.Ohnsw.knn_batch_filtered(w.hg, K, w.Q, f, ef=EF, counters=True)
    keys, kdist, knd, knh, kstage = H.Ohnsw.knn_batch_keyed(w.hg, K, w.Q, ef=EF, filter=f, counters=True, missing=MISSING)
    np.testing.assert_array_equal(keys, _translate(w.keys, ids))
    np.testing.assert_array_equal(_bits(kdist), _bits(dist))
    np.testing.assert_array_equal(knd, nd)
    np.testing.assert_array_equal(knh, nh)
    np.testing.assert_array_equal(kstage, stage)
    if case == "seven":
        assert (ids[:, 7:] == -1).all() and (ids[:, :7] >= 0).all()
        assert (keys[:, 7:] == MISSING).all() and np.isnan(kdist[:, 7:]).all()
        # the same filter made from the keys
        fk = w.hg.filter_by_keys(w.keys[allow])
        np.testing.assert_array_equal(fk.bits(), f.bits())
        k2, d2 = H.Ohnsw.knn_batch_keyed(w.hg, K, w.Q, ef=EF, filter=fk, missing=MISSING)
        np.testing.assert_array_equal(k2, keys)
        fk.release()
    f.release()


def test_keyed_search_on_a_half_marked_handle(H, world):
    w = world
    hg = w.fresh()
    hg.set_keys(w.keys)
    marked = np.random.default_rng(22).random(N) < 0.5
    hg.mark_deleted(np.flatnonzero(marked))
    ids, dist, nd, nh = H._search(hg, w.Q, EF, K, H.FILL_OHNSW, True)
    assert not marked[ids].any()
    keys, kdist, knd, knh, _ = H.Ohnsw.knn_batch_keyed(hg, K, w.Q, ef=EF, counters=True, missing=MISSING)
    np.testing.assert_array_equal(keys, w.keys[ids])
    np.testing.assert_array_equal(_bits(kdist), _bits(dist))
    np.testing.assert_array_equal(knd, nd)
    np.testing.assert_array_equal(knh, nh)
    # a marked node still has its key: the ids are explicit
    np.testing.assert_array_equal(hg.keys(np.flatnonzero(marked).astype(np.int32)), w.keys[marked])
    hg.release()


# ---- 4. remove -----------------------------------------------------------------------------------------------------------------

def test_remove_moves_the_keys_with_their_nodes(H, world):
    w = world
    dead = np.sort(np.random.default_rng(31).choice(N, size=300, replace=False))
    keyed, twin, third = w.fresh(), w.fresh(), w.fresh()
    keyed.set_keys(w.keys)
    third.set_keys(w.keys)
    new_a = H.Ohnsw.remove_batch(keyed, dead)
    new_b = H.Ohnsw.remove_batch(twin, dead)
    np.testing.assert_array_equal(new_a, new_b)
    want = _graph(twin)
    _same_graph(_graph(keyed), want)
    left = np.delete(w.keys, dead)
    np.testing.assert_array_equal(keyed.keys(), left)
    np.testing.assert_array_equal(keyed.find_keys(w.keys), new_a)           # removed: id_base - 1 = -1, as out_new_id says
    assert keyed.keys_info() == (True, 20 * (N - 300)) and twin.keys_info() == (False, 0)
    # by key, in another order
    new_c = third.remove_keys(w.keys[dead][::-1])
    np.testing.assert_array_equal(new_c, new_a)
    _same_graph(_graph(third), want)
    np.testing.assert_array_equal(third.keys(), left)
    assert third.vectors.shape == (N - 300, D)
    np.testing.assert_array_equal(third.vectors, w.X[new_a >= 0])
    # an absent key (one that was just removed) is refused, named, and nothing changes
    gone = int(w.keys[dead[5]])
    with pytest.raises(H.InvalidArgument, match=r"keys\[1\]=%d is not a stored key" % gone):
        third.remove_keys([int(left[0]), gone])
    assert third.info().n == N - 300
    np.testing.assert_array_equal(third.keys(), left)
    _same_graph(_graph(third), want)
    # the keyed search after the removal: the twin's rows in keys
    ti, td = H._search(twin, w.Q, EF, K, H.FILL_OHNSW)
    kk, kd = H.Ohnsw.knn_batch_keyed(keyed, K, w.Q, ef=EF)
    np.testing.assert_array_equal(kk, left[ti])
    np.testing.assert_array_equal(_bits(kd), _bits(td))
    for hg in (keyed, twin, third):
        hg.release()


def test_remove_every_node_then_insert_keyed(H, world):
    w = world
    hg = H.Ohnsw.build_batch_bigarray(w.X[:200], M, EFC, seed=1)
    keys = nasty_keys(200, seed=5)
    hg.set_keys(keys)
    hg.remove_keys(keys[::-1])
    assert hg.info().n == 0 and hg.keys_info() == (True, 0) and hg.keys().shape == (0,)
    np.testing.assert_array_equal(hg.find_keys(keys[:3]), [-1, -1, -1])
    with pytest.raises(H.InvalidArgument, match="keyed call"):
        H.Ohnsw.insert_batch(hg, w.X[:50], M, EFC, seed=1)
    ids = H.Ohnsw.insert_batch_keyed(hg, w.X[:50], keys[100:150], M, EFC, seed=1)
    np.testing.assert_array_equal(ids, np.arange(50))
    np.testing.assert_array_equal(hg.keys(), keys[100:150])
    twin = H.Ohnsw.build_batch_bigarray(w.X[:50], M, EFC, seed=1)
    _same_graph(_graph(hg), _graph(twin))
    # an EMPTY index without keys starts its keys with the keyed insert
    bare = H.Ohnsw.build_batch_bigarray(w.X[:20], M, EFC, seed=1)
    H.Ohnsw.remove_batch(bare, np.arange(20))
    assert bare.keys_info() == (False, 0)
    H.Ohnsw.insert_batch_keyed(bare, w.X[:50], keys[100:150], M, EFC, seed=1)
    np.testing.assert_array_equal(bare.keys(), keys[100:150])
    _same_graph(_graph(bare), _graph(twin))
    kk, kd = H.Ohnsw.knn_batch_keyed(bare, 5, w.Q, ef=EF)
    ti, td = H._search(twin, w.Q, EF, 5, H.FILL_OHNSW)
    np.testing.assert_array_equal(kk, keys[100:150][ti])
    np.testing.assert_array_equal(_bits(kd), _bits(td))
    for g in (hg, twin, bare):
        g.release()


# ---- 5. marks ------------------------------------------------------------------------------------------------------------------

def test_marks_by_key_and_compact(H, world):
    w = world
    S = np.sort(np.random.default_rng(41).choice(N, size=400, replace=False))
    keyed, twin = w.fresh(), w.fresh()
    keyed.set_keys(w.keys)
    keyed.mark_deleted_keys(w.keys[S][::-1])
    twin.mark_deleted(S)
    np.testing.assert_array_equal(keyed.deleted_mask(), twin.deleted_mask())
    assert keyed.deleted_count() == 400
    absent = MISSING
    with pytest.raises(H.InvalidArgument, match=r"keys\[0\]=%d is not a stored key" % absent):
        keyed.mark_deleted_keys([absent, int(w.keys[0])])
    with pytest.raises(H.InvalidArgument, match="not a stored key"):
        keyed.unmark_deleted_keys([int(w.keys[S[0]]), absent])
    np.testing.assert_array_equal(keyed.deleted_mask(), twin.deleted_mask())
    keyed.unmark_deleted_keys(w.keys[S[:100]])
    twin.unmark_deleted(S[:100])
    marked = twin.deleted_mask()
    np.testing.assert_array_equal(keyed.deleted_mask(), marked)
    assert marked.sum() == 300
    # filter_by_keys: exactly the named nodes, a marked node's bit clear
    named = np.concatenate([S[90:110], [0, 1, 2, N - 1]])
    fk = keyed.filter_by_keys(w.keys[named])
    want = np.zeros(N, bool)
    want[named] = True
    want &= ~marked
    assert marked[named].any() and want.sum() == fk.count()
    np.testing.assert_array_equal(fk.bits(), H.pack_allow(want, N))
    with pytest.raises(H.InvalidArgument, match=r"keys\[1\]=%d is not a stored key" % absent):
        keyed.filter_by_keys([int(w.keys[3]), absent, absent])
    fk.release()
    new_a, new_b = keyed.compact(), twin.compact()
    np.testing.assert_array_equal(new_a, new_b)
    left = w.keys[~marked]
    np.testing.assert_array_equal(keyed.keys(), left)
    _same_graph(_graph(keyed), _graph(twin))
    assert keyed.deleted_count() == 0
    ti, td, tnd, tnh = H._search(twin, w.Q, EF, K, H.FILL_OHNSW, True)
    kk, kd, knd, knh, stage = H.Ohnsw.knn_batch_keyed(keyed, K, w.Q, ef=EF, counters=True)
    np.testing.assert_array_equal(kk, left[ti])
    np.testing.assert_array_equal(_bits(kd), _bits(td))
    np.testing.assert_array_equal(knd, tnd)
    np.testing.assert_array_equal(knh, tnh)
    assert (stage == 0).all()
    keyed.release()
    twin.release()


# ---- 6. insert -----------------------------------------------------------------------------------------------------------------

def test_insert_keyed_appends_the_keys(H, world):
    w = world
    n1, n2 = 1500, 1750
    keyed = H.Ohnsw.build_batch_bigarray(w.X[:n1], M, EFC, seed=1)
    twin = H.Ohnsw.build_batch_bigarray(w.X[:n1], M, EFC, seed=1)
    keyed.set_keys(w.keys[:n1])
    f = keyed.filter(np.ones(n1, bool))
    for a, b in ((n1, n2), (n2, N)):
        got = H.Ohnsw.insert_batch_keyed(keyed, w.X[a:b], w.keys[a:b], M, EFC, seed=1)
        np.testing.assert_array_equal(got, H.Ohnsw.insert_batch(twin, w.X[a:b], M, EFC, seed=1))
        np.testing.assert_array_equal(keyed.keys(), w.keys[:b])
    with pytest.raises(H.InvalidArgument, match="the filter was made"):     # outgrown, as after any insert
        H.Ohnsw.knn_batch_keyed(keyed, K, w.Q, ef=EF, filter=f)
    f.release()
    want = _graph(twin)
    _same_graph(_graph(keyed), want)
    np.testing.assert_array_equal(keyed.find_keys(w.keys[::-1]), np.arange(N)[::-1])
    assert keyed.vectors.shape == (N, D)
    # refusals: a stored key, two equal keys in the call, a plain insert; n, keys and graph as they were
    fresh = [k for k in (10 ** 15 + 1, 10 ** 15 + 2, -10 ** 15) if k not in set(w.keys.tolist())]
    assert len(fresh) == 3
    B = w.X[:3]
    with pytest.raises(H.InvalidArgument, match=r"keys\[1\]=%d is a stored key already" % int(w.keys[1999])):
        H.Ohnsw.insert_batch_keyed(keyed, B, [fresh[0], int(w.keys[1999]), fresh[1]], M, EFC, seed=1)
    with pytest.raises(H.InvalidArgument, match=r"key %d appears twice in the call" % fresh[2]):
        H.Ohnsw.insert_batch_keyed(keyed, B, [fresh[2], fresh[0], fresh[2]], M, EFC, seed=1)
    with pytest.raises(H.InvalidArgument, match="keyed call"):
        H.Ohnsw.insert_batch(keyed, B, M, EFC, seed=1)
    assert keyed.info().n == N and keyed.n == N
    np.testing.assert_array_equal(keyed.keys(), w.keys)
    _same_graph(_graph(keyed), want)
    # an index with nodes and no keys refuses the keyed insert
    with pytest.raises(H.InvalidArgument, match="no keys"):
        H.Ohnsw.insert_batch_keyed(twin, B, fresh, M, EFC, seed=1)
    assert twin.info().n == N and twin.keys_info() == (False, 0)
    keyed.release()
    twin.release()


# ---- 7. save -------------------------------------------------------------------------------------------------------------------

def test_save_does_not_save_keys_and_set_keys_is_the_round_trip(H, world, tmp_path):
    w = world
    path = str(tmp_path / "keyed.idx")
    saved = w.hg.keys()
    w.hg.save(path)
    back = H.Hgraph.load(path)
    assert back.keys_info() == (False, 0)
    back.set_keys(saved)
    want = H.Ohnsw.knn_batch_keyed(w.hg, K, w.Q, ef=EF, counters=True, missing=MISSING)
    got = H.Ohnsw.knn_batch_keyed(back, K, w.Q, ef=EF, counters=True, missing=MISSING)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
    for a, b in zip(got[2:], want[2:]):
        np.testing.assert_array_equal(a, b)
    back.release()


# ---- 8. the C++ front end ------------------------------------------------------------------------------------------------------

def test_cpp_front_end_keys(H, tmp_path):
    from conftest import ROOT
    exe = str(tmp_path / "test_front_keys")
    lib_dir = os.path.join(ROOT, "ocaml-hnsw_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_front_keys.cpp"), "-o", exe, "-L", lib_dir, "-lhnsw_mi355x",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "keys front-end ok" in out.stdout, out.stdout + out.stderr
