"""The sharded index's query calls (ocaml-hnsw_amd/csrc/hnsw_sharded.hip) against the header's definition, which is in terms of
public calls: a sharded filter is one hnsw_filter_create per shard over the slice of the global mask, a sharded filtered row is the
merge of the rows hnsw_search_batch_filtered gives on the borrowed shard handles, a sharded range segment the merge of the shards'
own segments.  Every expectation is numpy over what the shard handles return through the single-index Python calls, compared bit
for bit (floats as uint32, dtypes checked).  Device 0 is listed several times, so one GPU is enough."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, NQ, M, EFC, SEED = 5003, 24, 70, 8, 40, 11
N_IP, D_IP = 3001, 100
EF, K = 32, 10
EXACT = 0xFFFFFFFF


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


def _pack(mask):
    """the words hnsw_filter_create takes for a boolean mask: bit v & 31 of word v >> 5, the tail of the last word clear"""
    words = (len(mask) + 31) // 32
    padded = np.zeros(words * 32, np.uint8)
    padded[:len(mask)] = mask
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def _bounds(s):
    return [s.shard(g)[1] for g in range(s.num_shards())] + [s.n]


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
    w.half = np.random.default_rng(17).random(N) < 0.5
    w.half_ip = np.random.default_rng(18).random(N_IP) < 0.5
    cache = {}

    def sharded(G, metric=0):
        if (G, metric) not in cache:
            X = w.X if metric == 0 else w.X_ip
            cache[(G, metric)] = H.ShardedHgraph.build(X, M, EFC, [0] * G, seed=SEED, metric=metric)
        return cache[(G, metric)]

    w.sharded = sharded
    # the radii of the range tests, from the exact distances of the whole table (computed once): below every distance, the batch's
    # median 5th-nearest distance, and the distance below which about 60 % of all (query, row) pairs lie
    radii = {}

    def radii_of(metric):
        if metric not in radii:
            X, Q = (w.X.astype(np.float64), w.Q.astype(np.float64)) if metric == 0 else (w.X_ip.astype(np.float64), w.Q_ip.astype(np.float64))
            if metric == 0:
                d = np.sqrt(((Q * Q).sum(axis=1)[:, None] - 2.0 * Q @ X.T + (X * X).sum(axis=1)[None, :]).clip(min=0.0))
            else:
                d = 1.0 - Q @ X.T                               # HNSW_METRIC_IP
            _, d5 = sharded(3, metric).brute_force_knn(5, Q.astype(np.float32))
            radii[metric] = (float(d.min()) - (0.5 if metric == 0 else 1.0), float(np.median(d5[:, 4])), float(np.quantile(d, 0.6)))
        return radii[metric]

    w.radii = radii_of
    yield w
    for s in cache.values():
        s.release()


# ---- 1. the sharded filter is the global mask cut at the shard bounds --------------------------------------------------------------

def _part_words(H, s, fhandle):
    """every part of the sharded filter `fhandle` read back: hnsw_sharded_filter_part, hnsw_filter_bits, hnsw_filter_count"""
    L = H.load()
    words, counts = [], []
    for g in range(s.num_shards()):
        p = ctypes.c_void_p()
        assert L.hnsw_sharded_filter_part(fhandle, g, ctypes.byref(p)) == H.OK
        n_g = s.shard(g)[0].info().n
        out = np.zeros((n_g + 31) // 32, np.uint32)
        assert L.hnsw_filter_bits(p, H._ptr(out)) == H.OK
        c = ctypes.c_int64(-1)
        assert L.hnsw_filter_count(p, ctypes.byref(c)) == H.OK
        words.append(out)
        counts.append(c.value)
    assert L.hnsw_sharded_filter_part(fhandle, s.num_shards(), ctypes.byref(p)) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_filter_part(fhandle, -1, ctypes.byref(p)) == H.ERR_BAD_ARG
    return words, counts


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_filter_parts_are_the_slices_of_the_global_mask(H, world, G):
    L = H.load()
    s = world.sharded(G)
    lo = _bounds(s)
    assert lo == [N * g // G for g in range(G + 1)]
    if G == 3:
        assert lo == [0, 1667, 3335, 5003] and all(b % 32 for b in lo[1:])
    edges = np.zeros(N, bool)
    for b in lo[1:-1]:
        edges[[b - 1, b]] = True                                # only the last row of a shard and the first of the next
    masks = {"half": world.half, "edges": edges, "ones": np.ones(N, bool), "zeros": np.zeros(N, bool)}
    for name, mask in masks.items():
        f = s.filter(mask)
        try:
            words, counts = _part_words(H, s, f.handle)
            for g in range(G):
                part = mask[lo[g]:lo[g + 1]]
                np.testing.assert_array_equal(words[g], _pack(part), err_msg="%s G %d part %d" % (name, G, g))
                np.testing.assert_array_equal(f.part_bits(g), words[g])
                assert counts[g] == int(part.sum())
            assert f.count() == int(mask.sum())
        finally:
            f.release()
    # junk above n in the last word of the caller's mask (n % 32 = 11): not counted, and not in the last part's last word
    junk = _pack(world.half).copy()
    junk[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(N % 32)
    fh = ctypes.c_void_p()
    assert L.hnsw_sharded_filter_create(s.handle, H._ptr(junk), N, ctypes.byref(fh)) == H.OK
    try:
        words, counts = _part_words(H, s, fh)
        for g in range(G):
            np.testing.assert_array_equal(words[g], _pack(world.half[lo[g]:lo[g + 1]]))
        c = ctypes.c_int64(-1)
        assert L.hnsw_sharded_filter_count(fh, ctypes.byref(c)) == H.OK and c.value == int(world.half.sum()) == sum(counts)
    finally:
        assert L.hnsw_sharded_filter_destroy(fh) == H.OK
    # a wrong n_bits: refused, *out NULL
    for n_bits in (N - 1, N + 1, 0):
        fh = ctypes.c_void_p(1)
        assert L.hnsw_sharded_filter_create(s.handle, H._ptr(junk), n_bits, ctypes.byref(fh)) == H.ERR_BAD_ARG and fh.value is None
    assert L.hnsw_sharded_filter_create(s.handle, None, N, ctypes.byref(fh)) == H.ERR_BAD_ARG
    with pytest.raises(H.InvalidArgument):
        s.filter(np.ones(N - 1, bool))


def test_a_filter_of_another_sharded_index_is_refused(H, world):
    L = H.load()
    s, t = world.sharded(3), world.sharded(2)
    f = t.filter(world.half)
    try:
        with pytest.raises(H.InvalidArgument, match="another hnsw_sharded"):
            s.knn_batch_filtered(world.Q, EF, K, f)
        with pytest.raises(H.InvalidArgument, match="another hnsw_sharded"):
            s.range_search(world.Q, 1.0, ef=16, filter=f)
        with pytest.raises(H.InvalidArgument, match="another hnsw_sharded"):
            s.brute_force_range(world.Q, 1.0, filter=f)
        p = H._SearchParams(EF, K, 0, 0)                        # ... and a null one, the outputs untouched
        out_i, out_d = np.full((NQ, K), 7, np.int64), np.full((NQ, K), 7, np.float32)
        for fh in (None, f.handle):
            assert L.hnsw_sharded_search_batch_filtered(s.handle, fh, H._ptr(world.Q), NQ, D, ctypes.byref(p), H._ptr(out_i), H._ptr(out_d), None,
                                                        None, None) == H.ERR_BAD_ARG
        assert (out_i == 7).all() and (out_d == 7).all()
    finally:
        f.release()


# ---- 2. filtered k-NN ---------------------------------------------------------------------------------------------------------------

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


def _check_filtered(H, s, Q, mask, ef, k, fill, sem, ctx):
    """the sharded call against the merge of hnsw_search_batch_filtered on every shard handle under its slice of the mask
    -> the per-shard stages [G][nq]"""
    lo = _bounds(s)
    rows = []
    for g in range(s.num_shards()):
        hg, first = s.shard(g)
        assert first == lo[g]
        rows.append(H._search_filtered(hg, mask[lo[g]:lo[g + 1]], Q, ef, k, fill, counters=True, sem=sem))
    want = np_merge(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), lo[:-1], k, s.id_base, fill)
    nd, nh = sum(r[2] for r in rows), sum(r[3] for r in rows)   # (uint32 arrays: the sums wrap as the kernel's do)
    stages = np.stack([r[4] for r in rows])
    got = s.knn_batch_filtered(Q, ef, k, mask, fill=fill, sem=sem, counters=True)
    _same(got, want + (nd, nh, stages.max(axis=0)), ctx)
    real = got[0] >= 0
    assert mask[got[0][real]].all(), ctx                        # (only allowed rows)
    return stages


def _knn_masks(lo):
    """selectivity 1, 0.5, 0.02, empty on shard 1 (the last shard if there is no shard 1) and dense elsewhere, 7 rows in all"""
    g1 = min(1, len(lo) - 2)
    hole = np.ones(N, bool)
    hole[lo[g1]:lo[g1 + 1]] = False
    seven = np.zeros(N, bool)
    seven[[0, 1, 1666, 1667, 3334, 4000, 5002]] = True
    return {"all": np.ones(N, bool), "half": np.random.default_rng(17).random(N) < 0.5, "sparse": np.random.default_rng(21).random(N) < 0.02,
            "hole": hole, "seven": seven}


@pytest.mark.parametrize("G", [1, 3, 8])
def test_filtered_search_is_the_merge_of_the_shards_filtered_rows(H, world, G):
    s = world.sharded(G)
    lo = _bounds(s)
    masks = _knn_masks(lo)
    sparse_stages = []
    for name, mask in masks.items():
        for sem in (H.SEM_OHNSW, H.SEM_FUNCTOR):
            for fill in (H.FILL_OHNSW, H.FILL_BA):
                stages = _check_filtered(H, s, world.Q, mask, EF, K, fill, sem, "G %d mask %s sem %d fill %d" % (G, name, sem, fill))
                if name == "sparse":
                    sparse_stages.append(stages)
                if name == "hole" and G > 1:
                    assert (stages[1] == EXACT).all()           # nothing allowed there: no walk
                if name == "seven":
                    assert (stages == EXACT).all()              # fewer than k allowed in every shard
    ids, dist = s.knn_batch_filtered(world.Q, EF, K, masks["seven"], fill=H.FILL_BA)
    assert (np.sort(ids[:, :7], axis=1) == np.flatnonzero(masks["seven"])).all() and (ids[:, 7:] == -1).all() and np.isposinf(dist[:, 7:]).all()
    if G == 8:
        # The sparse mask must exercise both kinds of shard answer.  With 8 shards of 625 or 626 rows its per-shard counts are
        # 22, 12, 12, 9, 13, 12, 13, 6 (numpy, seed 21): shards 3 and 7 allow fewer than k = 10 rows and answer from the exact
        # stage; the others allow at least k and the ladder's largest W (1024) holds a whole shard.
        counts = [int(masks["sparse"][a:b].sum()) for a, b in zip(lo, lo[1:])]
        assert min(counts) < K <= max(counts), counts
        st = np.stack(sparse_stages)
        assert (st == EXACT).any() and (st != EXACT).any(), "the sparse mask no longer gives both a ladder stage and the exact stage"


def test_filtered_search_inner_product(H, world):
    s = world.sharded(3, H.METRIC_IP)
    lo = _bounds(s)
    rows = []
    for g in range(3):
        rows.append(H._search_filtered(s.shard(g)[0], world.half_ip[lo[g]:lo[g + 1]], world.Q_ip, EF, K, H.FILL_BA, counters=True, sem=H.SEM_FUNCTOR))
    want = np_merge(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), lo[:-1], K, 0, H.FILL_BA)
    got = s.knn_batch_filtered(world.Q_ip, EF, K, world.half_ip, fill=H.FILL_BA, sem=H.SEM_FUNCTOR, counters=True)
    _same(got, want + (sum(r[2] for r in rows), sum(r[3] for r in rows), np.stack([r[4] for r in rows]).max(axis=0)), "IP")
    assert (got[1] < 0).any()                                   # negative distances: the order-preserving key is exercised


# ---- 3. the segment merge alone -----------------------------------------------------------------------------------------------------

def _segments(rng, n_lists, nq, max_len, only_list=None, equal_first=False):
    """per list lims / ids / dist: segments of 0 .. max_len entries, ascending under (distance, id), few distinct distances (negative
    ones too) so that ties across lists are common; first_row far apart, the upper half beyond 2^33"""
    values = np.array([-2.5, -1.0, -0.125, 0.0, 0.5, 0.5000001, 3.0, 1e30], np.float32)
    lims, ids, dist = [], [], []
    for g in range(n_lists):
        if only_list is not None:
            lens = np.full(nq, max_len if g == only_list else 0)
        else:
            kind = rng.integers(0, 4, size=nq)                  # 0: empty, 1: full, else ragged
            lens = np.where(kind == 0, 0, np.where(kind == 1, max_len, rng.integers(0, max_len + 1, size=nq)))
        lims.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        ids.append(np.concatenate([np.cumsum(rng.integers(1, 4, size=n)) - 1 for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32))
        dist.append(np.concatenate([np.sort(rng.choice(values, size=n)) for n in lens] + [np.zeros(0, np.float32)]).astype(np.float32))
    first = np.arange(n_lists, dtype=np.int64) * 5000 + np.where(np.arange(n_lists) >= (n_lists + 1) // 2, 2 ** 33, 0)
    if equal_first and n_lists > 1:
        first[1] = first[0]                                     # lists 0 and 1 number the same rows: equal global ids occur
    return lims, ids, dist, first


def np_merge_segments(lims, ids, dist, first):
    """the definition: per query every entry of every list under (distance, global id, list index); lims as the sum"""
    n_lists, nq = len(lims), len(lims[0]) - 1
    out_i, out_d = [], []
    for q in range(nq):
        gid = np.concatenate([first[g] + ids[g][lims[g][q]:lims[g][q + 1]].astype(np.int64) for g in range(n_lists)])
        dd = np.concatenate([dist[g][lims[g][q]:lims[g][q + 1]] for g in range(n_lists)])
        li = np.concatenate([np.full(lims[g][q + 1] - lims[g][q], g) for g in range(n_lists)])
        order = np.lexsort((li, gid, dd))
        out_i.append(gid[order])
        out_d.append(dd[order])
    return (np.sum(lims, axis=0).astype(np.int64), np.concatenate(out_i + [np.zeros(0, np.int64)]).astype(np.int64),
            np.concatenate(out_d + [np.zeros(0, np.float32)]).astype(np.float32))


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 70, 10), (3, 7, 0), (64, 16, 40), (5, 33, 3000), (64, 1, 5000)])
def test_merge_segments_operator(H, shape):
    n_lists, nq, max_len = shape
    rng = np.random.default_rng(1000 * n_lists + nq + max_len)
    cases = [dict(only_list=37)] if shape == (64, 1, 5000) else [dict(), dict(equal_first=True)] if shape == (2, 70, 10) else [dict()]
    for kw in cases:
        lims, ids, dist, first = _segments(rng, n_lists, nq, max_len, **kw)
        want = np_merge_segments(lims, ids, dist, first)
        r = H.merge_segments(lims, ids, dist, first, keep=True)
        try:
            assert r.size() == (nq, len(want[1]))
            got = r.fetch(counters=True)
        finally:
            r.release()
        _same(got[:3], want, "segments %s %s" % (shape, kw))
        assert all((c == 0).all() and c.dtype == np.uint32 for c in got[3:])     # the counters of such a result read as 0
        if kw.get("equal_first"):
            same = [np.intersect1d(first[0] + ids[0][lims[0][q]:lims[0][q + 1]], first[1] + ids[1][lims[1][q]:lims[1][q + 1]]).size for q in range(nq)]
            assert sum(same) > 0                                # (the same global id does occur in both lists)
    if shape == (5, 33, 3000):
        assert max(int(np.diff(l).max()) for l in lims) > 1024   # longer than any workgroup


def test_merge_segments_keeps_every_copy_of_an_entry(H):
    # the same (distance, global id) in three lists (the lower list's copy comes first): no copy is lost, none written twice
    lims = [np.array([0, 2]), np.array([0, 1]), np.array([0, 2])]
    ids = [np.array([4, 9]), np.array([4]), np.array([4, 9])]
    dist = [np.array([1.0, 2.0], np.float32), np.array([1.0], np.float32), np.array([1.0, 2.0], np.float32)]
    got = H.merge_segments(lims, ids, dist, [3, 3, 3])
    np.testing.assert_array_equal(got[0], [0, 5])
    np.testing.assert_array_equal(got[1], [7, 7, 7, 12, 12])
    np.testing.assert_array_equal(got[2], np.array([1, 1, 1, 2, 2], np.float32))


def test_merge_segments_orders_equal_distances_by_global_id(H):
    # What a single-index segment can hold where two pre-rounding keys gave one float distance: entries of one distance with the
    # higher id first.  The merged order is (distance, global id) there too, across the lists and inside one; the query beside it,
    # whose segments are in order, takes the merge's other path.
    lims = [np.array([0, 5, 8]), np.array([0, 3, 5]), np.array([0, 0, 0])]
    ids = [np.array([3, 9, 4, 2, 11, 1, 2, 3]), np.array([5, 1, 7, 0, 9]), np.zeros(0, np.int32)]
    dist = [np.array([0.5, 1.5, 1.5, 1.5, 2.0, 1.5, 1.5, 2.0], np.float32), np.array([1.5, 1.5, 1.5, 1.5, 2.0], np.float32), np.zeros(0, np.float32)]
    first = np.array([0, 4, 8], np.int64)
    want = np_merge_segments(lims, ids, dist, first)
    np.testing.assert_array_equal(want[1][:8], [3, 2, 4, 5, 9, 9, 11, 11])      # (list 1's 5, 1, 7 are the global rows 9, 5, 11)
    _same(H.merge_segments(lims, ids, dist, first), want, "descents")
    one = H.merge_segments(lims[:1], ids[:1], dist[:1], first[:1])              # one list: still put right
    _same(one, np_merge_segments(lims[:1], ids[:1], dist[:1], first[:1]), "descents, one list")
    np.testing.assert_array_equal(one[1], [3, 2, 4, 9, 11, 1, 2, 3])


# ---- 4. range search, exact form ------------------------------------------------------------------------------------------------------

def np_merge_ranges(parts, first):
    """per-shard fetches (lims, ids, dist, nd, nh, stage) -> the merged (lims, ids int64, dist, nd, nh, stage): per query the union
    under (distance, global id); counters summed, the stage the unsigned maximum"""
    lims, ids, dist = np_merge_segments([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], first)
    return (lims, ids, dist, sum(p[3] for p in parts), sum(p[4] for p in parts), np.stack([p[5] for p in parts]).max(axis=0))


def _check_range(H, s, Q, radius, ef, sem, mask, ctx):
    """a sharded range call (ef None: the exact form) against the merge of the single-index call on every shard handle under its
    slice of the mask -> (what the sharded call gave, the per-shard stages [G][nq])"""
    lo = _bounds(s)
    parts = []
    for g in range(s.num_shards()):
        part = None if mask is None else mask[lo[g]:lo[g + 1]]
        parts.append(H._range_search(s.shard(g)[0], Q, radius, ef, sem=sem, counters=True, filter=part))
    want = np_merge_ranges(parts, np.asarray(lo[:-1], np.int64))
    if ef is None:
        got = s.brute_force_range(Q, radius, filter=mask, counters=True)
    else:
        got = s.range_search(Q, radius, ef=ef, sem=sem, filter=mask, counters=True)
    _same(got, want, ctx)
    assert got[0][-1] == len(got[1]) == len(got[2]) and (got[2] <= radius).all(), ctx
    if mask is not None:
        assert mask[got[1] - s.id_base].all(), ctx
    return got, np.stack([p[5] for p in parts])


@pytest.mark.parametrize("G", [1, 3, 8])
def test_exact_range_is_the_merge_of_the_shards_segments(H, world, G):
    s = world.sharded(G)
    below, fifth, most = world.radii(0)
    for mask in (None, world.half):
        tag = "G %d mask %s" % (G, mask is not None)
        got, _ = _check_range(H, s, world.Q, below, None, 0, mask, tag + " below")
        assert got[0][-1] == 0                                  # below every distance: nq empty segments
        got, _ = _check_range(H, s, world.Q, fifth, None, 0, mask, tag + " fifth")
        assert 0 < got[0][-1] < 0.05 * NQ * N
        got, stages = _check_range(H, s, world.Q, most, None, 0, mask, tag + " most")
        share = got[0][-1] / (NQ * (N if mask is None else world.half.sum()))
        assert 0.5 < share < 0.7 and (stages == EXACT).all(), share
        got, _ = _check_range(H, s, world.Q[:3], np.inf, None, 0, mask, tag + " inf")
        n_all = N if mask is None else int(world.half.sum())
        np.testing.assert_array_equal(got[0], np.arange(4) * n_all)              # every allowed row, for each of the 3 queries
        if mask is None:
            np.testing.assert_array_equal(got[3], np.full(3, N, np.uint32))      # each row evaluated once, whatever the partition


def test_exact_range_inner_product(H, world):
    s = world.sharded(3, H.METRIC_IP)
    below, fifth, most = world.radii(1)
    got, _ = _check_range(H, s, world.Q_ip, fifth, None, 0, None, "IP fifth")
    assert got[0][-1] > 0 and (got[2] < 0).any()
    _check_range(H, s, world.Q_ip, most, None, 0, world.half_ip, "IP most masked")
    got, _ = _check_range(H, s, world.Q_ip, below, None, 0, None, "IP below")
    assert got[0][-1] == 0


def test_exact_range_on_integer_data_is_the_unsharded_scan(H):
    # values 0 .. 15 at d = 24: squared sums stay below 2^16, every distance is the root of an integer and two different keys never
    # round to one float, so ids and distance bits are those of one index over all rows
    rng = np.random.default_rng(9)
    X = rng.integers(0, 16, size=(1501, D)).astype(np.float32)
    Q = rng.integers(0, 16, size=(NQ, D)).astype(np.float32)
    mask = rng.random(1501) < 0.5
    s = H.ShardedHgraph.build(X, M, EFC, [0] * 3, seed=SEED)
    flat = H.Hgraph.flat(X)
    try:
        _, d5 = s.brute_force_knn(5, Q)
        for radius in (float(np.median(d5[:, 4])), 33.0, np.inf):
            for m in (None, mask):
                lims, ids, dist = s.brute_force_range(Q, radius, filter=m)
                fl, fi, fd = H.Ohnsw.brute_force_range(flat, radius, Q, filter=m)
                _same((lims, ids, dist), (fl, fi.astype(np.int64), fd), "integer data radius %s mask %s" % (radius, m is not None))
                assert lims[-1] > 0
        lims, ids, dist = s.brute_force_range(Q, 33.0)
        assert 0.3 < lims[-1] / (NQ * 1501) < 0.9 and (np.diff(dist) == 0).mean() > 0.3     # a large share of rows, full of equal distances
    finally:
        s.release()
        flat.release()


# ---- 5. range search, graph form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 3, 8])
def test_graph_range_is_the_merge_of_the_shards_segments(H, world, G):
    s = world.sharded(G)
    below, fifth, most = world.radii(0)
    for sem in (H.SEM_OHNSW, H.SEM_FUNCTOR):
        for mask in (None, world.half):
            tag = "G %d sem %d mask %s" % (G, sem, mask is not None)
            got, st_below = _check_range(H, s, world.Q, below, 16, sem, mask, tag + " below")
            assert got[0][-1] == 0 and (st_below == 0).all()    # W of 16 is not saturated: the ladder's first stage serves everyone
            _check_range(H, s, world.Q, fifth, 16, sem, mask, tag + " fifth")
            got, st_most = _check_range(H, s, world.Q, most, 16, sem, mask, tag + " most")
            assert (st_most > 0).mean() > 0.5                   # hundreds of rows in range per shard: W of 16 is saturated
            if G == 1:
                # one shard of 5003 rows with about 3000 in range: W is still saturated at 1024 members, so the exact stage answers.
                # (With 3 or 8 shards a shard holds at most 1668 rows, about 1000 in range: its W of 1024 is never saturated.)
                assert (st_most == EXACT).any(), "the 60 % radius no longer reaches the exact stage"


def test_graph_range_inner_product(H, world):
    s = world.sharded(3, H.METRIC_IP)
    _, fifth, most = world.radii(1)
    got, _ = _check_range(H, s, world.Q_ip, fifth, 16, H.SEM_FUNCTOR, world.half_ip, "IP graph fifth masked")
    _check_range(H, s, world.Q_ip, most, 16, H.SEM_OHNSW, None, "IP graph most")


# ---- 6. errors and lifetime -------------------------------------------------------------------------------------------------------------

def test_errors(H, world):
    L = H.load()
    s = world.sharded(3)
    f = s.filter(world.half)
    try:
        for call in (lambda: s.range_search(world.Q, np.nan, ef=16), lambda: s.brute_force_range(world.Q, np.nan),
                     lambda: s.range_search(world.Q, np.nan, ef=16, filter=f), lambda: s.brute_force_range(world.Q, np.nan, filter=f)):
            with pytest.raises(H.InvalidArgument, match="NaN"):
                call()
        with pytest.raises(H.InvalidArgument):
            s.range_search(world.Q, 1.0, ef=16, sem=H.SEM_FUNCTOR_NEAREST_K)
        with pytest.raises(H.InvalidArgument):
            s.knn_batch_filtered(world.Q, EF, K, f, sem=H.SEM_FUNCTOR_NEAREST_K)
        with pytest.raises(H.InvalidArgument):
            s.range_search(world.Q, 1.0, ef=0)
        with pytest.raises(H.Failure):
            s.range_search(world.Q, 1.0, ef=1025)
        with pytest.raises(H.InvalidArgument):
            s.knn_batch_filtered(world.Q, 8, K, f)              # k > ef
        out = ctypes.c_void_p(1)                                # an error leaves *out NULL
        rp = H._RangeParams(float("nan"), 16, 0)
        assert L.hnsw_sharded_range_search_batch(s.handle, None, H._ptr(world.Q), NQ, D, ctypes.byref(rp), ctypes.byref(out)) == H.ERR_BAD_ARG
        assert out.value is None
        # nq == 0: a no-op for the k-NN call, a valid empty result for the range calls
        none = np.zeros((0, D), np.float32)
        ids, dist = s.knn_batch_filtered(none, EF, K, f)
        assert ids.shape == (0, K) and dist.shape == (0, K)
        for res in (s.range_search(none, 1.0, ef=16, keep=True), s.brute_force_range(none, 1.0, filter=f, keep=True)):
            assert res.size() == (0, 0)
            lims, ri, rd, nd, nh, st = res.fetch(counters=True)
            np.testing.assert_array_equal(lims, [0])
            assert len(ri) == len(rd) == len(nd) == len(nh) == len(st) == 0
            res.release()
    finally:
        f.release()


def test_results_own_their_buffers(H, world):
    s = H.ShardedHgraph.build(world.X[:600], M, EFC, [0] * 2, seed=SEED)
    try:
        _, d5 = s.brute_force_knn(5, world.Q)
        radius = float(np.median(d5[:, 4]))
        a = s.brute_force_range(world.Q, radius, keep=True)     # two results alive at once
        b = s.range_search(world.Q, radius, ef=16, keep=True)
        fa, fb = a.fetch(counters=True), b.fetch(counters=True)
        assert fa[0][-1] > 0 and fb[0][-1] > 0 and all(p != 0 for p in a.device_pointers() + b.device_pointers())
        assert set(a.device_pointers()).isdisjoint(b.device_pointers())
    finally:
        s.release()
    _same(a.fetch(counters=True), fa, "after release() of the sharded index")
    _same(b.fetch(counters=True), fb, "after release() of the sharded index")
    a.release()
    b.release()
    with pytest.raises(H.InvalidArgument):
        a.fetch()


# ---- 7. the C++ front end ---------------------------------------------------------------------------------------------------------------

def test_cpp_front_end_sharded_query(H):
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_front_sharded_query")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sharded query front-end ok" in out.stdout, out.stdout + out.stderr
