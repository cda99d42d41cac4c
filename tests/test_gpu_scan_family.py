"""The exact scans are one family (ocaml-hnsw_amd/csrc/hnsw_scan_device.hip.h): the k-scan (hnsw_brute_force_batch), its masked
form (hnsw_search_batch_filtered's exact stage) and the range scan (hnsw_range_brute_force_batch) walk the rows with one body and
differ in what they keep.  Held here: the three compute ONE order -- the same ids, the same distance bits -- on the smallest shapes
that take every path of the body, and the ladder the filtered and the range search share carries nothing from one call to the
next.  Each scan alone is held against the oracle in test_gpu_brute_force.py, test_gpu_filter.py and test_gpu_range.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT = 0xFFFFFFFF
INF = float("inf")
SCAN_N, SCAN_NQ = 517, 9        # as in test_gpu_range.py: n is no multiple of 4 * UB for any NCH, nq is a full tile plus one
ALLOWED = [0, 31, 32, 258, 259, 484, 516]       # 7 < k: first, middle and last rows, both sides of a mask word's edge


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _floats(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _three_scans_agree(H, hg, Q, ctx):
    n = SCAN_N
    mask = np.zeros(n, bool)
    mask[ALLOWED] = True
    for slabs in (1, 3):
        hg.set_option("scan_slabs", slabs)
        c = "%s slabs %d" % (ctx, slabs)
        # 1. the k-scan with k = n against the range scan with every row in range
        ids, dist = H.Ohnsw.brute_force_knn(hg, n, Q)
        lims, rids, rdist = H.Ohnsw.brute_force_range(hg, INF, Q)
        np.testing.assert_array_equal(lims, np.arange(len(Q) + 1) * n, err_msg=c)
        np.testing.assert_array_equal(rids.reshape(len(Q), n), ids, err_msg=c + " k-scan ids")
        np.testing.assert_array_equal(_bits(rdist).reshape(len(Q), n), _bits(dist), err_msg=c + " k-scan distance bits")
        # 2. the masked scan (7 allowed nodes < k: no walk, the exact stage at once) against the range segment's allowed members
        fids, fdist, _, _, stage = H.Ohnsw.knn_batch_filtered(hg, 10, Q, mask, ef=16, counters=True)
        assert (stage == EXACT).all(), c
        keep = mask[rids]
        np.testing.assert_array_equal(fids[:, :7], rids[keep].reshape(len(Q), 7), err_msg=c + " masked ids")
        np.testing.assert_array_equal(_bits(fdist[:, :7]), _bits(rdist[keep].reshape(len(Q), 7)), err_msg=c + " masked distance bits")
        assert (fids[:, 7:] == -1).all() and np.isnan(fdist[:, 7:]).all(), c      # the fill
    hg.set_option("scan_slabs", 0)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [3, 100, 200, 300, 600])       # NCH 1, 2, 4, 8 (the tile in LDS), 16
def test_three_scans_one_order(H, d, metric):
    X, Q = _floats(SCAN_N, d, 500 + d), _floats(SCAN_NQ, d, 501 + d)
    hg = H.Hgraph.flat(X, metric=metric)
    assert hg.info().row_format in (0, 3)                     # float32 rows, or their split layout (d 100, 200): no compact copy
    _three_scans_agree(H, hg, Q, "d %d metric %d" % (d, metric))
    hg.release()


def test_three_scans_one_order_on_a_built_graph(H):
    X, Q = _floats(SCAN_N, 100, 600), _floats(SCAN_NQ, 100, 601)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    _three_scans_agree(H, hg, Q, "built graph")
    hg.release()


def test_shared_ladder_carries_nothing_over(H):
    """A range search, a filtered search and the range search again on one handle: both ladders escalate some but not all queries,
    so their short lists are not contiguous, and they run through the same scratch."""
    n, d, nq = 2003, 20, 64
    X, Q = _floats(n, d, 1), _floats(nq, d, 2)
    hg = H.Ohnsw.build_batch_bigarray(X, 8, 40, seed=7)
    # a radius that saturates W_16 for about half of the queries: the median distance of the 16th neighbour
    radius = float(np.median(H.Ohnsw.brute_force_knn(hg, 16, Q)[1][:, 15]))
    mask = np.random.default_rng(20).random(n) < 0.1         # test_gpu_filter.py's LADDER_MASK_SEED: stages 0, 1 and later ones

    def short_list_is_not_contiguous(stage):        # after some stage j of the ladder (the exact stage's number is above all)
        shorts = [np.flatnonzero(stage > j) for j in range(11)]
        return any(0 < len(s) < nq and (np.diff(s) > 1).any() for s in shorts)

    f0 = H.Ohnsw.knn_batch_filtered(hg, 10, Q, mask, ef=16, counters=True)
    r1 = H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True)
    f1 = H.Ohnsw.knn_batch_filtered(hg, 10, Q, mask, ef=16, counters=True)
    r2 = H.Ohnsw.range_search(hg, radius, Q, ef=16, counters=True)
    print("range stages %s, filtered stages %s" % (np.unique(r1[5], return_counts=True), np.unique(f1[4], return_counts=True)))
    assert short_list_is_not_contiguous(r1[5]) and short_list_is_not_contiguous(f1[4])
    assert len(r1[1]) > 0
    for a, b in zip(list(r1) + list(f0), list(r2) + list(f1)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    hg.release()
