"""The three synchronous host-buffer entry points (hnsw_search_batch, hnsw_brute_force_batch, hnsw_rerank_batch) give the same
bits wherever the caller's matrices live: every combination of pageable and page-locked (H.host_empty) query matrix, result pair
and -- for the re-rank -- candidate matrix against the all-pageable call, at batch sizes on both sides of the small block's
32768-byte bound (d = 24: 1 and 64 queries inside it, 400 queries = 38400 bytes of queries above it).  No oracle, no tolerance."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M, EF, K, CAND = 4000, 24, 8, 32, 5, 16
BATCHES = [1, 64, 400]


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    if H.device_count() < 1:
        pytest.skip("no HIP device")
    return H


@pytest.fixture(scope="module")
def case(H):
    """the index, the queries, and per batch size the all-pageable answers: knn with counters, exact scan, candidates and re-rank"""
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((max(BATCHES), D)).astype(np.float32)
    hg = H.Ohnsw.build_batch_bigarray(X, M, 40, seed=3)
    ref = {}
    for nq in BATCHES:
        q = Q[:nq].copy()
        cand = H.Ohnsw.knn_batch_bigarray(hg, CAND, q, ef=EF)[0]
        ref[nq] = {"knn": H.Ohnsw.knn_batch_bigarray(hg, K, q, ef=EF, counters=True),
                   "scan": H.Ohnsw.brute_force_knn(hg, K, q), "cand": cand, "rerank": H.Ohnsw.rerank(hg, K, q, cand)}
        assert (ref[nq]["knn"][0] >= 0).all() and (ref[nq]["knn"][2] > 0).all()
    yield hg, Q, ref
    hg.release()


def _placed(H, a, locked):
    """a copy of `a` in pageable or page-locked memory"""
    if not locked:
        return a.copy()
    b = H.host_empty(a.shape, a.dtype)
    b[...] = a
    return b


def _out(H, nq, locked):
    """a result pair to write into, prefilled with what no search returns"""
    ids, dist = _placed(H, np.full((nq, K), -7, np.int32), locked), _placed(H, np.full((nq, K), -1.0, np.float32), locked)
    return ids, dist


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))


@pytest.mark.parametrize("nq", BATCHES)
def test_knn_placements(H, case, nq):
    hg, Q, ref = case
    want = ref[nq]["knn"]
    for q_locked, out_locked, counters in itertools.product((False, True), (False, True), (False, True)):
        out = _out(H, nq, out_locked)
        got = H.Ohnsw.knn_batch_bigarray(hg, K, _placed(H, Q[:nq], q_locked), ef=EF, counters=counters, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _same(got, want)
        if counters:
            np.testing.assert_array_equal(got[2], want[2])
            np.testing.assert_array_equal(got[3], want[3])


@pytest.mark.parametrize("nq", BATCHES)
def test_brute_force_placements(H, case, nq):
    hg, Q, ref = case
    for q_locked, out_locked in itertools.product((False, True), (False, True)):
        out = _out(H, nq, out_locked)
        got = H.Ohnsw.brute_force_knn(hg, K, _placed(H, Q[:nq], q_locked), out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _same(got, ref[nq]["scan"])


@pytest.mark.parametrize("nq", BATCHES)
def test_rerank_placements(H, case, nq):
    hg, Q, ref = case
    for q_locked, cand_locked, out_locked in itertools.product((False, True), (False, True), (False, True)):
        out = _out(H, nq, out_locked)
        got = H.Ohnsw.rerank(hg, K, _placed(H, Q[:nq], q_locked), _placed(H, ref[nq]["cand"], cand_locked), out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _same(got, ref[nq]["rerank"])
