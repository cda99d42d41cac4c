"""hnsw_brute_force_batch's interface on every front end (no device needed): the header declares it, the library exports it,
the Python, OCaml and C++ fronts wrap it, without a device the call fails loudly, and dataset.brute_force_knn_l2 without a
device is what it was."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    return H


def test_header_declares_brute_force():
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert re.search(r"int32_t hnsw_brute_force_batch\(hnsw_index \*idx, const float \*queries, int64_t nq, int64_t q_stride,\s*"
                     r"int32_t k, int32_t fill, int32_t \*out_ids, float \*out_dist\);", hdr)
    assert re.search(r"int32_t hnsw_brute_force_batch_device\(hnsw_index \*idx, const float \*d_queries, int64_t nq, int64_t q_stride,\s*"
                     r"int32_t k, int32_t fill, int32_t \*d_ids, float \*d_dist, void \*stream\);", hdr)
    assert re.search(r"#define HNSW_ABI_VERSION 3\b", hdr)


def test_python_front_binds_brute_force(H):
    assert "hnsw_brute_force_batch" in H.ABI_SYMBOLS and "hnsw_brute_force_batch_device" in H.ABI_SYMBOLS
    assert callable(H.Ohnsw.brute_force_knn) and callable(H.brute_force_device) and callable(H.Hgraph.flat)
    L = H.load()
    assert L.hnsw_brute_force_batch.restype is not None and len(L.hnsw_brute_force_batch.argtypes) == 8
    assert L.hnsw_brute_force_batch_device.restype is not None and len(L.hnsw_brute_force_batch_device.argtypes) == 9


def test_ocaml_and_cpp_fronts_wrap_brute_force():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    assert re.search(r'foreign[^"]*"hnsw_brute_force_batch"', ml)
    assert re.search(r'foreign[^"]*"hnsw_brute_force_batch_device"', ml)
    assert "let brute_force_knn_l2 " in ml and "let brute_force_knn " in ml
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert "hnsw_brute_force_batch(" in hpp and " brute_force_knn(" in hpp


def test_flat_graph_has_no_edges(H):
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    hg = H.Hgraph.flat(X, metric=H.METRIC_IP, id_base=1)
    assert (hg.n, hg.d, hg.max_degree0, hg.max_layer, hg.entry_point, hg.id_base, hg.metric) == (4, 3, 1, 0, 1, 1, H.METRIC_IP)
    assert not hg.deg0.any() and (hg.nbr0 == -1).all()
    assert H.Hgraph.flat(np.zeros((0, 3), np.float32)).entry_point is None


def test_brute_force_fails_loudly_without_device(H):
    if H.device_count() > 0:
        pytest.skip("a device is present")
    hg = H.Hgraph.flat(np.zeros((4, 8), np.float32))
    with pytest.raises(H.Failure, match="no HIP device"):
        H.Ohnsw.brute_force_knn(hg, 2, np.ones((2, 8), np.float32))


def test_brute_force_checks_the_batch_shape_on_the_host(H):
    hg = H.Hgraph.flat(np.zeros((4, 8), np.float32))
    with pytest.raises(H.InvalidArgument, match=r"\[nq\]\[d\]"):
        H.Ohnsw.brute_force_knn(hg, 2, np.ones((2, 7), np.float32))


def _brute_force_knn_l2_before(train, test, k, block=256):
    """the body of dataset.brute_force_knn_l2 as it was before it gained `device`"""
    train = np.ascontiguousarray(train, np.float32)
    test = np.ascontiguousarray(test, np.float32)
    tn = (train.astype(np.float64) ** 2).sum(1)
    out = np.empty((test.shape[0], k), np.float32)
    for s in range(0, test.shape[0], block):
        q = test[s:s + block].astype(np.float64)
        d2 = tn[None, :] - 2.0 * (q @ train.T.astype(np.float64)) + (q ** 2).sum(1)[:, None]
        part = np.partition(d2, min(k, d2.shape[1]) - 1, axis=1)[:, :k]
        out[s:s + block] = np.sqrt(np.maximum(np.sort(part, axis=1), 0)).astype(np.float32)
    return out


def test_dataset_route_without_device_is_unchanged():
    import inspect
    from ocaml_hnsw_amd import dataset
    rng = np.random.default_rng(5)
    train = rng.uniform(-1, 1, size=(700, 24)).astype(np.float32)
    test = rng.uniform(-1, 1, size=(300, 24)).astype(np.float32)
    for k, block in ((1, 256), (10, 256), (10, 7)):
        want = _brute_force_knn_l2_before(train, test, k, block)
        np.testing.assert_array_equal(dataset.brute_force_knn_l2(train, test, k, block=block, device=None).view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(dataset.brute_force_knn_l2(train, test, k, block).view(np.uint32), want.view(np.uint32))
    for f in (dataset.brute_force_knn_l2, dataset.Dataset.random, dataset.Dataset.read_texmex):
        assert inspect.signature(f).parameters["device"].default is None
    ds = dataset.Dataset.random(8, 50, 5, 3, seed=2)
    np.testing.assert_array_equal(ds.test_distances.view(np.uint32), _brute_force_knn_l2_before(ds.train, ds.test, 3).view(np.uint32))


def test_scan_plan_is_the_arithmetic_it_replaced(tmp_path):
    """scan_plan (the cut of the k-scan and of the range scan into pieces and slabs) against the two loops it replaced, over a grid
    of (n, m, k, scan_slabs): tests/cpp/test_scan_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    import subprocess
    exe = str(tmp_path / "test_scan_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_scan_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"scan plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
