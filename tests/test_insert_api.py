"""hnsw_index_insert's interface on every front end (no device needed): the header declares it, the library exports it,
the Python, OCaml and C++ fronts wrap it, and without a device the call fails loudly."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    return H


def test_header_declares_insert():
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert re.search(r"int32_t hnsw_index_insert\(hnsw_index \*idx, const float \*vectors, int64_t m, int64_t row_stride,\s*"
                     r"const hnsw_build_params \*params\);", hdr)
    assert re.search(r"#define HNSW_ABI_VERSION 3\b", hdr)


def test_python_front_binds_insert(H):
    assert "hnsw_index_insert" in H.ABI_SYMBOLS
    assert callable(H.Ohnsw.insert_batch)
    L = H.load()
    assert L.hnsw_index_insert.restype is not None and len(L.hnsw_index_insert.argtypes) == 5


def test_ocaml_and_cpp_fronts_wrap_insert():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    assert re.search(r'foreign[^"]*"hnsw_index_insert"', ml)
    assert "let insert_batch " in ml
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert "hnsw_index_insert(" in hpp and "inline int64_t insert(" in hpp


def test_insert_fails_loudly_without_device(H):
    if H.device_count() > 0:
        pytest.skip("a device is present")
    X = np.zeros((4, 8), np.float32)
    hg = H.Hgraph(X, np.zeros(4, np.int32), np.full((4, 4), -1, np.int32), entry_point=0)
    with pytest.raises(H.Failure, match="no HIP device"):
        H.Ohnsw.insert_batch(hg, np.ones((2, 8), np.float32), 2, 10)


def test_insert_checks_the_batch_shape_on_the_host(H):
    X = np.zeros((4, 8), np.float32)
    hg = H.Hgraph(X, np.zeros(4, np.int32), np.full((4, 4), -1, np.int32), entry_point=0)
    with pytest.raises(H.InvalidArgument, match="index's d"):
        H.Ohnsw.insert_batch(hg, np.ones((2, 7), np.float32), 2, 10)
