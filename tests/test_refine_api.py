"""The re-rank operator and option "refine" at the drop-in boundary, without a device: the library exports
hnsw_rerank_batch / hnsw_rerank_batch_device, the Python, OCaml and C++ fronts name them, and the host-side checks
refuse bad arguments before anything touches a device."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


SYMBOLS = ("hnsw_rerank_batch", "hnsw_rerank_batch_device")


def test_library_exports_the_rerank_symbols(H):
    L = H.load()
    for s in SYMBOLS:
        assert s in H.ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert len(L.hnsw_rerank_batch.argtypes) == 10 and len(L.hnsw_rerank_batch_device.argtypes) == 11
    assert L.hnsw_abi_version() == 3           # added entry points do not bump it


def test_python_front_has_rerank(H):
    assert callable(H.Ohnsw.rerank) and callable(H.rerank_device)


def test_ocaml_binds_and_wraps_rerank():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    for s in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % s, ml), s
    assert "let rerank " in ml


def test_cpp_front_has_rerank():
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert re.search(r"\brerank\(const Hgraph &", hpp) and "hnsw_rerank_batch(" in hpp


def test_header_documents_operator_and_option():
    hdr = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert '"refine"' in hdr and "hnsw_rerank_batch_device" in hdr
    build = open(os.path.join(ROOT, "ocaml-hnsw_amd", "build.py")).read()
    assert '"hnsw_rerank.hip"' in build


def test_null_index_is_refused(H):
    L = H.load()
    assert L.hnsw_rerank_batch(None, None, 1, 1, None, 4, 2, 0, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_rerank_batch_device(None, None, 1, 1, None, 4, 2, 0, None, None, None) == H.ERR_BAD_ARG
