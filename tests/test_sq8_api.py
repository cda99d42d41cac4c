"""CPU-side checks of option "sq8_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_sq8.hip): the two introspection entry points exist in the
library and in every front end, the row format has its number, the header states the contract."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_sq8_params", "hnsw_index_sq8_codes")


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def test_symbols_are_exported_and_mirrored(H):
    L = H.load()
    for name, arity in zip(SYMBOLS, (3, 2)):
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, _header())
    assert callable(H.Hgraph.sq8_params) and callable(H.Hgraph.sq8_codes)
    assert L.hnsw_abi_version() == 3                       # additive entry points: the version stays


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    lo, s = ctypes.c_float(0), ctypes.c_float(0)
    assert L.hnsw_index_sq8_params(None, ctypes.byref(lo), ctypes.byref(s)) == H.ERR_BAD_ARG
    assert L.hnsw_index_sq8_codes(None, None) == H.ERR_BAD_ARG


def test_row_format_number(H):
    assert H.ROWS_SQ8 == 5
    assert re.search(r"\bHNSW_ROWS_SQ8\s*=\s*5\b", _header())
    assert (H.ROWS_F32, H.ROWS_BYTES, H.ROWS_SPLIT, H.ROWS_HALF) == (0, 2, 3, 4)


def test_header_documents_the_option():
    hdr = _header()
    para = hdr[hdr.index('"sq8_rows"      '):]
    para = para[:para.index("*/")]
    for needle in ("rint((x - lo) / s)", "ties to even", "s = 1 when hi == lo", "q' = (q - lo) / s", "q' = q", "min(ef, max(k, R))",
                   "HNSW_ERR_UNSUPPORTED", "HNSW_SEM_FUNCTOR_NEAREST_K", "hnsw_index_insert", "device_bytes", "Not saved",
                   "hnsw_index_sq8_params", "64 * NCH", "half_rows", "byte_rows"):
        assert needle in para, needle
    # the refine paragraph no longer says it does nothing for every other format
    refine = hdr[hdr.index('"refine"        '):]
    assert "sq8" in refine[:refine.index("*/")]


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert '"%s"' % name in ml and name in hpp
    assert "rows_sq8 = 5l" in ml and "HNSW_ROWS_SQ8" in hpp
