"""CPU-side checks of filtered search (ocaml-hnsw_amd/csrc/hnsw_filter.hip): the filter object's entry points and the search exist
in the library and in every front end, the header states the result's definition, and the Python side packs a mask's bits as the
C ABI reads them."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_filter_create", "hnsw_filter_destroy", "hnsw_filter_count", "hnsw_search_batch_filtered")
ARITY = (4, 1, 2, 11)


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def test_symbols_are_declared_exported_and_mirrored(H):
    L = H.load()
    hdr = _header()
    for name, arity in zip(SYMBOLS, ARITY):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32
    assert "typedef struct hnsw_filter hnsw_filter;" in hdr
    assert callable(H.Hgraph.filter) and callable(H.Ohnsw.knn_batch_filtered) and callable(H.Ba.knn_batch_filtered)
    assert callable(H.Filter.count) and callable(H.Filter.release)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let filter_create ", "let filter_count ", "let knn_batch_filtered "):
        assert wrapper in ml, wrapper
    assert "class Filter" in hpp and "knn_filtered(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_filter.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    para = hdr[hdr.index("THE RESULT of hnsw_search_batch_filtered"):]
    para = para[:para.index("*/")]
    for needle in ("LADDER", "e_{j+1} = min(1024, 2 * e_j)", "|A_{e_j}(q)| >= k", "compacted batch",
                   "EXACT STAGE", "n_allowed < k", "hnsw_brute_force_batch", "(distance, node id)",
                   "ALWAYS OVER THE FLOAT32 ROWS", "hnsw_distance_batch", "HNSW_ROWS_HALF", "HNSW_ROWS_SQ8", "id_base - 1",
                   '"refine" does not shorten', "0xFFFFFFFF", "out_nhops", "out_ndist", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "HNSW_ERR_EMPTY_INDEX", "HNSW_ERR_UNSUPPORTED", "DETERMINISM", "ONE filtered call in flight"):
        assert needle in para, needle
    obj = hdr[hdr.index("THE FILTER."):hdr.index("THE RESULT of hnsw_search_batch_filtered")]
    for needle in ("ceil(n_bits / 32)", "(v & 31)", "(v >> 5)", "whatever id_base is", "positions >= n", "hnsw_index_insert",
                   "another handle", "NOT counted in hnsw_index_info.device_bytes", "not saved"):
        assert needle in obj, needle


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    out = ctypes.c_void_p()
    c = ctypes.c_int64(7)
    assert L.hnsw_filter_create(None, None, 0, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_filter_create(None, None, 0, None) == H.ERR_BAD_ARG
    assert L.hnsw_filter_count(None, ctypes.byref(c)) == H.ERR_BAD_ARG and c.value == 7
    assert L.hnsw_filter_destroy(None) == H.OK
    p = H._SearchParams(16, 10, 0, 0)
    assert L.hnsw_search_batch_filtered(None, None, None, 0, 0, ctypes.byref(p), None, None, None, None, None) == H.ERR_BAD_ARG


def _words_by_hand(mask):
    w = np.zeros((len(mask) + 31) // 32, np.uint32)
    for v in np.flatnonzero(mask):
        w[v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    return w


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 70, 2003])
def test_bit_packing(H, n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.37
    mask[n - 1] = True                                          # the last node: the highest bit in use
    want = _words_by_hand(mask)
    got = H.pack_allow(mask, n)
    assert got.dtype == np.uint32 and got.shape == ((n + 31) // 32,)
    np.testing.assert_array_equal(got, want)
    if n % 32:
        assert int(got[-1]) >> (n % 32) == 0                    # nothing set past n
    ids = np.flatnonzero(mask)
    for id_base in (0, 1):
        for arr in (ids + id_base, (ids + id_base).astype(np.int32)[::-1], list(ids + id_base) + [int(ids[0]) + id_base]):
            np.testing.assert_array_equal(H.pack_allow(arr, n, id_base), want)
    np.testing.assert_array_equal(H.pack_allow(np.zeros(0, np.int64), n), np.zeros((n + 31) // 32, np.uint32))
    np.testing.assert_array_equal(H.pack_allow(np.ones(n, bool), n), _words_by_hand(np.ones(n, bool)))


def test_bit_packing_refuses_what_is_not_a_mask(H):
    with pytest.raises(H.InvalidArgument):
        H.pack_allow(np.ones(9, bool), 10)                      # a boolean mask of another length
    with pytest.raises(H.InvalidArgument):
        H.pack_allow([10], 10)                                  # an id past the last node
    with pytest.raises(H.InvalidArgument):
        H.pack_allow([0], 10, id_base=1)                        # ... below the first
    with pytest.raises(H.InvalidArgument):
        H.pack_allow(np.array([0.5]), 10)                       # not integers
