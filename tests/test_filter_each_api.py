"""CPU-side checks of the per-query form of filtered search and of filters made from labels (ocaml-hnsw_amd/csrc/hnsw_filter.hip):
hnsw_search_batch_filtered_each, hnsw_filter_create_by_label and hnsw_filter_bits exist in the library and in every front end, the
header states their definitions, and the layout of the exact stage (hnsw_filter_plan.h) keeps what the masked scan relies on."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_search_batch_filtered_each", "hnsw_filter_create_by_label", "hnsw_filter_bits")
ARITY = (13, 5, 2)


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
        decl = hdr[hdr.index("int32_t %s(" % name):]
        assert decl[:decl.index(";")].count(",") + 1 == arity, name      # the header's own argument list
    assert callable(H.Ohnsw.knn_batch_filtered_each) and callable(H.Ba.knn_batch_filtered_each)
    assert callable(H.Hgraph.filters_by_label) and callable(H.Filter.bits)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let filters_by_label ", "let filter_bits ", "let knn_batch_filtered_each "):
        assert wrapper in ml, wrapper
    assert "by_label(" in hpp and "bits()" in hpp and "knn_filtered_each(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_filter_each.cpp"))


def test_header_states_the_definitions():
    hdr = _header()
    para = hdr[hdr.index("THE RESULT of hnsw_search_batch_filtered_each"):]
    para = para[:para.index("*/")]
    for needle in ("filters[query_filter[q]]", "bit for bit", "DETERMINISM", "the query's filter", "n_allowed < k", "0xFFFFFFFF",
                   "out_nhops 0", "not affected", "LADDER", "ONE compacted batch", "ascending", "EXACT STAGE",
                   "n_allowed of the query's own filter", "ERRORS", "outputs untouched", "before any launch", "n_filters < 1",
                   "ANY entry", "whether or not a query names it", "0 .. n_filters - 1", "HNSW_ERR_UNSUPPORTED",
                   "HNSW_SEM_FUNCTOR_NEAREST_K", "HNSW_ERR_EMPTY_INDEX", "query_filter may be null", "appear twice",
                   "no upper limit on n_filters", "ONE filtered call in flight",
                   # filters from labels
                   "FILTERS FROM LABELS", "labels[v] == l", "-1 .. n_labels - 1", "in no filter", "before anything is allocated",
                   "All or nothing", "all NULL", "hnsw_filter_destroy", "hnsw_filter_count", "count 0",
                   "n_labels * ceil(n / 32) * 4 bytes", "NOT counted in hnsw_index_info.device_bytes",
                   # the mask back on the host
                   "hnsw_filter_bits", "ceil(n / 32) words", "bits past n clear"):
        assert needle in para, needle


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 10, 0, 0)
    assert L.hnsw_search_batch_filtered_each(None, None, 1, None, None, 0, 0, ctypes.byref(p), None, None, None, None, None) == H.ERR_BAD_ARG
    out = (ctypes.c_void_p * 3)(1, 2, 3)
    assert L.hnsw_filter_create_by_label(None, None, 0, 3, out) == H.ERR_BAD_ARG
    assert [out[i] for i in range(3)] == [None, None, None]      # all or nothing: every entry NULL
    assert L.hnsw_filter_create_by_label(None, None, 0, 3, None) == H.ERR_BAD_ARG
    out1 = (ctypes.c_void_p * 1)(7)
    assert L.hnsw_filter_create_by_label(None, None, 0, 0, out1) == H.ERR_BAD_ARG      # n_labels < 1: nothing of out is touched
    word = ctypes.c_uint32(5)
    assert L.hnsw_filter_bits(None, ctypes.byref(word)) == H.ERR_BAD_ARG and word.value == 5
    assert L.hnsw_filter_bits(None, None) == H.ERR_BAD_ARG


def test_filter_plan_keeps_tiles_within_one_filter(tmp_path):
    """filter_plan (the exact stage's rows by (filter, query), each filter's group padded to whole scan tiles) over a grid of batch
    sizes, filter counts, tiles and assignments: tests/cpp/test_filter_plan.cpp, a host program, under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_filter_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_filter_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"filter plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
