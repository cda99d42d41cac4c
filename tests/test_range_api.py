"""CPU-side checks of range search (ocaml-hnsw_amd/csrc/hnsw_range.hip): the six entry points exist in the library and in every
front end with the header's arity, the header states the result's definition, and what can be refused without a device is."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_range_search_batch", "hnsw_range_brute_force_batch", "hnsw_range_result_size", "hnsw_range_result_fetch",
           "hnsw_range_result_device", "hnsw_range_result_destroy")
ARITY = (6, 6, 3, 7, 4, 1)


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
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, arity in zip(SYMBOLS, ARITY):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;{]*?)\)\s*;" % name, bare, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32
    assert L.hnsw_range_brute_force_batch.argtypes[4] is ctypes.c_float             # the radius travels by value
    assert "typedef struct hnsw_range_result hnsw_range_result;" in hdr
    body = re.search(r"typedef struct hnsw_range_params \{(.*?)\} hnsw_range_params;", bare, flags=re.S).group(1)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == ["radius", "ef", "semantics"] == [f for f, _ in H._RangeParams._fields_]
    assert ctypes.sizeof(H._RangeParams) == 12
    assert callable(H.Ohnsw.range_search) and callable(H.Ohnsw.brute_force_range) and callable(H.Ba.range_search)
    assert callable(H.RangeResult.size) and callable(H.RangeResult.fetch) and callable(H.RangeResult.release)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let range_search ", "let brute_force_range "):
        assert wrapper in ml, wrapper
    assert re.findall(r'field range_params "([a-z_0-9]+)"', ml) == ["radius", "ef", "semantics"]      # header order
    assert "class RangeResult" in hpp and "range_search(" in hpp and "brute_force_range(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_range.cpp"))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"test_front_range"' in entry                        # build() compiles the driver
    build = open(os.path.join(ROOT, "ocaml-hnsw_amd", "build.py")).read()
    assert '"hnsw_range.hip"' in build


def test_header_states_the_definition():
    hdr = _header()
    para = hdr[hdr.index("THE RESULT of the range calls"):]
    para = para[:para.index("*/")]
    for needle in ("IN RANGE", "<= radius", "hnsw_distance_batch", "1 - <a,b>", "are a prefix", "NaN radius is HNSW_ERR_BAD_ARG",
                   "lims[q + 1] == lims[q]", "+inf gives everything",
                   "ORDER", "hnsw_brute_force_batch", "(distance, node id)", "id_base-based", "ALWAYS OVER THE FLOAT32 ROWS",
                   "in-range prefix of the full order over all n rows", "n = 0 gives HNSW_OK",
                   "LADDER", "e_{j+1} = min(1024, 2 * e_j)", "not saturated", "|W| < e_j", "> radius", "compacted batch",
                   "ascending query", "never modified",
                   "HNSW_ROWS_HALF", "HNSW_ROWS_SQ8", "k := e", '"refine" does not shorten',
                   "EXACT STAGE", "saturated at e = 1024", "0xFFFFFFFF", "out_nhops", "out_ndist", "plus n for the exact stage",
                   "leaves *out NULL", "ef < 1: HNSW_ERR_BAD_ARG", "ef > 1024: HNSW_ERR_UNSUPPORTED", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "HNSW_ERR_EMPTY_INDEX", "nq == 0: HNSW_OK", "2^31 - 1", "before any result buffer is allocated", "HNSW_ERR_OOM",
                   "DETERMINISM", "ONE range call in flight", "not counted in device_bytes", "no device-pointer form",
                   "hnsw_multi_replica"):
        assert needle in para, needle


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    out = ctypes.c_void_p(1)
    p = H._RangeParams(1.0, 16, 0)
    assert L.hnsw_range_search_batch(None, None, 0, 0, ctypes.byref(p), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_brute_force_batch(None, None, 0, 0, 1.0, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_range_search_batch(None, None, 0, 0, ctypes.byref(p), None) == H.ERR_BAD_ARG
    assert L.hnsw_range_brute_force_batch(None, None, 0, 0, 1.0, None) == H.ERR_BAD_ARG
    nq, total = ctypes.c_int64(7), ctypes.c_int64(7)
    assert L.hnsw_range_result_size(None, ctypes.byref(nq), ctypes.byref(total)) == H.ERR_BAD_ARG and nq.value == total.value == 7
    assert L.hnsw_range_result_fetch(None, None, None, None, None, None, None) == H.ERR_BAD_ARG
    ptr = ctypes.c_void_p(5)
    assert L.hnsw_range_result_device(None, ctypes.byref(ptr), None, None) == H.ERR_BAD_ARG and ptr.value == 5
    assert L.hnsw_range_result_destroy(None) == H.OK


def test_nan_radius_is_refused_before_a_device_is_needed(H):
    L = H.load()
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_brute_force_batch(None, None, 0, 0, float("nan"), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert "NaN" in L.hnsw_last_error().decode()
    out = ctypes.c_void_p(1)
    p = H._RangeParams(float("nan"), 16, 0)
    assert L.hnsw_range_search_batch(None, None, 0, 0, ctypes.byref(p), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert "NaN" in L.hnsw_last_error().decode()
