"""Option "half_rows" on every front end (no device needed): the header's row format and documentation, the Python, OCaml
and C++ constants, the set_option argument marshalling and the mapping of its errors."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def test_header_declares_the_row_format_and_the_option():
    hdr = _header()
    assert re.search(r"HNSW_ROWS_HALF = 4\b", hdr)
    assert re.search(r'"half_rows"', hdr)
    assert re.search(r"2 \* d for half rows", hdr)
    assert re.search(r"#define HNSW_ABI_VERSION 3\b", hdr)


def test_python_constants_match_the_header(H):
    hdr = _header()
    for name in ("F32", "BYTES", "SPLIT", "HALF"):
        m = re.search(r"HNSW_ROWS_%s = (\d+)" % name, hdr)
        assert m and getattr(H, "ROWS_" + name) == int(m.group(1)), name
    assert H.ROWS_HALF == 4


def test_ocaml_and_cpp_fronts_name_the_row_format():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    assert re.search(r"let rows_half = 4l", ml)
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert re.search(r"HALF = HNSW_ROWS_HALF", hpp)


def test_set_option_marshals_a_64_bit_value(H):
    L = H.load()
    assert L.hnsw_index_set_option.argtypes[1] is ctypes.c_char_p
    assert L.hnsw_index_set_option.argtypes[2] is ctypes.c_int64
    assert L.hnsw_index_set_option.restype is ctypes.c_int32


def test_set_option_errors_map_to_the_ocaml_exceptions(H):
    L = H.load()
    # a null handle is refused before any device is touched: Invalid_argument
    with pytest.raises(H.InvalidArgument, match="null argument"):
        H._check(L.hnsw_index_set_option(None, b"half_rows", -1))
    # what the option reports for data that does not fit fp16 (HNSW_ERR_UNSUPPORTED) is a Failure carrying its code
    with pytest.raises(H.Failure, match=r"^\[-7\]"):
        H._check(H.ERR_UNSUPPORTED)
