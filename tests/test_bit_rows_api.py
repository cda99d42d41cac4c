"""CPU-side checks of option "bit_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_bits.hip, hnsw_bits_walk.hip): the two introspection entry
points exist in the library and in every front end, the row format has its number, the header states the contract, and the knn
kernel's instances for the format are built as units of their own, outside the variant table."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_bit_params", "hnsw_index_bit_codes")


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def _paragraph():
    hdr = _header()
    para = hdr[hdr.index('"bit_rows"      '):]
    return " ".join(para[:para.index("int32_t hnsw_index_set_option(")].replace("\n *", " ").split())      # (one line: a rule may wrap)


def test_symbols_are_exported_and_mirrored(H):
    L = H.load()
    for name, arity in zip(SYMBOLS, (2, 2)):
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32
        decl = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\);" % name, _header())
        assert decl and re.sub(r"/\*.*?\*/", "", decl.group(1)).count(",") + 1 == arity     # (the parameters' comments apart)
    assert callable(H.Hgraph.bit_params) and callable(H.Hgraph.bit_codes)
    assert L.hnsw_abi_version() == 3                       # additive entry points: the version stays


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    t = (ctypes.c_float * 4)()
    assert L.hnsw_index_bit_params(None, t) == H.ERR_BAD_ARG
    assert L.hnsw_index_bit_codes(None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_set_option(None, b"bit_rows", 1) == H.ERR_BAD_ARG


def test_row_format_number(H):
    assert H.ROWS_BITS == 7
    assert re.search(r"\bHNSW_ROWS_BITS\s*=\s*7\b", _header())
    assert (H.ROWS_F32, H.ROWS_BYTES, H.ROWS_SPLIT, H.ROWS_HALF, H.ROWS_SQ8, H.ROWS_SQ8_DIM) == (0, 2, 3, 4, 5, 6)


def test_header_documents_the_option():
    hdr = _header()
    options = hdr[hdr.index("and one that CHANGES results"):hdr.index("int32_t hnsw_index_set_option(")]
    assert options.index('"sq8_dim_rows"  ') < options.index('"filter_collect" 0 = off') < options.index('"refine"        ') < options.index('"bit_rows"      ')
    para = _paragraph()
    for needle in ("x_i > t_i", "equality gives 0", "-0 counts as +0", "1 = on, the thresholds t at the column means",
                   "2 = on, the thresholds at zero", "bit i % 32 of word i / 32", "NW = ceil(d / 512)", "16 * NW words", "float64",
                   "fixed by (n, d) alone", "names the first such column", "HNSW_ERR_UNSUPPORTED", "popcount(row_word ^ query_word)",
                   "(float)(4 * H)", "WHATEVER the index's metric", "min(ef, max(k, R))", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "ONLY THE FIRST k BY HAMMING DISTANCE", '"refine" -1 (all ef) is the setting this format is meant for',
                   "hnsw_index_insert and hnsw_index_remove", "device_bytes", "n * 64 * NW bytes", "4 * 512 * NW bytes", "(d + 7) / 8",
                   "hnsw_index_bit_params", "HNSW_ROWS_BITS", "hnsw_sharded_set_option", "a page-locked host matrix is read in place"):
        assert needle in para, needle
    # the twin sentence
    assert ("bit for bit those of a float32-row L2 index with the same graph over S = where(X > t, 1, -1) (float32), "
            "searched with where(Q > t, 1, -1)") in para
    assert "every term of that float sum is 0 or 4 and every partial sum an integer <= 4096" in para
    # the exclusions, both ways
    assert "EXCLUSIONS" in para and "while byte rows are in use" in para
    assert "while option half_rows, sq8_rows, sq8_dim_rows or filter_collect is on" in para
    assert "of those four is set to 1 while this option is on" in para
    # what is not saved, what is not built
    assert "Not saved: a loaded index starts without the copy" in para
    assert ("Not built: hand-scheduled hop loops for this format, an asymmetric distance (float query against bits), more than one "
            "bit per dimension, a saved copy, \"filter_collect\" with bit rows, a changed default for \"refine\"") in para
    # the entries whose exclusion sentences other tests pin are what they were
    assert "while option half_rows, sq8_rows or filter_collect is on" in hdr


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert '"%s"' % name in ml and name in hpp
    assert "rows_bits = 7l" in ml and "BITS = HNSW_ROWS_BITS" in hpp
    assert "let bit_params" in ml and "let bit_codes" in ml and "inline Bits bits(const Hgraph &g)" in hpp


def test_walk_instances_are_units_of_their_own(H):
    """the Hamming walk's kernels (ROWS = 6) are built once per accept rule from their own source, beside the 20 + 16 variant objects"""
    import __graft_entry__ as ge
    build = ge._load_build_module()
    assert build.BITS_WALK_SOURCE == "hnsw_bits_walk.hip" and build.BITS_WALK_SOURCE in build.DEPS
    assert "hnsw_rows_bits.hip" in build.SOURCES and build.BITS_WALKS == [0, 1]
    assert len(build.VARIANTS) == 20 and len(build.COLLECT_VARIANTS) == 16
    for s in build.BITS_WALKS:
        assert os.path.exists(os.path.join(ROOT, "ocaml-hnsw_amd", "build", "hnsw_bits_walk_%d.o" % s)), s
    src = open(os.path.join(ROOT, "ocaml-hnsw_amd", "csrc", build.BITS_WALK_SOURCE)).read()
    assert "hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 6>" in src and "rows_in_flight_bits" in src
