"""CPU-side checks of option "sq8_dim_rows" (ocaml-hnsw_amd/csrc/hnsw_rows_sq8_dim.hip, hnsw_sq8_dim_walk.hip): the two
introspection entry points exist in the library and in every front end, the row format has its number, the header states the
contract, and the knn kernel's instances for the format are built as units of their own."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_sq8_dim_params", "hnsw_index_sq8_dim_codes")


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
    para = hdr[hdr.index('"sq8_dim_rows"  '):]
    return " ".join(para[:para.index('"filter_collect" 0 = off')].replace("\n *", " ").split())      # (one line: a rule may wrap)


def test_symbols_are_exported_and_mirrored(H):
    L = H.load()
    for name, arity in zip(SYMBOLS, (3, 2)):
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32
        decl = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\);" % name, _header())
        assert decl and decl.group(1).count(",") + 1 == arity
    assert callable(H.Hgraph.sq8_dim_params) and callable(H.Hgraph.sq8_dim_codes)
    assert L.hnsw_abi_version() == 3                       # additive entry points: the version stays


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    lo, s = (ctypes.c_float * 4)(), (ctypes.c_float * 4)()
    assert L.hnsw_index_sq8_dim_params(None, lo, s) == H.ERR_BAD_ARG
    assert L.hnsw_index_sq8_dim_codes(None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_set_option(None, b"sq8_dim_rows", 1) == H.ERR_BAD_ARG


def test_row_format_number(H):
    assert H.ROWS_SQ8_DIM == 6
    assert re.search(r"\bHNSW_ROWS_SQ8_DIM\s*=\s*6\b", _header())
    assert (H.ROWS_F32, H.ROWS_BYTES, H.ROWS_SPLIT, H.ROWS_HALF, H.ROWS_SQ8) == (0, 2, 3, 4, 5)


def test_header_documents_the_option():
    hdr = _header()
    options = hdr[hdr.index("and one that CHANGES results"):hdr.index("int32_t hnsw_index_set_option(")]
    assert options.index('"sq8_rows"      ') < options.index('"sq8_dim_rows"  ') < options.index('"filter_collect" 0 = off')
    para = _paragraph()
    for needle in ("rint((x - lo_i) / s_i)", "ties to even", "s_i = 1 when hi_i == lo_i", "a bound of -0 counts as +0", "q''", "s_i * q_i",
                   "fl((float)code * s_i)", "names the first such column", "min(ef, max(k, R))", "HNSW_ERR_UNSUPPORTED",
                   "HNSW_SEM_FUNCTOR_NEAREST_K", "hnsw_index_insert and hnsw_index_remove", "device_bytes", "Not saved",
                   "hnsw_index_sq8_dim_params", "64 * NCH", "HNSW_ROWS_SQ8_DIM", "hnsw_sharded_set_option", "visited_blocks"):
        assert needle in para, needle
    # the twin sentence
    assert ("bit for bit those of a float32-row L2 index with the same graph over Z = C.astype(float32) * s (numpy float32), "
            "searched with Q'' = Q - lo") in para
    assert "bit for bit the inner-product search over C.astype(float32) with q'" in para
    # the exclusions, both ways
    assert "EXCLUSIONS" in para and "while byte rows are in use" in para
    assert "while option half_rows, sq8_rows or filter_collect is on" in para and "set to 1 while this option is on" in para
    # what is not built
    assert "Not built: hand-scheduled loops for this format, a saved copy" in para
    # sq8_rows points here instead of calling it unbuilt
    sq8 = hdr[hdr.index('"sq8_rows"      '):hdr.index('"sq8_dim_rows"  ')]
    assert '"sq8_dim_rows"' in sq8 and "not built" not in sq8


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert '"%s"' % name in ml and name in hpp
    assert "rows_sq8_dim = 6l" in ml and "HNSW_ROWS_SQ8_DIM" in hpp


def test_walk_instances_are_units_of_their_own(H):
    """the L2 walk's kernels (ROWS = 5) are built once per accept rule from their own source, beside the 20 variant objects"""
    import __graft_entry__ as ge
    build = ge._load_build_module()
    assert build.SQ8_DIM_WALK_SOURCE == "hnsw_sq8_dim_walk.hip" and build.SQ8_DIM_WALK_SOURCE in build.DEPS
    assert "hnsw_rows_sq8_dim.hip" in build.SOURCES and build.SQ8_DIM_WALKS == [0, 1]
    for s in build.SQ8_DIM_WALKS:
        assert os.path.exists(os.path.join(ROOT, "ocaml-hnsw_amd", "build", "hnsw_sq8_dim_walk_%d.o" % s)), s
    src = open(os.path.join(ROOT, "ocaml-hnsw_amd", "csrc", build.SQ8_DIM_WALK_SOURCE)).read()
    assert "hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 5>" in src and "rows_in_flight_sq8_dim" in src
