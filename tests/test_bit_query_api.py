"""CPU-side checks of option "bit_query_bits" (ocaml-hnsw_amd/csrc/hnsw_rows_bits.hip, hnsw_bits_asym_walk.hip): the entry point
that returns the 4-bit query codes exists in the library and in every front end, the header states the rule, and the knn kernel's
instances for the walk are built as units of their own, beside those of the Hamming walk."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOL = "hnsw_index_bit_query_codes"


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
    assert hdr.index('"bit_rows"      ') < hdr.index('"bit_query_bits" ')
    para = hdr[hdr.index('"bit_query_bits" '):]
    return " ".join(para[:para.index("int32_t hnsw_index_set_option(")].replace("\n *", " ").split())      # (one line: a rule may wrap)


def test_symbol_is_exported_and_mirrored(H):
    L = H.load()
    assert SYMBOL in H.ABI_SYMBOLS
    fn = getattr(L, SYMBOL)
    assert fn.argtypes is not None and len(fn.argtypes) == 5 and fn.restype is ctypes.c_int32
    decl = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\);" % SYMBOL, _header())
    assert decl and re.sub(r"/\*.*?\*/", "", decl.group(1)).count(",") + 1 == 5           # (the parameters' comments apart)
    assert callable(H.Hgraph.bit_query_codes)
    assert L.hnsw_abi_version() == 3 and H.ABI_VERSION == 3    # an additive entry point: the version stays
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    assert '"%s"' % SYMBOL in ml and "let bit_query_codes" in ml
    assert SYMBOL in hpp and "bit_query_codes(const Hgraph &g" in hpp


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    q = (ctypes.c_float * 4)()
    out = (ctypes.c_int8 * 4)()
    assert L.hnsw_index_bit_query_codes(None, q, 1, 4, out) == H.ERR_BAD_ARG
    assert L.hnsw_index_set_option(None, b"bit_query_bits", 4) == H.ERR_BAD_ARG


def test_header_documents_the_option():
    para = _paragraph()
    assert para.startswith('"bit_query_bits" supersedes the "asymmetric distance" item')
    for needle in ("7.0f / a", "round-half-even", "p0 + 2 * p1 + 4 * p2 - 8 * p3", "2 * A - SV", "y_i = fl(q_i - t_i)",
                   "IEEE-rounded division", "-7..7", "every code of that query is 0", "orders by node id", "64 * NW words",
                   "popcount(row_word & plane_p word)", "c0 + 2 * c1 + 4 * c2 - 8 * c3", "WHATEVER the index's metric",
                   "Not saved", "hnsw_sharded_set_option", "hnsw_multi_replica", "hnsw_index_bit_query_codes", "HNSW_ROWS_BITS",
                   "RATE AND RECALL"):
        assert needle in para, needle
    assert ("TWIN: ids, members of W, hops and evaluations of this walk are bit for bit those of a float32-row HNSW_METRIC_IP index "
            "with the same graph over S = where(X > t, 1, -1) (float32), searched with V (the codes as float32)") in para
    assert "every partial sum an integer of magnitude <= 7168" in para
    # the paragraph above is what it was: its list of what is not built still names the item this option supersedes
    assert "an asymmetric distance (float query against bits)" in _header()


def test_walk_instances_are_units_of_their_own(H):
    """the walk's kernels (ROWS = 7) are built once per accept rule from their own source; the older lists are what they were"""
    import __graft_entry__ as ge
    build = ge._load_build_module()
    assert build.BITS_ASYM_WALK_SOURCE == "hnsw_bits_asym_walk.hip" and build.BITS_ASYM_WALK_SOURCE in build.DEPS
    assert build.BITS_ASYM_WALKS == [0, 1]
    assert build.BITS_WALKS == [0, 1] and build.SQ8_DIM_WALKS == [0, 1]
    assert len(build.VARIANTS) == 20 and len(build.COLLECT_VARIANTS) == 16
    for s in build.BITS_ASYM_WALKS:
        assert os.path.exists(os.path.join(ROOT, "ocaml-hnsw_amd", "build", "hnsw_bits_asym_walk_%d.o" % s)), s
        assert os.path.exists(os.path.join(ROOT, "ocaml-hnsw_amd", "build", "hnsw_bits_walk_%d.o" % s)), s
    src = open(os.path.join(ROOT, "ocaml-hnsw_amd", "csrc", build.BITS_ASYM_WALK_SOURCE)).read()
    assert "hnsw_search_kernel<NCH, RB, NSLOT, 1, S_, 7>" in src and "rows_in_flight_bits" in src
    old = open(os.path.join(ROOT, "ocaml-hnsw_amd", "csrc", build.BITS_WALK_SOURCE)).read()
    assert "hnsw_search_kernel<NCH, RB, NSLOT, 0, S_, 6>" in old


def test_query_stride_against_the_kernels_words(tmp_path):
    """walk_query_words for every d in 1..1024, with and without the planes: the words the query transforms write and the walks read
    lie inside a row of that stride, each written once -- and the planes of a narrow row (d = 20: 64 words) do not fit its padded
    float stride (32): tests/cpp/test_bits_plan.cpp, a host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_bits_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_bits_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"bits plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) == 2048, out.stdout + out.stderr
    import __graft_entry__ as ge
    assert "hnsw_bits_plan.h" in ge._load_build_module().DEPS
