"""CPU-side checks of soft deletion and of range search under an allow-mask (ocaml-hnsw_amd/csrc/hnsw_soft_delete.hip,
hnsw_range.hip): the seven entry points exist in the library and in every front end with the header's arity, the header states
their definitions, what can be refused without a device is, and the plain-number half of the marks (hnsw_mark_plan.h: the live
mask under a renumbering) agrees with a naive restatement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_range_search_batch_filtered", "hnsw_range_brute_force_batch_filtered", "hnsw_index_mark_deleted",
           "hnsw_index_unmark_deleted", "hnsw_index_deleted_count", "hnsw_index_deleted_bits", "hnsw_index_compact")
ARITY = (7, 7, 3, 3, 2, 2, 2)


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
    assert L.hnsw_range_brute_force_batch_filtered.argtypes[5] is ctypes.c_float    # the radius travels by value
    for method in ("mark_deleted", "unmark_deleted", "deleted_count", "deleted_mask", "compact"):
        assert callable(getattr(H.Hgraph, method)), method
    import inspect
    for fn in (H.Ohnsw.range_search, H.Ohnsw.brute_force_range, H.Ba.range_search):
        assert "filter" in inspect.signature(fn).parameters
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name + "(" in hpp, name
    for wrapper in ("let mark_deleted ", "let unmark_deleted ", "let deleted_count ", "let deleted_mask ", "let compact ",
                    "let range_search ?(semantics = 0) ?(filter", "let brute_force_range ?(filter"):
        assert wrapper in ml, wrapper
    for wrapper in ("inline void mark_deleted(", "inline void unmark_deleted(", "inline int64_t deleted_count(", "inline std::vector<int32_t> compact(",
                    "range_search(const Hgraph &g, const Filter &f,", "brute_force_range(const Hgraph &g, const Filter &f,"):
        assert wrapper in hpp, wrapper
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_soft_delete.cpp"))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"test_front_soft_delete"' in entry                  # build() compiles the driver
    build = open(os.path.join(ROOT, "ocaml-hnsw_amd", "build.py")).read()
    for f in ("hnsw_soft_delete.hip", "hnsw_mark_plan.h"):
        assert '"%s"' % f in build, f
        assert os.path.exists(os.path.join(ROOT, "ocaml-hnsw_amd", "csrc", f))


def test_header_states_the_definitions():
    hdr = _header()
    para = hdr[hdr.index("THE RESULT of the filtered range calls"):]
    para = " ".join(para[:para.index("*/")].replace("\n *", " ").split())
    for needle in ("SEGMENT", "left out and the", "order kept", "STAGE AND HOPS", "whatever the mask says", "out_stage and out_nhops equal",
                   "re-ranked first", "mask is applied after", "EVALUATIONS", "n_allowed instead of n", "NO WALK", "allows no node",
                   "0xFFFFFFFF", "both counters are 0", "ERRORS", "null, foreign or stale filter", "HNSW_ERR_BAD_ARG", "leaves *out NULL",
                   "SINGLE FILTER ONLY", "per-query filters and per-query radii are not built", "not as a host post-filter",
                   "never counted, stored, sorted or held against", "2^31 - 1", "without a set bit", '"no mask" of the same driver'):
        assert needle in para, needle
    para = hdr[hdr.index("soft deletion owned by the index: mark, search around, compact"):]
    para = " ".join(para[:para.index("*/")].replace("\n *", " ").split())         # (one line: a rule may wrap)
    for needle in ("THE MARKS", "LIVE", "first mark", "NOT counted in hnsw_index_info.device_bytes", "id_base-based", "does nothing",
                   "m == 0 is a no-op", "an id out of range", "a duplicate within the call", "null ids with m > 0", "m < 0",
                   "not yet waited for", "replica of an hnsw_multi", "hnsw_index_deleted_bits", "ceil(n / 32) words",
                   "EPOCH", "changes at least one bit", "GRAPH", "stay in the graph", "no region is cut off",
                   "only while n_deleted > 0", "bit for bit", "hnsw_search_batch_filtered under LIVE", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "*out_count = the real entries", "k smallest LIVE nodes", "_filtered forms under LIVE", "ANDed with the live mask",
                   "label counts as -1", "new nodes are live", "out_new_id's numbering", "before the swap", "HNSW_ERR_UNSUPPORTED",
                   "compact or unmark first", "marked nodes are not saved", "NOT AFFECTED", "hnsw_distance_batch", "hnsw_rerank_batch",
                   "hnsw_select_neighbours_batch", "n stays the stored", "EVERY NODE MARKED", "not HNSW_ERR_EMPTY_INDEX", "COUNT BACK AT 0",
                   "never marked", "accepted again", "hnsw_index_remove(idx, the marked ids ascending, n_deleted, out_new_id)",
                   "Afterwards nothing is marked", "identity", "NOT BUILT", "saved marks", "filters that survive a mark"):
        assert needle in para, needle


def test_null_handles_are_refused_on_the_host_with_the_outputs_untouched(H):
    L = H.load()
    p = H._RangeParams(1.0, 16, 0)
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_search_batch_filtered(None, None, None, 0, 0, ctypes.byref(p), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_brute_force_batch_filtered(None, None, None, 0, 0, 1.0, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_range_search_batch_filtered(None, None, None, 0, 0, ctypes.byref(p), None) == H.ERR_BAD_ARG
    assert L.hnsw_range_brute_force_batch_filtered(None, None, None, 0, 0, 1.0, None) == H.ERR_BAD_ARG
    out = ctypes.c_void_p(1)
    assert L.hnsw_range_brute_force_batch_filtered(None, None, None, 0, 0, float("nan"), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert "NaN" in L.hnsw_last_error().decode()
    ids = np.array([0, 1], np.int64)
    assert L.hnsw_index_mark_deleted(None, ids.ctypes.data_as(ctypes.c_void_p), 2) == H.ERR_BAD_ARG
    assert L.hnsw_index_unmark_deleted(None, ids.ctypes.data_as(ctypes.c_void_p), 2) == H.ERR_BAD_ARG
    assert L.hnsw_index_mark_deleted(None, None, 0) == H.ERR_BAD_ARG
    c = ctypes.c_int64(77)
    assert L.hnsw_index_deleted_count(None, ctypes.byref(c)) == H.ERR_BAD_ARG and c.value == 77
    words = np.full(4, 77, np.uint32)
    assert L.hnsw_index_deleted_bits(None, words.ctypes.data_as(ctypes.c_void_p)) == H.ERR_BAD_ARG and (words == 77).all()
    new_id = np.full(4, 77, np.int32)
    assert L.hnsw_index_compact(None, new_id.ctypes.data_as(ctypes.c_void_p)) == H.ERR_BAD_ARG and (new_id == 77).all()


def test_mark_plan_against_a_naive_restatement(tmp_path):
    """renumber_live_mask and marked_ids over a grid of n, marked sets, removals and inserts: tests/cpp/test_mark_plan.cpp, a host
    program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_mark_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_mark_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"mark plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
