"""CPU-side checks of grouped search (ocaml-hnsw_amd/csrc/hnsw_group.hip): the six entry points exist in the library and in every
front end, the header states the definition, null handles are refused on the host, and the exact stage's cut of its queries
(hnsw_group_plan.h) keeps what the driver relies on."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_labels_create", "hnsw_labels_destroy", "hnsw_labels_info", "hnsw_labels_get", "hnsw_search_batch_grouped",
           "hnsw_brute_force_batch_grouped")
ARITY = (5, 1, 4, 2, 13, 11)


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
    assert "typedef struct hnsw_labels hnsw_labels;" in hdr
    assert callable(H.Ohnsw.knn_batch_grouped) and callable(H.Ohnsw.brute_force_grouped) and callable(H.Ba.knn_batch_grouped)
    assert callable(H.Hgraph.labels) and callable(H.Labels.info) and callable(H.Labels.get)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let labels_create ", "let labels_info ", "let labels_get ", "let knn_batch_grouped ", "let brute_force_grouped "):
        assert wrapper in ml, wrapper
    assert "class Labels" in hpp and "knn_grouped(" in hpp and "brute_force_grouped(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_grouped.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    para = hdr[hdr.index("---- grouped search"):]
    para = re.sub(r"\s*\n \*\s*", " ", para[:para.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    # the new section is the header's last: nothing of the existing text moved
    assert hdr.index("---- grouped search") > hdr.index("int32_t hnsw_merge_segments(")
    for needle in ("THE LABELS", "-1 .. n_labels - 1", "in no group", "before anything is allocated", "*out is NULL",
                   "gets -1 in the device copy", "hnsw_labels_get", "it is stale", "n_labelled", "n_groups",
                   "4 * n bytes on the device, NOT counted in", "Not saved",
                   "THE RESULT of hnsw_search_batch_grouped", "ELIGIBLE", "first eligible member of each label",
                   "1. LADDER", "e_{j+1} = min(1024, 2 * e_j)", "|G(W_{e_j}(q))| >= k", "never filtered or grouped",
                   "2. EXACT STAGE", "n_groups < k or f->n_allowed < k", "pre-square-root key, then the node id", "label -1",
                   "3. DISTANCES ARE ALWAYS OVER THE FLOAT32 ROWS", "HNSW_ROWS_SQ8_DIM", "k := e", "does not depend on the order",
                   "4. OUTPUTS", "out_labels [nq][k]", "0xFFFFFFFF", "plus n_labelled for the exact stage",
                   "5. ERRORS", "HNSW_ERR_UNSUPPORTED", "HNSW_SEM_FUNCTOR_NEAREST_K", "HNSW_ERR_EMPTY_INDEX", "outputs untouched",
                   "6. DETERMINISM", "ONE filtered, range or grouped call in flight per handle", "no device-pointer form",
                   "8 * n_labels bytes per query", "HNSW_ERR_OOM", "does not depend on option \"scan_slabs\"",
                   "NOT BUILT", "group_size > 1", "one label object per query", "hnsw_sharded_* grouped forms",
                   "option \"filter_collect\" for this call"):
        assert needle in para, needle
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "hnsw_search_batch_grouped" in design and "group_size > 1" in design


def test_null_handles_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 10, 0, 0)
    out = ctypes.c_void_p(7)
    assert L.hnsw_labels_create(None, None, 0, 3, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    out = ctypes.c_void_p(7)
    assert L.hnsw_labels_create(None, None, 0, 0, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None     # n_labels < 1
    assert L.hnsw_labels_create(None, None, 0, 3, None) == H.ERR_BAD_ARG
    assert L.hnsw_labels_destroy(None) == H.OK
    a = ctypes.c_int32(5)
    assert L.hnsw_labels_info(None, ctypes.byref(a), None, None) == H.ERR_BAD_ARG and a.value == 5
    assert L.hnsw_labels_get(None, ctypes.byref(a)) == H.ERR_BAD_ARG and a.value == 5
    assert L.hnsw_search_batch_grouped(None, None, None, None, 0, 0, ctypes.byref(p), None, None, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch_grouped(None, None, None, None, 0, 0, 10, 0, None, None, None) == H.ERR_BAD_ARG


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_group.hip" in b.SOURCES and "hnsw_group.hip" in b.DEPS and "hnsw_group_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16


def test_group_plan_against_a_naive_restatement(tmp_path):
    """group_plan over a grid of (n_labels, m, T): the piece is a multiple of T, at least T, within the scratch bound whenever T
    queries fit, and every query lies in exactly one piece: tests/cpp/test_group_plan.cpp, a host program, under AddressSanitizer
    and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_group_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_group_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"group plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
