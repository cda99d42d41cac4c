"""CPU-side checks of the keys an index owns (ocaml-hnsw_amd/csrc/hnsw_keys.hip): the twelve entry points exist in the library and
in every front end, the header states the definitions, null handles and null arrays are refused on the host, and the arithmetic
that is plain numbers (hnsw_keys_plan.h: the lookup on a sorted array, the renumbering rule) holds against a naive restatement."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_set_keys", "hnsw_index_clear_keys", "hnsw_index_keys_info", "hnsw_index_keys_of", "hnsw_index_keys_of_device",
           "hnsw_index_find_keys", "hnsw_search_batch_keyed", "hnsw_index_insert_keyed", "hnsw_index_remove_keys",
           "hnsw_index_mark_deleted_keys", "hnsw_index_unmark_deleted_keys", "hnsw_filter_create_by_keys")
ARITY = (3, 1, 3, 5, 6, 4, 12, 6, 4, 3, 3, 4)


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
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == arity, name                       # the header's own argument list
    # keys and missing_key cross the ABI as 64-bit values, not as ctypes' default C int
    assert L.hnsw_search_batch_keyed.argtypes[6] is ctypes.c_int64 and L.hnsw_index_keys_of.argtypes[3] is ctypes.c_int64
    for name in ("set_keys", "clear_keys", "keys", "find_keys", "keys_info", "remove_keys", "mark_deleted_keys", "unmark_deleted_keys",
                 "filter_by_keys"):
        assert callable(getattr(H.Hgraph, name)), name
    assert callable(H.Ohnsw.knn_batch_keyed) and callable(H.Ba.knn_batch_keyed) and callable(H.Ohnsw.insert_batch_keyed)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let set_keys ", "let keys_of ", "let find_keys ", "let knn_batch_keyed ", "let insert_batch_keyed ", "let remove_keys ",
                    "let mark_deleted_keys "):
        assert wrapper in ml, wrapper
    for fn in ("set_keys(", "clear_keys(", "keys_info(", "keys_of(", "find_keys(", "knn_keyed(", "insert_keyed(", "remove_keys(",
               "mark_deleted_keys(", "unmark_deleted_keys(", "by_keys("):
        assert fn in hpp, fn
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_keys.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    start = hdr.index("---- keys: stable 64-bit names")
    # the new section is the header's last: nothing of the existing text moved
    assert start > hdr.index("int32_t hnsw_brute_force_batch_grouped(")
    para = hdr[start:]
    para = re.sub(r"\s*\n \*\s*", " ", para[:para.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    for needle in ("every value legal", "pairwise distinct", "SIGNED", "bit for bit as before", "NOT counted in hnsw_index_info.device_bytes",
                   "n must be the index's n", "smallest duplicated key", "All or nothing", "HNSW_ERR_OOM included",
                   "does not move the graph epoch", "a shard of an hnsw_sharded is refused",
                   "one that never had keys",
                   "missing_key", "fill id -1", "still has its key", "m must be n", "range results, grouped rows",
                   "id_base - 1 if there is none", "Repeated keys in the call are fine", "m == 0 is a no-op",
                   "those of hnsw_search_batch (marks honoured as there)", "hnsw_search_batch_filtered(f)", "bit-identical",
                   "zero for the plain path of an unmarked handle", "one translate launch", "not a second pass over host memory",
                   "link for link", "Refused before anything is built", "two equal keys in the call", "An EMPTY index without keys",
                   "pointing at the keyed call", "must never hold a node without one",
                   "new_key_of[new_id[v]] = key_of[v]", "inside the all-or-nothing swap", "Removing every node",
                   "hnsw_index_remove(find(keys))", "hnsw_index_mark_deleted(find(keys))", "hnsw_index_unmark_deleted(find(keys))",
                   "nothing is changed", "allows exactly the named nodes", "ANDed with the live mask", "naming the first by position",
                   "keys are NOT saved", "hnsw_index_set_keys on the loaded handle is the round trip",
                   "NOT BUILT", "keys for hnsw_sharded and hnsw_multi", "upsert", "saved keys",
                   "keyed forms of the range, grouped and per-query-filter calls", "compose those with hnsw_index_keys_of"):
        assert needle in para, needle
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("hnsw_search_batch_keyed", "keys_translate_kernel", "keys_dup_kernel", "keys_find_kernel", "keys_renumber_kernel",
                   "keys_allow_kernel", "upsert"):
        assert needle in design, needle
    assert "hnsw_index_set_keys" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hnsw_search_batch_keyed" in open(os.path.join(ROOT, "README.md")).read()


def test_null_handles_and_null_arrays_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 10, 0, 0)
    b = H._BuildParams(8, 40, 0, 0, 1, 0, 0, 0, 0)
    key = ctypes.c_int64(5)
    a32, a64 = ctypes.c_int32(7), ctypes.c_int64(7)
    assert L.hnsw_index_set_keys(None, ctypes.byref(key), 1) == H.ERR_BAD_ARG
    assert L.hnsw_index_set_keys(None, None, 0) == H.ERR_BAD_ARG
    assert L.hnsw_index_clear_keys(None) == H.ERR_BAD_ARG
    assert L.hnsw_index_keys_info(None, ctypes.byref(a32), ctypes.byref(a64)) == H.ERR_BAD_ARG and a32.value == 7 and a64.value == 7
    assert L.hnsw_index_keys_of(None, None, 0, -1, ctypes.byref(key)) == H.ERR_BAD_ARG and key.value == 5
    assert L.hnsw_index_keys_of_device(None, None, 0, -1, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_find_keys(None, ctypes.byref(key), 1, ctypes.byref(a64)) == H.ERR_BAD_ARG and a64.value == 7
    assert L.hnsw_search_batch_keyed(None, None, None, 0, 0, ctypes.byref(p), -1, None, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_insert_keyed(None, None, 0, 0, None, ctypes.byref(b)) == H.ERR_BAD_ARG
    assert L.hnsw_index_remove_keys(None, ctypes.byref(key), 1, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_mark_deleted_keys(None, ctypes.byref(key), 1) == H.ERR_BAD_ARG
    assert L.hnsw_index_unmark_deleted_keys(None, ctypes.byref(key), 1) == H.ERR_BAD_ARG
    out = ctypes.c_void_p(7)
    assert L.hnsw_filter_create_by_keys(None, ctypes.byref(key), 1, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_filter_create_by_keys(None, ctypes.byref(key), 1, None) == H.ERR_BAD_ARG
    assert b"null" in L.hnsw_last_error()


def test_python_refuses_keys_that_are_no_int64(H):
    with pytest.raises(H.InvalidArgument):
        H._keys([1.5, 2.0])
    with pytest.raises(H.InvalidArgument):
        H._keys([2 ** 63])
    k = H._keys([-2 ** 63, 2 ** 63 - 1, -1, 0])
    assert k.dtype.name == "int64" and k.tolist() == [-2 ** 63, 2 ** 63 - 1, -1, 0]


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_keys.hip" in b.SOURCES and "hnsw_keys.hip" in b.DEPS and "hnsw_keys_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16


def test_keys_plan_against_a_naive_restatement(tmp_path):
    """keys_position on sorted arrays of length 0, 1, 2 and 1000 that hold INT64_MIN and INT64_MAX, asked for keys below, between
    and above; the renumbering rule against a brute-force restatement; the smallest duplicate: tests/cpp/test_keys_plan.cpp, a
    host program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_keys_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_keys_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"keys plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
