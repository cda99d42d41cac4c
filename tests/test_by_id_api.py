"""CPU-side checks of the searches by stored item (ocaml-hnsw_amd/csrc/hnsw_by_id.hip): the five entry points exist in the library and
in every front end, the ABI version stays, the header's last section states the definition, null handles and null arrays are refused
on the host, and the arithmetic that is plain numbers (hnsw_by_id_plan.h: the drop-self rule on one row, (ef', k') and their limits,
the chunk bounds of hnsw_knn_graph) holds against a naive restatement."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_get_rows_device", "hnsw_search_batch_by_id", "hnsw_search_batch_by_key", "hnsw_brute_force_batch_by_id", "hnsw_knn_graph")
ARITY = (6, 9, 10, 8, 5)


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
    # counts, strides and missing_key cross the ABI as 64-bit values, not as ctypes' default C int
    assert L.hnsw_search_batch_by_key.argtypes[5] is ctypes.c_int64 and L.hnsw_search_batch_by_key.argtypes[2] is ctypes.c_int64
    assert L.hnsw_index_get_rows_device.argtypes[2] is ctypes.c_int64 and L.hnsw_index_get_rows_device.argtypes[4] is ctypes.c_int64
    assert L.hnsw_search_batch_by_id.argtypes[2] is ctypes.c_int64 and L.hnsw_search_batch_by_id.argtypes[4] is ctypes.c_int32
    for fn in (H.Ohnsw.knn_batch_by_id, H.Ohnsw.knn_batch_by_key, H.Ohnsw.brute_force_by_id, H.Ba.knn_batch_by_id, H.Ba.knn_batch_by_key,
               H.Hgraph.knn_graph, H.rows_device):
        assert callable(fn)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let knn_batch_by_id ", "let knn_batch_by_key ", "let brute_force_by_id ", "let knn_graph "):
        assert wrapper in ml, wrapper
    for fn in ("knn_by_id(", "knn_by_key(", "brute_force_by_id(", "knn_graph(", "rows_device("):
        assert fn in hpp, fn
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_by_id.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    start = hdr.index("---- search by stored item")
    # the new section is the header's last: nothing of the existing text moved
    assert start > hdr.index("int32_t hnsw_filter_create_by_keys(")
    assert hdr.count("/* ----", start - 3) == 1 and "#ifdef __cplusplus\n}\n#endif\n#endif /* HNSW_MI355X_H */" in hdr[start:]
    para = hdr[start:]
    para = re.sub(r"\s*\n \*\s*", " ", para[:para.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    for needle in ("position p deleted", "ef' = max(ef, k + 1)", "first by position", "row of d zeros", "graph_chunk_rows",
                   "bit for bit", "k' = k + 1", "the smallest j in [0, k]", "the first k of them", "Trailing fill entries stay fill",
                   "N(N(x))", "a legal QUERY", "not on the batch it is in", "It uses no scratch of the handle",
                   "HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG", "k + 1 > 1024 is HNSW_ERR_UNSUPPORTED", "nq == 0 is a no-op",
                   "by_id(find_keys(keys))", "A handle without keys is HNSW_ERR_BAD_ARG", "lower-numbered duplicates",
                   "default 65536, values < 1 refused", "n == 0 is HNSW_OK", "accepted read-only",
                   "NOT BUILT", "a device-pointer form of the search by id", "hnsw_sharded_* forms", "range search by id",
                   "starting the layer-0 walk at the node itself", "overlap of one chunk's download"):
        assert needle in para, needle
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("hnsw_search_batch_by_id", "gather_rows16_kernel", "drop_self_kernel", "Not built:", "hnsw_knn_graph"):
        assert needle in design, needle
    assert "hnsw_search_batch_by_id" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hnsw_search_batch_by_id" in open(os.path.join(ROOT, "README.md")).read()


def test_null_handles_and_null_arrays_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 10, 0, 0)
    i32, i64, f32 = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_float(7.0)
    assert L.hnsw_index_get_rows_device(None, None, 0, None, 0, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_get_rows_device(None, ctypes.byref(i32), 1, ctypes.byref(f32), 4, None) == H.ERR_BAD_ARG and f32.value == 7.0
    assert L.hnsw_search_batch_by_id(None, ctypes.byref(i32), 1, ctypes.byref(p), 1, ctypes.byref(i32), ctypes.byref(f32), None, None) == H.ERR_BAD_ARG
    assert L.hnsw_search_batch_by_id(None, None, 0, ctypes.byref(p), 0, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_search_batch_by_id(None, None, 0, None, 0, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_search_batch_by_key(None, ctypes.byref(i64), 1, ctypes.byref(p), 1, -1, ctypes.byref(i64), ctypes.byref(f32), None, None) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch_by_id(None, ctypes.byref(i32), 1, 10, 0, 1, ctypes.byref(i32), ctypes.byref(f32)) == H.ERR_BAD_ARG
    assert L.hnsw_knn_graph(None, ctypes.byref(p), 0, ctypes.byref(i32), ctypes.byref(f32)) == H.ERR_BAD_ARG
    assert L.hnsw_knn_graph(None, None, 0, None, None) == H.ERR_BAD_ARG
    assert i32.value == 7 and i64.value == 7 and f32.value == 7.0
    assert b"null" in L.hnsw_last_error()


def test_python_refuses_ids_that_are_no_int32(H):
    with pytest.raises(H.InvalidArgument):
        H._ids32([1.5, 2.0])
    with pytest.raises(H.InvalidArgument):
        H._ids32([2 ** 31])
    a = H._ids32([[0, 5], [2 ** 31 - 1, -1]])
    assert a.dtype.name == "int32" and a.tolist() == [0, 5, 2 ** 31 - 1, -1]


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_by_id.hip" in b.SOURCES and "hnsw_by_id.hip" in b.DEPS and "hnsw_by_id_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16


def test_by_id_plan_against_a_naive_restatement(tmp_path):
    """drop-self on rows with self at 0, in the middle, at k, absent, twice and among fill entries, k = 1 and k = 1023; the limits; the
    chunk bounds for n = 0, 1, chunk - 1, chunk, chunk + 1: tests/cpp/test_by_id_plan.cpp, a host program, under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "test_by_id_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_by_id_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"by-id plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
