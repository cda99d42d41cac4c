"""CPU-side checks of the paged searches (ocaml-hnsw_amd/csrc/hnsw_after.hip): the two entry points exist in the library and in every
front end, the ABI version stays, the header's last section states the definition, null handles, null arrays, nq < 0 and a NaN cursor
are refused on the host with outputs untouched, and the arithmetic that is plain numbers (hnsw_after_plan.h: ord, the cursor's word,
"after", the next cursor, the L2 key bound) holds against its definitions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_search_batch_after", "hnsw_brute_force_batch_after")
ARITY = (13, 11)


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
        decl = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("int32_t %s(" % name):], flags=re.S)      # (a comment may hold a ';')
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == arity, name                       # the header's own argument list
    # counts and strides cross the ABI as 64-bit values, not as ctypes' default C int
    for name in SYMBOLS:
        assert getattr(L, name).argtypes[4] is ctypes.c_int64 and getattr(L, name).argtypes[5] is ctypes.c_int64
    assert L.hnsw_brute_force_batch_after.argtypes[6] is ctypes.c_int32 and L.hnsw_brute_force_batch_after.argtypes[7] is ctypes.c_int32
    for fn in (H.Ohnsw.knn_batch_after, H.Ohnsw.brute_force_after, H.Ohnsw.knn_pages, H.Ba.knn_batch_after):
        assert callable(fn)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)
    # the cursor: 8 bytes, (float distance, int32 id); the start cursor is before every node
    assert H.CURSOR_DTYPE.itemsize == 8 and H.CURSOR_DTYPE.names == ("dist", "id")
    assert H.CURSOR_DTYPE.fields["dist"][1] == 0 and H.CURSOR_DTYPE.fields["id"][1] == 4
    assert H.CURSOR_START["dist"] == -np.inf and H.CURSOR_START["id"] == -2 ** 31
    assert re.search(r"typedef struct hnsw_cursor \{ float dist; int32_t id; \} hnsw_cursor;", hdr)
    assert re.search(r"#define HNSW_CURSOR_START \{ -INFINITY, INT32_MIN \}", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let knn_batch_after ", "let brute_force_after ", "let cursor_start "):
        assert wrapper in ml, wrapper
    for fn in ("struct Cursor", "knn_after(", "brute_force_after("):
        assert fn in hpp, fn
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_after.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    start = hdr.index("#### paged k-NN search")
    # the new section is the header's last: nothing of the existing text moved
    assert start > hdr.index("int32_t hnsw_index_update(")
    tail = hdr[start:]
    assert "/* ----" not in tail and "/* ====" not in tail and "/* ####" not in tail
    assert tail.rstrip().endswith("#ifdef __cplusplus\n}\n#endif\n#endif /* HNSW_MI355X_H */")
    para = re.sub(r"\s*\n \*\s*", " ", tail[:tail.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    for needle in ("0. ORDER", "hnsw_distance_batch", "over the float32 rows whatever row_format says", "N(X) with N(q)", "-0 below +0",
                   "a positive NaN above +inf", "The PAGED ORDER is (ord(D), node id)", "BEFORE the square root", "a caller never sees keys",
                   "a coarsening", "under inner product and cosine the two coincide", "v + id_base > c.id", "compared in 64 bits",
                   "{r, INT32_MAX}", "{r, id_base - 1}", "A NaN c.dist is HNSW_ERR_BAD_ARG", "before any launch",
                   "1. ELIGIBLE", "not marked deleted", "2. hnsw_brute_force_batch_after", "It needs no graph", "n = 0 is HNSW_OK",
                   "never depends on option scan_slabs or on the row format", "3. hnsw_search_batch_after", "(ef = e, k = e)",
                   "re-ranked with k := e", "e_{j+1} = min(1024, 2 e_j)", "UNDER THE PAGED ORDER", "only runs of equal D",
                   "ascending query order", "EXACT STAGE", "0xFFFFFFFF", "The walk is never modified", "4. out_next[q]",
                   "the input cursor when the row has none", "\"exhausted\"", "5. CONSEQUENCES", "pairwise disjoint",
                   "are the full paged order", "bit for bit where the row's distances are distinct", "6. COUNTERS",
                   "adds the number of allowed live nodes", "outputs are untouched on error", "7. DETERMINISM", "8. Scratch is the handle's",
                   "9. NOT BUILT", "device-pointer forms", "per-query filters", "hnsw_index_keys_of", "hnsw_sharded and hnsw_multi forms",
                   "RENUMBER the nodes", "10. COST", "past about rank 1024 - k", "walks the whole ladder first"):
        assert needle in para, needle
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("hnsw_search_batch_after", "hnsw_brute_force_batch_after", "after_select_kernel", "ScanAfter", "l2_key_hi", "a coarsening"):
        assert needle in design, needle
    assert "hnsw_search_batch_after" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hnsw_search_batch_after" in open(os.path.join(ROOT, "README.md")).read()


def test_null_handles_null_arrays_negative_counts_and_nan_cursors_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 4, 0, 0)
    q = (ctypes.c_float * 4)(1, 2, 3, 4)
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    dist = (ctypes.c_float * 4)(7, 7, 7, 7)
    cur = np.array([(0.5, 3)], dtype=H.CURSOR_DTYPE)
    nan = np.array([(np.nan, 3)], dtype=H.CURSOR_DTYPE)
    nxt = np.array([(7.0, 7)], dtype=H.CURSOR_DTYPE)
    nd, nh, st = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    tail = (H._ptr(nxt), ctypes.byref(nd), ctypes.byref(nh), ctypes.byref(st))
    for c in (cur, nan, None):
        assert L.hnsw_search_batch_after(None, None, H._ptr(c) if c is not None else None, q, 1, 4, ctypes.byref(p), ids, dist, *tail) == H.ERR_BAD_ARG
        assert b"null" in L.hnsw_last_error()
        assert L.hnsw_brute_force_batch_after(None, None, H._ptr(c) if c is not None else None, q, 1, 4, 4, 0, ids, dist, H._ptr(nxt)) == H.ERR_BAD_ARG
        assert b"null" in L.hnsw_last_error()
    assert L.hnsw_search_batch_after(None, None, None, None, 1, 4, ctypes.byref(p), None, None, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_search_batch_after(None, None, None, q, 1, 4, None, ids, dist, *tail) == H.ERR_BAD_ARG
    assert L.hnsw_search_batch_after(None, None, H._ptr(cur), q, -1, 4, ctypes.byref(p), ids, dist, *tail) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch_after(None, None, None, None, 1, 4, 4, 0, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_brute_force_batch_after(None, None, H._ptr(cur), q, -1, 4, 4, 0, ids, dist, H._ptr(nxt)) == H.ERR_BAD_ARG
    assert list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and nxt[0]["dist"] == 7.0 and nxt[0]["id"] == 7
    assert nd.value == 7 and nh.value == 7 and st.value == 7


def test_python_shapes_the_cursors(H):
    class Fake:
        d, n, metric, id_base, handle = 4, 0, 0, 0, None
    with pytest.raises(H.InvalidArgument, match="one cursor per query"):
        H.Ohnsw.brute_force_after(Fake(), 3, np.zeros((3, 4), np.float32), after=np.zeros(2, H.CURSOR_DTYPE))
    with pytest.raises(H.InvalidArgument, match="batch must be"):
        H.Ohnsw.knn_batch_after(Fake(), 3, np.zeros((3, 5), np.float32))
    one = H._cursors(H.CURSOR_START, 3)
    assert one.shape == (3,) and (one["dist"] == -np.inf).all() and (one["id"] == -2 ** 31).all()
    assert H._cursors(None, 3) is None


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_after.hip" in b.SOURCES and "hnsw_after.hip" in b.DEPS and "hnsw_after_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16


@pytest.mark.parametrize("sanitize", [False, True])
def test_after_plan_against_its_definitions(tmp_path, sanitize):
    """ord strictly monotone over a sweep with +-0, subnormals, +-inf and a NaN; "after" and the cursor's word against a naive tuple
    compare; the next cursor; hi(D) = max{s : sqrtf(s) <= D} through the neighbouring floats for more than 10^5 values of D:
    tests/cpp/test_after_plan.cpp, a host program, built with the host compiler and, a second time, under AddressSanitizer and
    UndefinedBehaviorSanitizer (a stand-alone binary)"""
    exe = str(tmp_path / "test_after_plan")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_after_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"after plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 100000, out.stdout + out.stderr
