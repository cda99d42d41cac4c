"""CPU-side checks of the upsert (ocaml-hnsw_amd/csrc/hnsw_upsert.hip): the two entry points exist in the library and in every front
end, the ABI version stays, the header's last section states the definition, null handles, null arrays and m < 0 are refused on the
host, and the arithmetic that is plain numbers (hnsw_upsert_plan.h: the split of a call into stored and new rows, the node counts,
the out_new_id / out_replaced fills, the refusals, the smallest duplicated key) holds against a naive restatement."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_index_upsert_keyed", "hnsw_index_update")
ARITY = (8, 7)


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
    # counts and strides cross the ABI as 64-bit values, not as ctypes' default C int
    assert L.hnsw_index_upsert_keyed.argtypes[3] is ctypes.c_int64 and L.hnsw_index_upsert_keyed.argtypes[4] is ctypes.c_int64
    assert L.hnsw_index_update.argtypes[3] is ctypes.c_int64 and L.hnsw_index_update.argtypes[4] is ctypes.c_int64
    for fn in (H.Ohnsw.upsert_batch_keyed, H.Ohnsw.update_batch, H.Hgraph.upsert):
        assert callable(fn)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let upsert_batch_keyed ", "let update_batch "):
        assert wrapper in ml, wrapper
    for fn in ("upsert_keyed(", "update("):
        assert fn in hpp, fn
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_upsert.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    start = hdr.index("==== upsert: replace or add vectors")
    # the new section is the header's last: nothing of the existing text moved
    assert start > hdr.index("int32_t hnsw_knn_graph(")
    tail = hdr[start:]
    assert "/* ----" not in tail and "/* ====" not in tail[4:]
    assert tail.rstrip().endswith("#ifdef __cplusplus\n}\n#endif\n#endif /* HNSW_MI355X_H */")
    para = re.sub(r"\s*\n \*\s*", " ", tail[:tail.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    for needle in ("THE DEFINITION is ONE equivalence", "hnsw_index_remove_keys", "hnsw_index_insert_keyed", "in the call's order",
                   "link for link on every layer", "row for row", "level for level", "key for key", "entry point and max_layer",
                   "hnsw_index_sq8_params", "hnsw_index_sq8_dim_params", "hnsw_index_bit_params", "the marks", "bit for bit",
                   "moves on once", "n_old - |P|", "comes back live", "hnsw_index_remove(ids)", "hnsw_index_insert(X)",
                   "pointing at the keyed call", "id_base - 1 for a replaced node", "m == 0 is a no-op", "the identity",
                   "the call IS hnsw_index_insert_keyed", "equals hnsw_build of X", "two equal keys in the call", "the smallest such key",
                   "an EMPTY index without keys", "an id out of range or repeated",
                   "submitted requests not waited for", "a replica of an hnsw_multi", "a shard of an hnsw_sharded", "rows wider than 2M / M",
                   "a NaN or infinite new value", "holds no query of the final n", "All or nothing", "HNSW_ERR_OOM",
                   "a degree overflow that exhausts its retries", "exactly as before", "filters made before still accepted",
                   "two copies", "a third copy", "runs the removal again",
                   "NOT BUILT", "upsert for hnsw_sharded and hnsw_multi", "an in-place update that keeps the node's id", "saved keys"):
        assert needle in para, needle
    # the keys section keeps its NOT BUILT paragraph and points here
    keys = hdr[hdr.index("---- keys: stable 64-bit names"):hdr.index("int32_t hnsw_index_set_keys(")]
    keys = re.sub(r"\s*\n \*\s*", " ", keys)
    assert "NOT BUILT: keys for hnsw_sharded and hnsw_multi" in keys and "upsert" in keys and "hnsw_index_upsert_keyed" in keys
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("hnsw_index_upsert_keyed", "hnsw_index_update", "grow_graph_in_place", "remove_graph", "One swap", "two copies",
                   "runs the removal again", "Not built:"):
        assert needle in design, needle
    assert "hnsw_index_upsert_keyed" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hnsw_index_upsert_keyed" in open(os.path.join(ROOT, "README.md")).read()


def test_null_handles_null_arrays_and_negative_counts_are_refused_on_the_host(H):
    L = H.load()
    b = H._BuildParams(8, 40, 0, 0, 1, 0, 0, 0, 0)
    key, f32, i32, u8 = ctypes.c_int64(5), ctypes.c_float(7.0), ctypes.c_int32(7), ctypes.c_uint8(7)
    args = (ctypes.byref(f32), ctypes.byref(key), 1, 1, ctypes.byref(b), ctypes.byref(u8), ctypes.byref(i32))
    assert L.hnsw_index_upsert_keyed(None, *args) == H.ERR_BAD_ARG
    assert b"null" in L.hnsw_last_error()
    assert L.hnsw_index_upsert_keyed(None, None, None, 0, 0, ctypes.byref(b), None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_upsert_keyed(None, None, None, 0, 0, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_upsert_keyed(None, ctypes.byref(f32), ctypes.byref(key), -1, 1, ctypes.byref(b), None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_update(None, ctypes.byref(key), ctypes.byref(f32), 1, 1, ctypes.byref(b), ctypes.byref(i32)) == H.ERR_BAD_ARG
    assert L.hnsw_index_update(None, None, None, 0, 0, ctypes.byref(b), None) == H.ERR_BAD_ARG
    assert L.hnsw_index_update(None, None, None, 0, 0, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_index_update(None, ctypes.byref(key), ctypes.byref(f32), -1, 1, ctypes.byref(b), None) == H.ERR_BAD_ARG
    assert key.value == 5 and f32.value == 7.0 and i32.value == 7 and u8.value == 7
    assert b"null" in L.hnsw_last_error()


def test_python_refuses_mismatched_counts(H):
    import numpy as np

    class Fake:
        d, n, metric, id_base = 4, 0, 0, 0
    with pytest.raises(H.InvalidArgument, match="keys for"):
        H.Ohnsw.upsert_batch_keyed(Fake(), np.zeros((3, 4), np.float32), [1, 2], 8, 40)
    with pytest.raises(H.InvalidArgument, match="ids for"):
        H.Ohnsw.update_batch(Fake(), [1, 2], np.zeros((3, 4), np.float32), 8, 40)
    with pytest.raises(H.InvalidArgument, match="index's d"):
        H.Ohnsw.upsert_batch_keyed(Fake(), np.zeros((2, 5), np.float32), [1, 2], 8, 40)


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_upsert.hip" in b.SOURCES and "hnsw_upsert.hip" in b.DEPS and "hnsw_upsert_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16


@pytest.mark.parametrize("sanitize", [False, True])
def test_upsert_plan_against_a_naive_restatement(tmp_path, sanitize):
    """the partition, the positions, the out_new_id / out_replaced fills, duplicate detection naming the smallest key, over the cases
    all stored, none stored, m == 0 and every node replaced: tests/cpp/test_upsert_plan.cpp, a host program, built with the host
    compiler and, a second time, under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone binary)"""
    exe = str(tmp_path / "test_upsert_plan")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_upsert_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"upsert plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
