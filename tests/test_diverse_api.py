"""CPU-side checks of the diversified searches (ocaml-hnsw_amd/csrc/hnsw_diverse.hip): the four entry points exist in the library and
in every front end with the header's arity, the ABI version stays, the header's last section states the definition, the refusals
that need no device leave the outputs untouched (a NaN lambda, lambda -0.1 and 1.5, null handles and arrays, nq < 0, bad strides and
k), build.py lists the new source with the variant counts of before, and the arithmetic that is plain numbers (hnsw_diverse_plan.h)
holds against its definitions, plainly and under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_diversify_batch", "hnsw_diversify_batch_device", "hnsw_search_batch_diverse", "hnsw_brute_force_batch_diverse")
ARITY = (12, 13, 14, 11)


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
        decl = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("int32_t %s(" % name):], flags=re.S)
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == arity, name                       # the header's own argument list
    # counts and strides cross the ABI as 64-bit values, lambda as a C float
    for name in ("hnsw_diversify_batch", "hnsw_diversify_batch_device", "hnsw_brute_force_batch_diverse"):
        assert getattr(L, name).argtypes[2] is ctypes.c_int64 and getattr(L, name).argtypes[3] is ctypes.c_int64
    assert L.hnsw_search_batch_diverse.argtypes[3] is ctypes.c_int64 and L.hnsw_search_batch_diverse.argtypes[4] is ctypes.c_int64
    assert L.hnsw_diversify_batch.argtypes[7] is ctypes.c_float and L.hnsw_diversify_batch_device.argtypes[7] is ctypes.c_float
    assert L.hnsw_search_batch_diverse.argtypes[7] is ctypes.c_float and L.hnsw_brute_force_batch_diverse.argtypes[6] is ctypes.c_float
    for fn in (H.Ohnsw.diversify, H.Ohnsw.knn_batch_diverse, H.Ohnsw.brute_force_diverse, H.Ba.knn_batch_diverse, H.diversify_device):
        assert callable(fn)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in ("hnsw_diversify_batch", "hnsw_search_batch_diverse", "hnsw_brute_force_batch_diverse"):
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name + "(" in hpp, name
    for wrapper in ("let diversify ", "let knn_batch_diverse ", "let brute_force_diverse "):
        assert wrapper in ml, wrapper
    for fn in ("struct Diverse", "inline Diverse diversify(", "inline Diverse knn_diverse(", "inline Diverse brute_force_diverse("):
        assert fn in hpp, fn
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_diverse.cpp"))


def test_header_states_the_definition():
    hdr = _header()
    start = hdr.index("++++ diversified k-NN search")
    # the new section is the header's last: nothing of the existing text moved
    assert start > hdr.index("int32_t hnsw_brute_force_batch_after(")
    tail = hdr[start:]
    assert "/* ----" not in tail and "/* ====" not in tail and "/* ####" not in tail and "/* ++++" not in tail
    assert tail.rstrip().endswith("#ifdef __cplusplus\n}\n#endif\n#endif /* HNSW_MI355X_H */")
    para = re.sub(r"\s*\n \*\s*", " ", tail[:tail.index("*/")])        # (the comment's line breaks: a phrase may span two lines)
    for needle in ("0. THE OPERATOR", "ONE definition", "exactly hnsw_rerank_batch's", "entries < id_base are padding", "cand_stride in 1..1024",
                   "the device form skips it", "1. THE NUMBERS", "the float hnsw_distance_batch returns", "whatever row_format says",
                   "with k = cand_stride", "no new order is invented", "the stored float32 row of s as the query", "N(X) called with N(Q)",
                   "not normalised again", "2. SELECTION", "mu = fl(1.0f - lambda)", "Pick 1 is the candidate of rank 0",
                   "g(v) = fl( fl(lambda * r(v)) - fl(mu * m(v)) )", "no fused multiply-add", "-0 equals +0", "the smallest rank wins",
                   "3. OUTPUT", "SELECTION ORDER", "+inf for pick 1", "out_div the same float", "with lambda = 1",
                   "bit for bit hnsw_rerank_batch's", "its own candidates only", "no promise", "outputs untouched", "nq == 0 is a no-op",
                   "HNSW_ERR_UNSUPPORTED", "lambda NaN or outside [0, 1]", "4. THE SEARCHES", "hnsw_search_batch with k := pool",
                   "params->k <= pool <= params->ef", "inherited, not restated", "option refine", "the tie-overflow repair",
                   "option filter_collect", "reads the ids where the search left them", "k <= pool <= 1024", "It takes no filter",
                   "not counted in device_bytes", "6. NOT BUILT", "per-query filters", "hnsw_index_keys_of", "device-pointer forms",
                   "hnsw_sharded and hnsw_multi forms", "a per-query lambda", "7. COST", "tools/diverse_rate.py"):
        assert needle in para, needle
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("hnsw_diversify_kernel", "hnsw_diversify_batch", "hnsw_search_batch_diverse", "hnsw_brute_force_batch_diverse", "DiverseOut",
                   "wave_min_u64"):
        assert needle in design, needle
    assert "hnsw_search_batch_diverse" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hnsw_search_batch_diverse" in open(os.path.join(ROOT, "README.md")).read()


def _outputs():
    ids = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    dist = (ctypes.c_float * 4)(7, 7, 7, 7)
    div = (ctypes.c_float * 4)(7, 7, 7, 7)
    return ids, dist, div


def _untouched(ids, dist, div):
    return list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and list(div) == [7.0] * 4


@pytest.mark.parametrize("lam", [float("nan"), -0.1, 1.5, float("inf")])
def test_a_lambda_outside_the_unit_interval_is_refused_on_the_host(H, lam):
    """every entry point names lambda before it looks at the handle: refused with no device, outputs untouched"""
    L = H.load()
    p = H._SearchParams(16, 4, 0, 0)
    q = (ctypes.c_float * 4)(1, 2, 3, 4)
    cand = (ctypes.c_int32 * 8)(*range(8))
    ids, dist, div = _outputs()
    nd, nh, st = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    calls = (lambda: L.hnsw_diversify_batch(None, q, 1, 4, cand, 8, 4, lam, 0, ids, dist, div),
             lambda: L.hnsw_diversify_batch_device(None, q, 1, 4, cand, 8, 4, lam, 0, ids, dist, div, None),
             lambda: L.hnsw_search_batch_diverse(None, None, q, 1, 4, ctypes.byref(p), 8, lam, ids, dist, div, ctypes.byref(nd), ctypes.byref(nh),
                                                 ctypes.byref(st)),
             lambda: L.hnsw_brute_force_batch_diverse(None, q, 1, 4, 4, 8, lam, 0, ids, dist, div))
    for call in calls:
        assert call() == H.ERR_BAD_ARG
        assert b"lambda" in L.hnsw_last_error()
    assert _untouched(ids, dist, div) and nd.value == 7 and nh.value == 7 and st.value == 7


def test_null_handles_and_bad_numbers_are_refused_on_the_host(H):
    L = H.load()
    p = H._SearchParams(16, 4, 0, 0)
    q = (ctypes.c_float * 4)(1, 2, 3, 4)
    cand = (ctypes.c_int32 * 8)(*range(8))
    ids, dist, div = _outputs()
    # a null handle, everything else in order
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 8, 4, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"null" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch_device(None, q, 1, 4, cand, 8, 4, 0.5, 0, ids, dist, div, None) == H.ERR_BAD_ARG and b"null" in L.hnsw_last_error()
    assert L.hnsw_search_batch_diverse(None, None, q, 1, 4, ctypes.byref(p), 8, 0.5, ids, dist, div, None, None, None) == H.ERR_BAD_ARG
    assert b"null" in L.hnsw_last_error()
    assert L.hnsw_brute_force_batch_diverse(None, q, 1, 4, 4, 8, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"null" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, 0, 4, cand, 8, 4, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG     # (nq == 0 does not excuse it)
    # the operator's plain numbers, refused before the handle is looked at
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 0, 1, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"cand_stride" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 1025, 4, 0.5, 0, ids, dist, div) == H.ERR_UNSUPPORTED and b"1024" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 8, 0, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"k must be" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 8, 9, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"k must be" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, 1, 4, cand, 8, 4, 0.5, 2, ids, dist, div) == H.ERR_BAD_ARG and b"fill" in L.hnsw_last_error()
    assert L.hnsw_diversify_batch(None, q, -1, 4, cand, 8, 4, 0.5, 0, ids, dist, div) == H.ERR_BAD_ARG and b"nq" in L.hnsw_last_error()
    assert L.hnsw_search_batch_diverse(None, None, q, 1, 4, None, 8, 0.5, ids, dist, div, None, None, None) == H.ERR_BAD_ARG
    assert _untouched(ids, dist, div)


def test_python_shapes_the_arguments(H):
    class Fake:
        d, n, metric, id_base, handle = 4, 0, 0, 0, None
    with pytest.raises(H.InvalidArgument, match=r"cand must be \[nq\]\[cand_stride\]"):
        H.Ohnsw.diversify(Fake(), 2, np.zeros((3, 4), np.float32), np.zeros((2, 5), np.int32))
    with pytest.raises(H.InvalidArgument, match="batch must be"):
        H.Ohnsw.knn_batch_diverse(Fake(), 3, np.zeros((3, 5), np.float32), pool=8)
    with pytest.raises(H.InvalidArgument, match="lambda"):
        H.Ohnsw.brute_force_diverse(Fake(), 3, np.zeros((3, 4), np.float32), pool=8, lam=2.0)


def test_build_lists_the_new_source_and_no_new_variant():
    import __graft_entry__ as ge
    b = ge._load_build_module()
    assert "hnsw_diverse.hip" in b.SOURCES and "hnsw_diverse.hip" in b.DEPS and "hnsw_diverse_plan.h" in b.DEPS
    assert len(b.VARIANTS) == 20 and len(b.COLLECT_VARIANTS) == 16
    assert len(b.SQ8_DIM_WALKS) == 2 and len(b.BITS_WALKS) == 2 and len(b.BITS_ASYM_WALKS) == 2


@pytest.mark.parametrize("sanitize", [False, True])
def test_diverse_plan_against_its_definitions(tmp_path, sanitize):
    """the refusals; mu and g as three rounded operations against a by-hand rounding (a fused multiply-add is told apart); g's ordered
    word with the zeros folded; the argmin's word; the LDS of a wave; the selection rule against a naive restatement over random and
    heavily tied inputs: tests/cpp/test_diverse_plan.cpp, a host program, built with the host compiler and, a second time, under
    AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone binary)"""
    exe = str(tmp_path / "test_diverse_plan")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "test_diverse_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"diverse plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 100000, out.stdout + out.stderr
