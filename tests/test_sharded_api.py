"""CPU-side checks of the sharded index (ocaml-hnsw_amd/csrc/hnsw_sharded.hip): the entry points exist in the library and in every
front end with the header's arity, the ABI version stays, the header section states the definition, and what can be refused
without a device is refused on the host."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_sharded_build", "hnsw_sharded_create", "hnsw_sharded_load", "hnsw_sharded_destroy", "hnsw_sharded_num_shards",
           "hnsw_sharded_shard", "hnsw_sharded_get_info", "hnsw_sharded_set_option", "hnsw_sharded_search_batch",
           "hnsw_sharded_brute_force_batch", "hnsw_merge_lists")
ARITY = (8, 4, 4, 1, 2, 4, 6, 3, 9, 8, 12)


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def _section():
    hdr = _header()
    sec = hdr[hdr.index("---- sharded index"):]
    return sec[:sec.index("*/")]


def test_symbols_are_declared_exported_and_mirrored(H):
    L = H.load()
    hdr = _header()
    for name, arity in zip(SYMBOLS, ARITY):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32, name
    assert "typedef struct hnsw_sharded hnsw_sharded;" in hdr
    for method in ("build", "create", "load", "save", "shard", "info", "set_option", "release", "knn_batch", "brute_force_knn"):
        assert callable(getattr(H.ShardedHgraph, method)), method
    assert callable(H.merge_lists)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let sharded_build ", "let sharded_knn_batch ", "let sharded_brute_force ", "let merge_lists "):
        assert wrapper in ml, wrapper
    assert "class Sharded" in hpp and "merge_lists(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_sharded.cpp"))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"test_front_sharded"' in entry                      # build() compiles the driver
    build = open(os.path.join(ROOT, "ocaml-hnsw_amd", "build.py")).read()
    assert '"hnsw_sharded.hip"' in build


def test_header_states_the_definition():
    sec = _section()
    for needle in ("floor(n * g / G)", "seed + g", "(distance, global id)", "int64", "1..64", "NOT BUILT", "ROUNDING EXCEPTION",
                   "pre-square-root key", "integers below 2^16", "lo_g + v + id_base", "first_row = lo_g", "n < n_shards",
                   "more than once", "hnsw_build(vectors + lo_g * row_stride", "LOCAL ids", "running sum", "hnsw_index_load",
                   "hnsw_index_save", "hnsw_index_insert, hnsw_index_remove and hnsw_index_mark_deleted", "set back",
                   "hnsw_search_batch returns", "IEEE <", "sums over the shards", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "HNSW_ERR_EMPTY_INDEX", "DETERMINISM", "hnsw_brute_force_batch(shard g, k)", "bit for bit", "devices[0]",
                   "ONE call in flight per handle", "[n_lists][nq][k_in]", "non-decreasing", "k_in in 1..1024", "k_out in 1..1024",
                   "nq == 0 is a no-op"):
        assert needle in sec, needle


def test_bad_arguments_are_refused_on_the_host(H):
    L = H.load()
    out = ctypes.c_void_p(1)
    dev = (ctypes.c_int32 * 65)()
    x = (ctypes.c_float * 8)()
    p = H._BuildParams(8, 40, 0, 0, 11, 0, 0, 0, 0)
    # n_shards outside 1..64, n < n_shards: refused before anything is built, *out NULL
    for n, g in ((8, 0), (8, 65), (2, 3)):
        out.value = 1
        assert L.hnsw_sharded_build(x, n, 1, 1, ctypes.byref(p), dev, g, ctypes.byref(out)) == H.ERR_BAD_ARG, (n, g)
        assert out.value is None
    for g in (0, 65):
        out.value = 1
        assert L.hnsw_sharded_create(dev, dev, g, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
        out.value = 1
        assert L.hnsw_sharded_load(dev, dev, g, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_sharded_build(None, 8, 1, 1, ctypes.byref(p), dev, 2, ctypes.byref(out)) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_build(x, 8, 1, 1, ctypes.byref(p), dev, 2, None) == H.ERR_BAD_ARG
    # null handles
    c = ctypes.c_int32(7)
    assert L.hnsw_sharded_destroy(None) == H.OK
    assert L.hnsw_sharded_num_shards(None, ctypes.byref(c)) == H.ERR_BAD_ARG and c.value == 7
    assert L.hnsw_sharded_shard(None, 0, ctypes.byref(out), None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_get_info(None, None, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_set_option(None, b"refine", 0) == H.ERR_BAD_ARG
    sp = H._SearchParams(16, 10, 0, 0)
    assert L.hnsw_sharded_search_batch(None, None, 0, 0, ctypes.byref(sp), None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_brute_force_batch(None, None, 0, 0, 10, 0, None, None) == H.ERR_BAD_ARG


def test_merge_lists_checks_its_ranges_on_the_host(H):
    L = H.load()
    ids = (ctypes.c_int32 * 4)()
    dist = (ctypes.c_float * 4)()
    first = (ctypes.c_int64 * 65)()
    oi = (ctypes.c_int64 * 4)()
    od = (ctypes.c_float * 4)()

    def call(n_lists=2, nq=1, k_in=2, k_out=2, fill=0, first_row=first, i=ids):
        return L.hnsw_merge_lists(0, i, dist, first_row, n_lists, nq, k_in, k_out, 0, fill, oi, od)

    for bad in (dict(n_lists=0), dict(n_lists=65), dict(k_in=0), dict(k_in=1025), dict(k_out=0), dict(k_out=1025), dict(fill=2),
                dict(nq=-1), dict(i=None)):
        assert call(**bad) == H.ERR_BAD_ARG, bad
    down = (ctypes.c_int64 * 2)(5, 4)
    assert call(first_row=down) == H.ERR_BAD_ARG                # first_row must be non-decreasing
    assert call(nq=0) == H.OK                                   # a no-op: no device is touched
    assert call(nq=0, i=None) == H.OK


def test_shard_plan_against_a_naive_restatement(tmp_path):
    """shard_lo, cut_mask, SegPlan and check_lims (hnsw_shard_plan.h: the partition bound, the cut of a global mask into per-shard
    masks, the segment merge's bases and its two refusals, the lims validation): tests/cpp/test_shard_plan.cpp, a host program,
    under AddressSanitizer and UndefinedBehaviorSanitizer"""
    import subprocess
    exe = str(tmp_path / "test_shard_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_shard_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    done = re.search(r"shard plan ok: (\d+) cases, 0 differ", out.stdout)
    assert out.returncode == 0 and done and int(done.group(1)) > 0, out.stdout + out.stderr
