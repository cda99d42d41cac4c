"""CPU-side checks of the sharded index's query calls (ocaml-hnsw_amd/csrc/hnsw_sharded.hip): the sharded filter, filtered k-NN,
range search and the segment merge exist in the library and in every front end with the header's arity, the header section states
the definition, and what can be refused without a device is refused on the host."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ("hnsw_sharded_filter_create", "hnsw_sharded_filter_destroy", "hnsw_sharded_filter_count", "hnsw_sharded_filter_part",
           "hnsw_sharded_search_batch_filtered", "hnsw_sharded_range_search_batch", "hnsw_sharded_range_brute_force_batch",
           "hnsw_sharded_range_result_size", "hnsw_sharded_range_result_fetch", "hnsw_sharded_range_result_device",
           "hnsw_sharded_range_result_destroy", "hnsw_merge_segments")
ARITY = (4, 1, 2, 3, 11, 7, 7, 3, 7, 4, 1, 9)


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
    sec = hdr[hdr.index("---- sharded index: a filter over the global rows"):]
    return sec[:sec.index("*/")]


def test_symbols_are_declared_exported_and_mirrored(H):
    L = H.load()
    hdr = _header()
    for name, arity in zip(SYMBOLS, ARITY):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert name in H.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity and fn.restype is ctypes.c_int32, name
    assert "typedef struct hnsw_sharded_filter hnsw_sharded_filter;" in hdr
    assert "typedef struct hnsw_sharded_range_result hnsw_sharded_range_result;" in hdr
    for method in ("filter", "knn_batch_filtered", "range_search", "brute_force_range"):
        assert callable(getattr(H.ShardedHgraph, method)), method
    for method in ("count", "part_bits", "release"):
        assert callable(getattr(H.ShardedFilter, method)), method
    for method in ("size", "fetch", "device_pointers", "release"):
        assert callable(getattr(H.ShardedRangeResult, method)), method
    assert callable(H.merge_segments)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3           # additive entry points: the version stays


def test_other_front_ends_bind_the_symbols():
    ml = open(os.path.join(ROOT, "ocaml-hnsw_amd", "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(ROOT, "ocaml-hnsw_amd", "host", "hnsw_front.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r'foreign[^"]*"%s"' % name, ml), name
        assert name in hpp, name
    for wrapper in ("let sharded_filter_create ", "let sharded_knn_batch_filtered ", "let sharded_range_search ",
                    "let sharded_brute_force_range ", "let merge_segments "):
        assert wrapper in ml, wrapper
    for piece in ("class ShardedFilter", "class ShardedRangeResult", "knn_filtered(const ShardedFilter", "ShardedRangeResult range_search(",
                  "ShardedRangeResult brute_force_range(", "inline ShardedRangeResult merge_segments("):
        assert piece in hpp, piece
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_front_sharded_query.cpp"))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"test_front_sharded_query"' in entry                # build() compiles the driver


def test_header_states_the_definition():
    sec = _section()
    for needle in ("(distance, global id)", "maximum over the shards", "lims[q] = the sum over g of lims_g[q]", "2^31 - 1", "lower list",
                   "NOT part", "hnsw_filter_create_by_label", "hnsw_search_batch_filtered_each", "GLOBAL rows", "bit v & 31 of word v >> 5",
                   "n = lo_G", "hnsw_filter_create(shard g, B_g, n_g)", "All or nothing", "never goes stale", "another hnsw_sharded",
                   "hnsw_search_batch_filtered(shard g, f's part g", "sums over the", "0xFFFFFFFF", "HNSW_SEM_FUNCTOR_NEAREST_K",
                   "HNSW_ERR_EMPTY_INDEX", "first_row[g] + id", "IEEE <", "ROUNDING EXCEPTION", "HNSW_ERR_UNSUPPORTED", "one host thread per shard",
                   "at most 16", "peer copies", "ONE call in flight", "n_lists in 1..64", "non-decreasing", "counters read as 0",
                   "insert, remove and marks"):
        assert needle in sec, needle
    # the first sharded section keeps its wording and points here
    hdr = _header()
    first = hdr[hdr.index("---- sharded index"):]
    first = first[:first.index("*/")]
    assert "Sharded insert, remove and marks are NOT BUILT; filters and range calls: see below." in first


def test_null_handles_and_null_out_are_refused_on_the_host(H):
    L = H.load()
    out = ctypes.c_void_p(1)
    c = ctypes.c_int64(7)
    bits = (ctypes.c_uint32 * 4)()
    assert L.hnsw_sharded_filter_create(None, bits, 8, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_sharded_filter_create(None, bits, 8, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_filter_destroy(None) == H.OK
    assert L.hnsw_sharded_filter_count(None, ctypes.byref(c)) == H.ERR_BAD_ARG and c.value == 7
    assert L.hnsw_sharded_filter_part(None, 0, ctypes.byref(out)) == H.ERR_BAD_ARG
    sp = H._SearchParams(16, 10, 0, 0)
    assert L.hnsw_sharded_search_batch_filtered(None, None, None, 0, 0, ctypes.byref(sp), None, None, None, None, None) == H.ERR_BAD_ARG
    rp = H._RangeParams(1.0, 16, 0)
    out.value = 1
    assert L.hnsw_sharded_range_search_batch(None, None, None, 0, 0, ctypes.byref(rp), ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_sharded_range_search_batch(None, None, None, 0, 0, ctypes.byref(rp), None) == H.ERR_BAD_ARG
    out.value = 1
    assert L.hnsw_sharded_range_brute_force_batch(None, None, None, 0, 0, 1.0, ctypes.byref(out)) == H.ERR_BAD_ARG and out.value is None
    assert L.hnsw_sharded_range_brute_force_batch(None, None, None, 0, 0, 1.0, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_range_result_size(None, ctypes.byref(c), ctypes.byref(c)) == H.ERR_BAD_ARG and c.value == 7
    assert L.hnsw_sharded_range_result_fetch(None, None, None, None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_range_result_device(None, None, None, None) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_range_result_destroy(None) == H.OK


def test_merge_segments_checks_its_ranges_on_the_host(H):
    L = H.load()
    lims_ok = (ctypes.c_int64 * 2)(0, 1)
    ids = (ctypes.c_int32 * 2)()
    dist = (ctypes.c_float * 2)()
    first = (ctypes.c_int64 * 65)()
    out = ctypes.c_void_p(1)

    def table(*arrays):
        return (ctypes.c_void_p * 65)(*[ctypes.addressof(a) for a in arrays])

    def call(n_lists=2, nq=1, lims=(lims_ok, lims_ok), first_row=first, o=out):
        out.value = 1
        lt = table(*lims) if lims is not None else None
        rc = L.hnsw_merge_segments(0, n_lists, nq, lt, table(ids, ids), table(dist, dist), first_row, 0, ctypes.byref(o) if o is not None else None)
        return rc

    for bad in (dict(n_lists=0), dict(n_lists=65), dict(nq=-1), dict(lims=None), dict(first_row=None)):
        assert call(**bad) == H.ERR_BAD_ARG and out.value is None, bad
    assert call(o=None) == H.ERR_BAD_ARG
    assert call(first_row=(ctypes.c_int64 * 2)(5, 4)) == H.ERR_BAD_ARG and out.value is None       # first_row must be non-decreasing
    assert call(lims=(lims_ok, (ctypes.c_int64 * 2)(1, 1))) == H.ERR_BAD_ARG and out.value is None   # a lims must start at 0
    assert call(nq=2, lims=((ctypes.c_int64 * 3)(0, 1, 1), (ctypes.c_int64 * 3)(0, 2, 1))) == H.ERR_BAD_ARG and out.value is None   # ... and not decrease
    huge = (ctypes.c_int64 * 2)(0, 2 ** 31 - 1)                 # two lists of 2^31 - 1 entries: too many, found before anything is read
    assert call(lims=(huge, huge)) == H.ERR_UNSUPPORTED and out.value is None
    with pytest.raises(H.InvalidArgument):
        H.merge_segments([[0, 1]], [[0, 1]], [[0.5]], [0])      # ids[g] has not lims[g][nq] entries
    with pytest.raises(H.InvalidArgument):
        H.merge_segments([[0, 1], [0, 1, 1]], [[0], [0]], [[0.5], [0.5]], [0, 0])
