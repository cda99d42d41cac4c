"""CPU-side checks of HNSW_METRIC_COSINE (ocaml-hnsw_amd/csrc/hnsw_cosine.hip): the header declares the metric and its two entry
points and states the contract they follow from, the three front ends name them, dataset.metric_of maps the ann-benchmarks names,
and without a device the normaliser fails loudly."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "ocaml-hnsw_amd")


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge._load_build_module().build()
    import ocaml_hnsw_amd as H
    H.load()
    return H


def _header():
    return open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()


def test_header_declares_the_metric_and_both_functions(H):
    hdr = _header()
    assert re.search(r"HNSW_METRIC_COSINE\s*=\s*2\b", hdr)
    assert re.search(r"HNSW_METRIC_L2\s*=\s*0\b", hdr) and re.search(r"HNSW_METRIC_IP\s*=\s*1\b", hdr)
    assert H.METRIC_COSINE == 2 and (H.METRIC_L2, H.METRIC_IP) == (0, 1)
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+hnsw_normalise_batch\(int32_t device, const float \*in, int64_t n, int32_t d, int64_t in_stride, "
                     r"float \*out, int64_t out_stride,\s*float \*out_norms\s*\);", bare)
    assert re.search(r"int32_t\s+hnsw_index_get_rows\(const hnsw_index \*idx, const int64_t \*ids\s*, int64_t m,\s*float \*out, "
                     r"int64_t out_stride\);", bare)
    # new symbols and one enum value only: the ABI version is what it was
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)
    L = H.load()
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3
    for name, arity in (("hnsw_normalise_batch", 8), ("hnsw_index_get_rows", 5)):
        assert name in H.ABI_SYMBOLS and len(getattr(L, name).argtypes) == arity


def test_header_states_the_contract():
    hdr = " ".join(_header().replace("*", " ").split())
    for needle in (
            # the twin sentence
            "A COSINE index over X answers every call on queries Q with exactly the bits (ids, distances, counters, stages, graph links) "
            "of an IP index over N(X) called with N(Q)",
            # the normaliser: what it depends on, its order, the special rows
            "a function of the row's d values only",
            "acc = fma(v, v, acc)",
            "p[j] += p[j + 8 mod 16]; p[j] += p[j + 4 mod 16]; p[j] += p[j + 2 mod 16]; p[j] += p[j + 1 mod 16]",
            "norm = sqrt(s), correctly rounded",
            "A row whose sum of squares is 0 becomes all zeros, its norm reads 0, and its cosine distance to everything is 1",
            "A row whose sum of squares is NaN or infinite becomes all NaN",
            # the consequences
            "stores N(X) as its float32 rows",
            "all or nothing",
            "the message names the first such row",
            "zero rows are accepted",
            "on hnsw_index_load the rows are not normalised again: N(N(x)) is not N(x) bit for bit",
            "the file format stays 2",
            "report 2",
            "no head split",
            # the multi refusal
            'hnsw_multi_create refuses a COSINE desc with HNSW_ERR_UNSUPPORTED, "cosine: not built for hnsw_multi"',
            # the operators
            "n == 0 is HNSW_OK",
            "out may be in with the same stride (in == out with different strides: HNSW_ERR_BAD_ARG)",
            "one scratch matrix of the batch's size per caller stream",
            "cannot be recorded by a stream capture",
            "d > 1024: HNSW_ERR_UNSUPPORTED",
            "ids NULL: all n rows in order, m must be n",
            "nothing is written"):
        assert needle in hdr, needle


def test_front_ends_name_the_new_symbols():
    py = open(os.path.join(PKG, "__init__.py")).read()
    ml = open(os.path.join(PKG, "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(PKG, "host", "hnsw_front.hpp")).read()
    for needle in ("METRIC_COSINE = 2", "def normalise(X, device=0, norms=False)", "def rows(self, ids=None)", '"hnsw_normalise_batch"',
                   '"hnsw_index_get_rows"'):
        assert needle in py, needle
    for needle in ("let metric_cosine = 2", "let normalise ", "let rows ", 'foreign ~from:lib ~release_runtime_lock:true "hnsw_normalise_batch"',
                   'foreign ~from:lib ~release_runtime_lock:true "hnsw_index_get_rows"'):
        assert needle in ml, needle
    for needle in ("inline std::vector<float> normalise(const Mat &batch", "inline std::vector<float> rows(const Hgraph &g",
                   "hnsw_normalise_batch(", "hnsw_index_get_rows(", "HNSW_METRIC_COSINE"):
        assert needle in hpp, needle
    # the new translation unit is one the build compiles
    import __graft_entry__ as ge
    build = ge._load_build_module()
    assert "hnsw_cosine.hip" in build.SOURCES and "hnsw_cosine.hip" in build.DEPS
    assert len(build.VARIANTS) == 20 and len(build.COLLECT_VARIANTS) == 16       # no search-kernel variant was added


def test_metric_is_accepted_where_a_metric_is(H):
    import inspect
    for fn in (H.Hgraph.__init__, H.Hgraph.flat.__func__, H.Ohnsw.build_batch_bigarray, H.Ohnsw.insert_batch, H.ShardedHgraph.build.__func__):
        assert "metric" in inspect.signature(fn).parameters, fn
    X = np.eye(4, 8, dtype=np.float32)
    hg = H.Hgraph.flat(X, metric=H.METRIC_COSINE)
    assert hg.metric == 2 and hg._desc()[0].metric == 2
    assert hg.vectors is not None and np.array_equal(hg.vectors, X)         # the host copy stays the caller's matrix


def test_dataset_metric_of(H):
    import ocaml_hnsw_amd.dataset as dataset
    assert dataset.metric_of("euclidean") == H.METRIC_L2
    assert dataset.metric_of("angular") == H.METRIC_COSINE
    assert dataset.metric_of("cosine") == H.METRIC_COSINE
    assert dataset.metric_of(b"angular") == H.METRIC_COSINE                 # (an HDF5 attribute read as bytes)
    for other in ("hamming", "jaccard", "", "Angular", None, 2):
        with pytest.raises(H.InvalidArgument):
            dataset.metric_of(other)


def test_arguments_are_checked_on_the_host(H):
    L = H.load()
    x = np.ones((2, 4), np.float32)
    o = np.empty((2, 4), np.float32)
    p = H._ptr
    assert L.hnsw_normalise_batch(0, p(x), 0, 4, 4, p(o), 4, None) == H.OK              # n == 0: nothing to do, no device asked for
    assert L.hnsw_normalise_batch(0, p(x), 2, 1025, 1025, p(o), 1025, None) == H.ERR_UNSUPPORTED
    assert b"1024" in L.hnsw_last_error()
    assert L.hnsw_normalise_batch(0, p(x), 2, 0, 4, p(o), 4, None) == H.ERR_BAD_ARG
    assert L.hnsw_normalise_batch(0, p(x), -1, 4, 4, p(o), 4, None) == H.ERR_BAD_ARG
    assert L.hnsw_normalise_batch(0, None, 2, 4, 4, p(o), 4, None) == H.ERR_BAD_ARG
    assert L.hnsw_normalise_batch(0, p(x), 2, 4, 4, None, 4, None) == H.ERR_BAD_ARG
    assert L.hnsw_normalise_batch(0, p(x), 2, 4, 3, p(o), 4, None) == H.ERR_BAD_ARG     # short strides
    assert L.hnsw_normalise_batch(0, p(x), 2, 4, 4, p(o), 3, None) == H.ERR_BAD_ARG
    assert L.hnsw_normalise_batch(0, p(o), 1, 4, 4, p(o), 8, None) == H.ERR_BAD_ARG     # out is in, but at another stride
    assert L.hnsw_index_get_rows(None, None, 0, p(o), 4) == H.ERR_BAD_ARG
    with pytest.raises(H.InvalidArgument):
        H.normalise(np.ones(4, np.float32))                                             # not [n][d]


def test_fails_loudly_without_device(H):
    if H.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(H.Failure, match="no HIP device"):
        H.normalise(np.ones((3, 8), np.float32))
    hg = H.Hgraph.flat(np.eye(4, 8, dtype=np.float32), metric=H.METRIC_COSINE)
    with pytest.raises(H.Failure, match="no HIP device"):
        hg.rows()
