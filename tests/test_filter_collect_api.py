"""CPU-side checks of option "filter_collect" (filtered k-NN from every node the walk evaluates: hnsw_search_collect_kernel in
ocaml-hnsw_amd/csrc/hnsw_device.hip.h, instantiated by csrc/hnsw_collect_variants.hip): the header states the definition, the
collect kernel's variant objects are listed once for the compiler and once for the build and all of them are built, the ABI is
what it was, and the option is refused on the host where no handle is given."""
import os
import re

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


def test_header_states_the_definition():
    hdr = _header()
    filtered = hdr[hdr.index("THE RESULT of hnsw_search_batch_filtered"):]
    filtered = filtered[:filtered.index("*/")]
    # the new paragraph stands after point 6 of the filtered-search definition, before the scratch note
    assert filtered.index("6. DETERMINISM") < filtered.index("WITH OPTION filter_collect") < filtered.index("Scratch (a stage's W")
    para = filtered[filtered.index("WITH OPTION filter_collect"):filtered.index("Scratch (a stage's W")]
    for needle in ("THE EVALUATED SET", "layer-0 entry node", "adj0(c)", "layer-0 loop expands", "does not depend on what the visited",
                   '"visited_blocks"', "Upper-layer evaluations are not collected", "hnsw_brute_force_batch", "pre-square-root",
                   "hnsw_distance_batch", "THE STAGE TEST", "|R_e(q)| >= k", "e_{j+1} = min(1024, 2 * e_j)", "unchanged exact stage",
                   "nothing is re-ranked", "(e_j, e_j)", "tied with max(W) at the k-th place", "DETERMINISM", "hnsw_search_batch_filtered_each",
                   "n_deleted > 0", "hnsw_sharded_set_option", "Range search is not affected", "k > 128", "two key registers",
                   "not saved"):
        assert needle in para, needle
    options = hdr[hdr.index("and one that CHANGES results"):hdr.index("int32_t hnsw_index_set_option(")]
    assert options.index('"sq8_rows"      ') < options.index('"filter_collect"') < options.index('"refine"        ')
    entry = options[options.index('"filter_collect"'):options.index('"refine"        ')]
    for needle in ("0 = off (default", "EVERY node the layer-0 walk evaluates", "HNSW_ERR_BAD_ARG", "k > 128", "EXCLUSIONS",
                   "float32, byte and split rows", '"half_rows" or "sq8_rows"', "the index unchanged", "Not saved",
                   "Range search is not affected", "RATE AND RECALL", "tools/filter_rate.py --collect", "profiles/filter_collect.txt"):
        assert needle in entry, needle


def _macro_triples(name):
    src = open(os.path.join(PKG, "csrc", "hnsw_internal.h")).read()
    body = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % name, src).group(1)
    return [tuple(int(v) for v in t) for t in re.findall(r"X\((\d+), (\d+), (\d+)\)", body)]


def test_collect_variant_list_matches_build_script_and_is_built(H):
    import __graft_entry__ as ge
    build = ge._load_build_module()
    listed = _macro_triples("HNSW_COLLECT_VARIANTS")
    # both metrics, both accept rules, the four exact-row formats (no half rows: 4)
    assert len(listed) == len(set(listed)) == 16, listed
    assert sorted(listed) == sorted(build.COLLECT_VARIANTS) == sorted((m, s, f) for m in (0, 1) for s in (0, 1) for f in (0, 1, 2, 3))
    # the knn kernel's own list is what it was
    assert sorted(_macro_triples("HNSW_SEARCH_VARIANTS")) == sorted(build.VARIANTS)
    assert len(build.VARIANTS) == 20
    assert build.COLLECT_SOURCE == "hnsw_collect_variants.hip" and build.COLLECT_SOURCE in build.DEPS
    assert os.path.exists(os.path.join(PKG, "csrc", build.COLLECT_SOURCE))
    # every listed object is built (the fixture ran the build) and linked: the library resolves, which it would not with a
    # launcher of the host's table missing
    for v in listed:
        assert os.path.exists(os.path.join(PKG, "build", "hnsw_collect_variants_%d_%d_%d.o" % v)), v
    # nothing else spells a triple out
    capi = open(os.path.join(PKG, "csrc", "hnsw_capi.hip")).read()
    assert not re.search(r"collect_launch_\d", capi)
    assert "HNSW_COLLECT_VARIANTS(HNSW_C_ENTRY)" in capi


def test_abi_is_unchanged(H):
    L = H.load()
    hdr = _header()
    assert re.search(r"#define\s+HNSW_ABI_VERSION\s+3\b", hdr)
    assert L.hnsw_abi_version() == H.ABI_VERSION == 3
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(hnsw_[a-z_0-9]+)\s*\(", bare)))
    assert declared == sorted(H.ABI_SYMBOLS)                    # no new entry point: the option goes through hnsw_index_set_option
    assert not [s for s in declared if "collect" in s]
    # SearchArgs, which every existing kernel takes, did not grow: the collect kernel's extras travel in a struct of their own
    dev = open(os.path.join(PKG, "csrc", "hnsw_device.hip.h")).read()
    args = dev[dev.index("struct SearchArgs {"):]
    args = args[:args.index("};")]
    assert "mask" not in args and "which" not in args
    assert re.search(r"hnsw_search_collect_kernel\(const IndexView iv, const SearchArgs a, const CollectArgs c\)", dev)


def test_null_handle_is_refused_on_the_host(H):
    L = H.load()
    assert L.hnsw_index_set_option(None, b"filter_collect", 1) == H.ERR_BAD_ARG
    assert L.hnsw_sharded_set_option(None, b"filter_collect", 1) == H.ERR_BAD_ARG


def test_front_ends_name_the_option():
    py = open(os.path.join(PKG, "__init__.py")).read()
    ml = open(os.path.join(PKG, "ocaml", "hnsw_mi355x.ml")).read()
    hpp = open(os.path.join(PKG, "host", "hnsw_front.hpp")).read()
    for txt in (py, ml, hpp):
        assert '"filter_collect"' in txt
