"""ocaml-hnsw_amd -- MI355X-native HNSW search behind ocaml-hnsw's own API surface.

Host-side mirror (Python, over the C ABI of include/hnsw_mi355x.h) of the reference modules whose
search bodies move to the GPU:

    Ohnsw.knn / Ohnsw.knn_batch_bigarray / Ohnsw.distance_l2      lib/ohnsw.ml:859-899
    Ba.knn / Ba.knn_batch (= Hnsw.Ba, MakeBatch(EuclideanBa))     lib/hnsw.ml:763-777, 817-819

Same names, argument meaning and error behaviour (Invalid_argument -> InvalidArgument,
Failure -> Failure).  The OCaml graph builder stays OCaml: this side takes the flattened graph
(`Hgraph`) that the OCaml shim produces.  There is no CPU path: every compute call goes to
libhnsw_mi355x.so and fails loudly if the library or a device is missing.
"""
import ctypes as _C
import os as _os

import numpy as _np

_PKG_DIR = _os.path.dirname(_os.path.abspath(__file__)) if "__file__" in globals() and \
    _os.path.basename(_os.path.dirname(_os.path.abspath(__file__))) == "ocaml-hnsw_amd" else \
    _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "ocaml-hnsw_amd")
LIB_PATH = _os.environ.get("HNSW_LIB_PATH") or _os.path.join(_PKG_DIR, "libhnsw_mi355x.so")

OK, ERR_BAD_ARG, ERR_EMPTY_INDEX, ERR_DEGREE_OVERFLOW = 0, -1, -2, -3
ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED = -4, -5, -6, -7
METRIC_L2, METRIC_IP = 0, 1
# 1 - <a,b> / (|a| |b|): the index stores N(X) and normalises every query batch itself (the twin contract of the C header); a
# Hgraph's host copy `vectors` stays the caller's matrix
METRIC_COSINE = 2
FILL_OHNSW, FILL_BA = 0, 1
SEM_OHNSW, SEM_FUNCTOR, SEM_FUNCTOR_NEAREST_K = 0, 1, 2
# IndexInfo.row_format: what the knn searches read (HNSW_ROWS_*); ROWS_HALF only after set_option("half_rows", 1), ROWS_SQ8 only
# after set_option("sq8_rows", 1), ROWS_SQ8_DIM only after set_option("sq8_dim_rows", 1)
ROWS_F32, ROWS_BYTES, ROWS_SPLIT, ROWS_HALF, ROWS_SQ8 = 0, 2, 3, 4, 5
ROWS_SQ8_DIM = 6
ROWS_BITS = 7            # only after set_option("bit_rows", 1 or 2)

ABI_VERSION = 3          # HNSW_ABI_VERSION of include/hnsw_mi355x.h this mirror was written against

# Every symbol include/hnsw_mi355x.h declares (tests check the .so exports all of them and compare the arities): name -> argument
# types, the result an int32 status unless spelled out as (argument types, result type).  load() applies the table.
_vp, _i32, _i64, _str, _f32 = _C.c_void_p, _C.c_int32, _C.c_int64, _C.c_char_p, _C.c_float
_ABI = {
    "hnsw_abi_version": (None, _i32),
    "hnsw_last_error": (None, _str),
    "hnsw_device_count": [_vp],
    "hnsw_index_create": [_vp, _i32, _vp],
    "hnsw_index_destroy": [_vp],
    "hnsw_index_get_info": [_vp, _vp],
    "hnsw_normalise_batch": [_i32, _vp, _i64, _i32, _i64, _vp, _i64, _vp],
    "hnsw_index_get_rows": [_vp, _vp, _i64, _vp, _i64],
    "hnsw_index_set_option": [_vp, _str, _i64],
    "hnsw_index_row_bytes": [_vp, _vp],
    "hnsw_index_sq8_params": [_vp, _vp, _vp],
    "hnsw_index_sq8_codes": [_vp, _vp],
    "hnsw_index_sq8_dim_params": [_vp, _vp, _vp],
    "hnsw_index_sq8_dim_codes": [_vp, _vp],
    "hnsw_index_bit_params": [_vp, _vp],
    "hnsw_index_bit_codes": [_vp, _vp],
    "hnsw_index_bit_query_codes": [_vp, _vp, _i64, _i64, _vp],
    "hnsw_search_batch": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "hnsw_search_batch_device": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_search_batch_h2d": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_knn": [_vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_distance_batch": [_vp, _vp, _i64, _i64, _vp, _i32, _vp],
    "hnsw_distance_batch_device": [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _vp],
    "hnsw_brute_force_batch": [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp],
    "hnsw_brute_force_batch_device": [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp],
    "hnsw_rerank_batch": [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _vp, _vp],
    "hnsw_rerank_batch_device": [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "hnsw_filter_create": [_vp, _vp, _i64, _vp],
    "hnsw_filter_destroy": [_vp],
    "hnsw_filter_count": [_vp, _vp],
    "hnsw_search_batch_filtered": [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_search_batch_filtered_each": [_vp, _vp, _i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_filter_create_by_label": [_vp, _vp, _i64, _i32, _vp],
    "hnsw_filter_bits": [_vp, _vp],
    "hnsw_range_search_batch": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_range_brute_force_batch": [_vp, _vp, _i64, _i64, _f32, _vp],
    "hnsw_range_search_batch_filtered": [_vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_range_brute_force_batch_filtered": [_vp, _vp, _vp, _i64, _i64, _f32, _vp],
    "hnsw_range_result_size": [_vp, _vp, _vp],
    "hnsw_range_result_fetch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_range_result_device": [_vp, _vp, _vp, _vp],
    "hnsw_range_result_destroy": [_vp],
    "hnsw_build": [_vp, _i64, _i32, _i64, _vp, _i32, _vp],
    "hnsw_index_insert": [_vp, _vp, _i64, _i64, _vp],
    "hnsw_index_remove": [_vp, _vp, _i64, _vp],
    "hnsw_index_mark_deleted": [_vp, _vp, _i64],
    "hnsw_index_unmark_deleted": [_vp, _vp, _i64],
    "hnsw_index_deleted_count": [_vp, _vp],
    "hnsw_index_deleted_bits": [_vp, _vp],
    "hnsw_index_compact": [_vp, _vp],
    "hnsw_select_neighbours_batch": [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "hnsw_index_layer_stats": [_vp, _i32, _vp],
    "hnsw_index_layer_isolated": [_vp, _i32, _vp, _i64, _vp],
    "hnsw_index_locality_codes": [_vp, _vp],
    "hnsw_index_visited_blocks": [_vp, _vp, _vp],
    "hnsw_index_prepare": [_vp, _vp],
    "hnsw_index_save": [_vp, _str],
    "hnsw_index_load": [_str, _i32, _vp],
    "hnsw_index_export_layer0": [_vp, _vp, _vp],
    "hnsw_index_export_upper_count": [_vp, _i32, _vp],
    "hnsw_index_export_upper": [_vp, _i32, _vp, _vp, _vp],
    "hnsw_search_layer_batch": [_vp, _i32, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_search_one_batch": [_vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp],
    "hnsw_index_kernel_times": [_vp, _vp, _vp, _vp],
    "hnsw_search_submit": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_search_wait": [_vp, _vp, _vp, _vp, _vp],
    "hnsw_multi_create": [_vp, _vp, _i32, _vp],
    "hnsw_multi_destroy": [_vp],
    "hnsw_multi_num_replicas": [_vp, _vp],
    "hnsw_multi_replica": [_vp, _i32, _vp],
    "hnsw_multi_search_batch": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "hnsw_multi_search_batch_device": [_vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "hnsw_multi_copy_result": [_vp, _i32, _vp, _vp],
    "hnsw_multi_debug_counters": [_vp, _vp],
    "hnsw_sharded_build": [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp],
    "hnsw_sharded_create": [_vp, _vp, _i32, _vp],
    "hnsw_sharded_load": [_vp, _vp, _i32, _vp],
    "hnsw_sharded_destroy": [_vp],
    "hnsw_sharded_num_shards": [_vp, _vp],
    "hnsw_sharded_shard": [_vp, _i32, _vp, _vp],
    "hnsw_sharded_get_info": [_vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_sharded_set_option": [_vp, _str, _i64],
    "hnsw_sharded_search_batch": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "hnsw_sharded_brute_force_batch": [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp],
    "hnsw_merge_lists": [_i32, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp],
    "hnsw_sharded_filter_create": [_vp, _vp, _i64, _vp],
    "hnsw_sharded_filter_destroy": [_vp],
    "hnsw_sharded_filter_count": [_vp, _vp],
    "hnsw_sharded_filter_part": [_vp, _i32, _vp],
    "hnsw_sharded_search_batch_filtered": [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_sharded_range_search_batch": [_vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_sharded_range_brute_force_batch": [_vp, _vp, _vp, _i64, _i64, _f32, _vp],
    "hnsw_sharded_range_result_size": [_vp, _vp, _vp],
    "hnsw_sharded_range_result_fetch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_sharded_range_result_device": [_vp, _vp, _vp, _vp],
    "hnsw_sharded_range_result_destroy": [_vp],
    "hnsw_merge_segments": [_i32, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _vp],
    "hnsw_host_register": [_vp, _i64],
    "hnsw_host_unregister": [_vp],
    "hnsw_host_alloc": [_vp, _i64],
    "hnsw_host_free": [_vp],
    "hnsw_labels_create": [_vp, _vp, _i64, _i32, _vp],
    "hnsw_labels_destroy": [_vp],
    "hnsw_labels_info": [_vp, _vp, _vp, _vp],
    "hnsw_labels_get": [_vp, _vp],
    "hnsw_search_batch_grouped": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_brute_force_batch_grouped": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp],
    "hnsw_index_set_keys": [_vp, _vp, _i64],
    "hnsw_index_clear_keys": [_vp],
    "hnsw_index_keys_info": [_vp, _vp, _vp],
    "hnsw_index_keys_of": [_vp, _vp, _i64, _i64, _vp],
    "hnsw_index_keys_of_device": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_index_find_keys": [_vp, _vp, _i64, _vp],
    "hnsw_search_batch_keyed": [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hnsw_index_insert_keyed": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_index_remove_keys": [_vp, _vp, _i64, _vp],
    "hnsw_index_mark_deleted_keys": [_vp, _vp, _i64],
    "hnsw_index_unmark_deleted_keys": [_vp, _vp, _i64],
    "hnsw_filter_create_by_keys": [_vp, _vp, _i64, _vp],
    "hnsw_index_get_rows_device": [_vp, _vp, _i64, _vp, _i64, _vp],
    "hnsw_search_batch_by_id": [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp],
    "hnsw_search_batch_by_key": [_vp, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _vp, _vp],
    "hnsw_brute_force_batch_by_id": [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "hnsw_knn_graph": [_vp, _vp, _i32, _vp, _vp],
    "hnsw_index_upsert_keyed": [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "hnsw_index_update": [_vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hnsw_search_batch_after": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_brute_force_batch_after": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp],
    "hnsw_diversify_batch": [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp],
    "hnsw_diversify_batch_device": [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp],
    "hnsw_search_batch_diverse": [_vp, _vp, _vp, _i64, _i64, _vp, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    "hnsw_brute_force_batch_diverse": [_vp, _vp, _i64, _i64, _i32, _i32, _f32, _i32, _vp, _vp, _vp],
}
ABI_SYMBOLS = list(_ABI)


class InvalidArgument(ValueError):
    """OCaml Invalid_argument (e.g. "knn: empty hgraph", lib/ohnsw.ml:862)."""


class Failure(RuntimeError):
    """OCaml Failure: device / runtime errors."""


class _LayerDesc(_C.Structure):
    _fields_ = [("n_nodes", _C.c_int64), ("nodes", _C.c_void_p), ("deg", _C.c_void_p),
                ("nbr", _C.c_void_p)]


class _IndexDesc(_C.Structure):
    _fields_ = [("vectors", _C.c_void_p), ("n", _C.c_int64), ("d", _C.c_int32),
                ("row_stride", _C.c_int64), ("metric", _C.c_int32), ("id_base", _C.c_int32),
                ("max_degree0", _C.c_int32), ("max_degree", _C.c_int32), ("max_layer", _C.c_int32),
                ("entry_point", _C.c_int64), ("deg0", _C.c_void_p), ("nbr0", _C.c_void_p),
                ("upper", _C.c_void_p), ("expected_ef", _C.c_int32), ("expected_semantics", _C.c_int32)]


class _SearchParams(_C.Structure):
    _fields_ = [("ef", _C.c_int32), ("k", _C.c_int32), ("fill", _C.c_int32), ("semantics", _C.c_int32)]


class _RangeParams(_C.Structure):
    _fields_ = [("radius", _C.c_float), ("ef", _C.c_int32), ("semantics", _C.c_int32)]


class _BuildParams(_C.Structure):
    _fields_ = [("num_connections", _C.c_int32), ("num_nodes_search_construction", _C.c_int32),
                ("metric", _C.c_int32), ("id_base", _C.c_int32), ("seed", _C.c_uint64),
                ("max_batch", _C.c_int32), ("batch_div", _C.c_int32), ("expected_ef", _C.c_int32), ("expected_semantics", _C.c_int32)]


class LayerStats(_C.Structure):
    _fields_ = [("num_nodes", _C.c_int64), ("min_degree", _C.c_int32), ("max_degree", _C.c_int32),
                ("mean_degree", _C.c_double), ("num_isolated", _C.c_int64)]


class IndexInfo(_C.Structure):
    _fields_ = [("n", _C.c_int64), ("d", _C.c_int32), ("metric", _C.c_int32), ("id_base", _C.c_int32),
                ("max_degree0", _C.c_int32), ("max_degree", _C.c_int32), ("max_layer", _C.c_int32),
                ("entry_point", _C.c_int64), ("device_bytes", _C.c_int64),
                ("row_stride_bytes", _C.c_int64), ("device", _C.c_int32), ("row_format", _C.c_int32)]


_lib = None


def load():
    """dlopen the in-tree libhnsw_mi355x.so (built by build.py / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _os.path.exists(LIB_PATH):
        raise Failure("%s is missing: run `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                      "there is no CPU fallback" % LIB_PATH)
    L = _C.CDLL(LIB_PATH)
    L.hnsw_abi_version.restype = _i32
    if L.hnsw_abi_version() != ABI_VERSION:
        raise Failure("%s speaks ABI version %d, this binding %d: rebuild it (python __graft_entry__.py)" % (LIB_PATH, L.hnsw_abi_version(), ABI_VERSION))
    for name, sig in _ABI.items():
        f = getattr(L, name)
        f.argtypes, f.restype = sig if isinstance(sig, tuple) else (sig, _i32)
    _lib = L
    return L


def _check(rc):
    if rc == OK:
        return
    msg = load().hnsw_last_error().decode()
    if rc in (ERR_BAD_ARG, ERR_EMPTY_INDEX, ERR_DEGREE_OVERFLOW):
        raise InvalidArgument(msg)
    raise Failure("[%d] %s" % (rc, msg))


def device_count():
    c = _C.c_int32(0)
    rc = load().hnsw_device_count(_C.byref(c))
    return c.value if rc == OK else 0


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_C.c_void_p)


def _rows(a):
    """[n][d] fp32 whose rows are contiguous but may be spaced (a Lacaml sub-matrix keeps its parent's
    leading dimension): returned as (array, row stride in floats) without copying when possible."""
    a = _np.asarray(a)
    if (a.dtype == _np.float32 and a.ndim == 2 and a.shape[0] > 0 and a.strides[1] == 4
            and a.strides[0] % 4 == 0 and a.strides[0] >= 4 * a.shape[1]):
        return a, a.strides[0] // 4
    a = _np.ascontiguousarray(a, dtype=_np.float32)
    return a, (a.shape[1] if a.ndim == 2 else 0)


def _batch(hgraph_d, batch, min_rows=0):
    """A query batch for an index of hgraph_d dimensions -> (Q, q_stride, nq) as the library takes them (see _rows)."""
    Q, qs = _rows(batch)
    if Q.ndim != 2 or Q.shape[0] < min_rows or (Q.shape[0] and Q.shape[1] != hgraph_d):
        raise InvalidArgument("batch must be [nq][d], nq >= 1" if min_rows else "batch must be [nq][d]")
    return Q, max(qs, hgraph_d), Q.shape[0]


def normalise(X, device=0, norms=False):
    """hnsw_normalise_batch: N(X), the rows a METRIC_COSINE index stores for X and searches for a query batch X, as a fresh
    [n][d] float32 matrix (norms=True: and the norms [n]).  A zero row stays zero (norm 0); a row whose sum of squares is not
    finite becomes NaN.  What a caller uses to pre-normalise data for other tools, or to build the IP twin of a COSINE index."""
    A, stride = _rows(X)
    if A.ndim != 2:
        raise InvalidArgument("X must be [n][d]")
    n, d = A.shape
    out = _np.empty((n, d), _np.float32)
    nrm = _np.empty(n, _np.float32) if norms else None
    _check(load().hnsw_normalise_batch(device, _ptr(A), n, d, max(stride, d), _ptr(out), d, _ptr(nrm)))
    return (out, nrm) if norms else out


def _keys(keys):
    """a vector of keys as the library reads it: contiguous int64 (every int64 value is a legal key)"""
    a = _np.asarray(keys)
    if a.size and a.dtype.kind not in "iu":
        raise InvalidArgument("keys must be integers")
    if a.dtype == _np.uint64 and a.size and int(a.max()) >= 2 ** 63:
        raise InvalidArgument("keys must fit a signed 64-bit integer")
    return _np.ascontiguousarray(a, dtype=_np.int64).reshape(-1)


MISSING_KEY = -1         # the default `missing` of the keyed calls: what a row holds where the search wrote its fill id


def _out_pair(nq, k, out):
    """The result matrices (ids, dist) of nq queries: fresh ones, or out = the caller's pair (e.g. pinned matrices it reuses
    batch after batch), which the library fills as nq * k contiguous words each."""
    if out is None:
        return _np.empty((nq, max(k, 0)), _np.int32), _np.empty((nq, max(k, 0)), _np.float32)
    ids, dist = out
    if ids.shape != (nq, k) or dist.shape != (nq, k) or ids.dtype != _np.int32 or dist.dtype != _np.float32 \
            or not ids.flags["C_CONTIGUOUS"] or not dist.flags["C_CONTIGUOUS"]:
        raise InvalidArgument("out must be (int32 [nq][k], float32 [nq][k]), C-contiguous")
    return ids, dist


class Hgraph:
    """The flattened form of Ohnsw.Hgraph.t (lib/ohnsw.ml:307-312) / Hnsw.Ba.Hgraph.t
    (lib/hnsw.ml:342-348) that crosses the C ABI: vectors + per-layer neighbour rows in the
    reference's iteration order, ids `id_base`-based (0 for Ohnsw, 1 for Hnsw.Ba).

    vectors [n][d] fp32; deg0 [n]; nbr0 [n][max_degree0]; upper = list of (nodes, deg, nbr) for
    layers 1..max_layer; entry_point id_base-based or None (empty hgraph)."""

    def __init__(self, vectors, deg0, nbr0, upper=(), entry_point=None, id_base=0,
                 max_degree=None, metric=METRIC_L2, expected_ef=0, expected_sem=SEM_OHNSW):
        self.vectors, self.row_stride = _rows(vectors)
        if self.vectors.ndim != 2:
            raise InvalidArgument("vectors must be [n][d]")
        self.n, self.d = self.vectors.shape
        self.deg0 = _np.ascontiguousarray(deg0, dtype=_np.int32)
        self.nbr0 = _np.ascontiguousarray(nbr0, dtype=_np.int32)
        if self.nbr0.ndim != 2 or self.nbr0.shape[0] != self.n or self.deg0.shape != (self.n,):
            raise InvalidArgument("deg0 / nbr0 shapes do not match n")
        self.max_degree0 = int(self.nbr0.shape[1])
        self.upper = []
        for (nodes, deg, nbr) in upper:
            nodes = _np.ascontiguousarray(nodes, dtype=_np.int64)
            deg = _np.ascontiguousarray(deg, dtype=_np.int32)
            nbr = _np.ascontiguousarray(nbr, dtype=_np.int32).reshape(len(nodes), -1)
            self.upper.append((nodes, deg, nbr))
        self.max_layer = len(self.upper)
        self.max_degree = int(max_degree if max_degree is not None else
                              (self.upper[0][2].shape[1] if self.upper else max(1, self.max_degree0 // 2)))
        self.id_base = int(id_base)
        self.entry_point = None if entry_point is None or entry_point < id_base else int(entry_point)
        self.metric = int(metric)
        # hnsw_index_desc.expected_ef / expected_semantics: the upload then also prepares searches with these parameters
        self.expected_ef, self.expected_sem = int(expected_ef), int(expected_sem)
        self._index = None
        self._device = None

    # The host copy of the vectors.  Ohnsw.insert_batch appends the new rows as parts of their own: one call costs its own
    # rows, not a copy of all n; the parts are joined into one [n][d] array when the vectors are next read.
    @property
    def vectors(self):
        parts = self.__dict__.get("_vparts")
        if parts is None:
            return None
        if len(parts) > 1:
            parts[:] = [_np.concatenate(parts)]
        return parts[0]

    @vectors.setter
    def vectors(self, value):
        self._vparts = None if value is None else [value]
        self.row_stride = 0 if value is None else value.strides[0] // 4      # (floats; __init__ and _append_vectors know better)

    def _append_vectors(self, rows):
        parts = self.__dict__.get("_vparts")
        if parts is None:
            return
        if len(parts) == 1:
            parts[0] = _np.ascontiguousarray(parts[0], dtype=_np.float32)     # (no copy for a contiguous float32 array)
        parts.append(_np.array(rows, dtype=_np.float32))
        self.row_stride = self.d

    @classmethod
    def _from_handle(cls, handle, device, vectors=None):
        """Wrap an index that already lives on the device (hnsw_build, hnsw_index_load), leaving every field __init__ sets; the
        host copy of the graph is fetched on demand by export()."""
        self = cls.__new__(cls)
        self.vectors = vectors
        self._index, self._device = handle, device
        self.expected_ef, self.expected_sem = 0, SEM_OHNSW
        inf = self.info()
        self.d, self.id_base, self.metric = int(inf.d), int(inf.id_base), int(inf.metric)
        self._adopt(inf)
        return self

    def _adopt(self, info):
        """Follow the device index: n, widths, max_layer and entry_point from its hnsw_index_info; the host copy of the graph,
        if there was one, is stale (export() fetches it)."""
        self.n = int(info.n)
        self.max_degree0, self.max_degree, self.max_layer = info.max_degree0, info.max_degree, info.max_layer
        self.entry_point = int(info.entry_point) if info.entry_point >= self.id_base else None
        self.deg0 = self.nbr0 = self.upper = None

    def export(self):
        """Fetch the flattened graph from the device: fills deg0, nbr0, upper (ids id_base-based)."""
        L = load()
        self.deg0 = _np.empty(self.n, _np.int32)
        self.nbr0 = _np.empty((self.n, self.max_degree0), _np.int32)
        _check(L.hnsw_index_export_layer0(self.handle, _ptr(self.deg0), _ptr(self.nbr0)))
        self.upper = []
        for l in range(1, self.max_layer + 1):
            c = _C.c_int64(0)
            _check(L.hnsw_index_export_upper_count(self.handle, l, _C.byref(c)))
            nodes = _np.empty(c.value, _np.int64)
            deg = _np.empty(c.value, _np.int32)
            nbr = _np.empty((c.value, self.max_degree), _np.int32)
            _check(L.hnsw_index_export_upper(self.handle, l, _ptr(nodes), _ptr(deg), _ptr(nbr)))
            self.upper.append((nodes, deg, nbr))
        return self

    def rows(self, ids=None):
        """hnsw_index_get_rows: the float32 rows the device index holds for the nodes `ids` (id_base-based; None: all n, in order)
        as a fresh [m][d] matrix -- for METRIC_COSINE N(X), not the caller's matrix that `vectors` keeps"""
        if ids is None:
            m, p = self.info().n, None
        else:
            ids = _np.ascontiguousarray(ids, dtype=_np.int64).reshape(-1)
            m, p = ids.size, _ptr(ids)
        out = _np.empty((m, self.d), _np.float32)
        if m:
            _check(load().hnsw_index_get_rows(self.handle, p, m, _ptr(out), self.d))
        return out

    def knn_graph(self, k, ef=None, exact=False, sem=SEM_OHNSW, fill=FILL_OHNSW, distances=True):
        """hnsw_knn_graph: the k-NN graph of the whole index -> (ids [n][k], distances [n][k]), distances=False: ids alone.  Row v is
        the row of Ohnsw.knn_batch_by_id for node id_base + v without the node itself (exact=True: of Ohnsw.brute_force_by_id),
        computed on the device in chunks of option "graph_chunk_rows" nodes; ef None: ef == k."""
        n = self.info().n
        ids = _np.empty((n, max(int(k), 0)), _np.int32)
        dist = _np.empty((n, max(int(k), 0)), _np.float32) if distances else None
        p = _SearchParams(int(k) if ef is None else int(ef), int(k), fill, sem)
        _check(load().hnsw_knn_graph(self.handle, _C.byref(p), 1 if exact else 0, _ptr(ids), _ptr(dist)))
        return (ids, dist) if distances else ids

    def locality_codes(self):
        """hnsw_index_locality_codes: the permutation of 0 .. n-1 that keys the visited set's bitmap blocks (introspection)."""
        out = _np.empty(self.n, _np.int32)
        _check(load().hnsw_index_locality_codes(self.handle, _ptr(out)))
        return out

    def visited_blocks(self, ef, sem=0):
        """hnsw_index_visited_blocks: 0 = searches at this ef use the tag cache, else log2 of the bitmap-block slots"""
        p = _SearchParams(ef, 1, FILL_OHNSW, sem)
        out = _C.c_int32(0)
        _check(load().hnsw_index_visited_blocks(self.handle, _C.byref(p), _C.byref(out)))
        return out.value

    def prepare(self, ef, sem=SEM_OHNSW):
        """hnsw_index_prepare: everything the first search with this ef and accept rule would do once (the visited-structure
        decision, the kernel's residency, its code object), now"""
        p = _SearchParams(ef, 1, FILL_OHNSW, sem)
        _check(load().hnsw_index_prepare(self.handle, _C.byref(p)))
        return self

    def stats(self):
        """Hgraph.Stats.compute (lib/hnsw.ml:353-375): {num_nodes, layer_sizes, layer_connectivity}; a layer's
        connectivity is the reference's mima record {min, max, mean, isolated}, `isolated` the list of node ids
        (descending, as the reference's fold conses it)."""
        out = {"num_nodes": self.n, "layer_sizes": {}, "layer_connectivity": {}}
        for l in range(self.max_layer + 1):
            st = LayerStats()
            _check(load().hnsw_index_layer_stats(self.handle, l, _C.byref(st)))
            iso = _np.empty(max(int(st.num_isolated), 1), _np.int64)
            c = _C.c_int64(0)
            _check(load().hnsw_index_layer_isolated(self.handle, l, _ptr(iso), int(st.num_isolated), _C.byref(c)))
            out["layer_sizes"][l] = int(st.num_nodes)
            out["layer_connectivity"][l] = {"min": st.min_degree, "max": st.max_degree,
                                            "mean": st.mean_degree, "isolated": iso[:min(c.value, int(st.num_isolated))].tolist()}
        return out

    def save(self, path):
        """Write the flattened index (vectors + graph) to `path` (hnsw_index_save)."""
        _check(load().hnsw_index_save(self.handle, str(path).encode()))

    @classmethod
    def load(cls, path, device=0):
        """Read a flattened index file straight into HBM (hnsw_index_load)."""
        h = _C.c_void_p()
        _check(load().hnsw_index_load(str(path).encode(), device, _C.byref(h)))
        return cls._from_handle(h, device)

    @classmethod
    def flat(cls, vectors, metric=METRIC_L2, id_base=0):
        """An edgeless graph over the vectors (zero degrees, row width 1, entry point the first node): for callers who only
        want the exact scan (Ohnsw.brute_force_knn)."""
        X, _ = _rows(vectors)
        if X.ndim != 2:
            raise InvalidArgument("vectors must be [n][d]")
        n = X.shape[0]
        return cls(vectors, _np.zeros(n, _np.int32), _np.full((n, 1), -1, _np.int32), entry_point=id_base if n else None,
                   id_base=id_base, max_degree=1, metric=metric)

    def _desc(self):
        """(hnsw_index_desc, keep-alive) of the host copy of the flattened graph."""
        if self.vectors is None or self.deg0 is None:
            raise InvalidArgument("no host copy of the graph: call export() (and keep the vectors) first")
        nl = self.max_layer
        layers = (_LayerDesc * max(nl, 1))()
        for i, (nodes, deg, nbr) in enumerate(self.upper):
            if nbr.shape[1] != self.max_degree and len(nodes):
                raise InvalidArgument("upper rows must be max_degree wide")
            layers[i].n_nodes = len(nodes)
            layers[i].nodes, layers[i].deg, layers[i].nbr = nodes.ctypes.data, deg.ctypes.data, nbr.ctypes.data
        d = _IndexDesc()
        d.vectors = self.vectors.ctypes.data
        d.n, d.d, d.row_stride = self.n, self.d, self.row_stride
        d.metric, d.id_base = self.metric, self.id_base
        d.max_degree0, d.max_degree, d.max_layer = self.max_degree0, self.max_degree, nl
        d.entry_point = self.id_base - 1 if self.entry_point is None else self.entry_point
        d.deg0, d.nbr0 = self.deg0.ctypes.data, self.nbr0.ctypes.data
        d.upper = _C.cast(layers, _C.c_void_p)
        d.expected_ef, d.expected_semantics = self.expected_ef, self.expected_sem
        return d, layers

    def to_device(self, device=0):
        """Upload to HBM (hnsw_index_create).  Idempotent per device."""
        if self._index is not None and self._device == device:
            return self
        self.release()
        d, _keep = self._desc()
        h = _C.c_void_p()
        _check(load().hnsw_index_create(_C.byref(d), device, _C.byref(h)))
        self._index, self._device = h, device
        return self

    @property
    def handle(self):
        if self._index is None:
            self.to_device(0)
        return self._index

    def info(self):
        inf = IndexInfo()
        _check(load().hnsw_index_get_info(self.handle, _C.byref(inf)))
        return inf

    def set_option(self, name, value):
        """hnsw_index_set_option: every option of the C header by its name ("byte_rows", "half_rows", "sq8_rows", "sq8_dim_rows", "bit_rows", "bit_query_bits", "refine", ...).
        "filter_collect" 1 makes the filtered searches (knn_batch_filtered, knn_batch_filtered_each, the plain searches under
        marks) answer from every node the layer-0 walk evaluates, not from the final W only (k <= 128, exact rows; default 0)"""
        _check(load().hnsw_index_set_option(self.handle, name.encode(), int(value)))

    def row_bytes(self):
        """Bytes of one vector as the knn searches read it (d: byte and sq8 rows of either kind, 2 d: half rows, 4 d: float32 rows)."""
        v = _C.c_int64(0)
        _check(load().hnsw_index_row_bytes(self.handle, _C.byref(v)))
        return v.value

    def sq8_params(self):
        """hnsw_index_sq8_params -> (lo, scale) as float32 of the sq8 copy (set_option("sq8_rows", 1)): x ~ lo + scale * code"""
        lo, s = _C.c_float(0), _C.c_float(0)
        _check(load().hnsw_index_sq8_params(self.handle, _C.byref(lo), _C.byref(s)))
        return _np.float32(lo.value), _np.float32(s.value)

    def sq8_codes(self):
        """hnsw_index_sq8_codes -> the codes of the sq8 copy, uint8 [n][d] (the rows' padding is not exported)"""
        out = _np.empty((self.info().n, self.d), _np.uint8)
        _check(load().hnsw_index_sq8_codes(self.handle, _ptr(out)))
        return out

    def sq8_dim_params(self):
        """hnsw_index_sq8_dim_params -> (lo, scale), two float32 arrays of length d, of the per-dimension sq8 copy
        (set_option("sq8_dim_rows", 1)): x[i] ~ lo[i] + scale[i] * code[i]"""
        lo, s = _np.empty(self.d, _np.float32), _np.empty(self.d, _np.float32)
        _check(load().hnsw_index_sq8_dim_params(self.handle, _ptr(lo), _ptr(s)))
        return lo, s

    def sq8_dim_codes(self):
        """hnsw_index_sq8_dim_codes -> the codes of the per-dimension sq8 copy, uint8 [n][d] (the rows' padding is not exported)"""
        out = _np.empty((self.info().n, self.d), _np.uint8)
        _check(load().hnsw_index_sq8_dim_codes(self.handle, _ptr(out)))
        return out

    def bit_params(self):
        """hnsw_index_bit_params -> t, float32 [d]: the thresholds of the 1-bit copy (set_option("bit_rows", 1): the column means,
        2: zeros); bit i of a row is x[i] > t[i]"""
        t = _np.empty(self.d, _np.float32)
        _check(load().hnsw_index_bit_params(self.handle, _ptr(t)))
        return t

    def bit_codes(self):
        """hnsw_index_bit_codes -> the codes of the 1-bit copy, uint32 [n][ceil(d / 32)]: dimension i is bit i % 32 of word i // 32
        (numpy.packbits(X > t, axis=1, bitorder="little") viewed as uint32; the rows' padding words are not exported)"""
        out = _np.empty((self.info().n, (self.d + 31) // 32), _np.uint32)
        _check(load().hnsw_index_bit_codes(self.handle, _ptr(out)))
        return out

    def bit_query_codes(self, Q):
        """hnsw_index_bit_query_codes -> int8 [nq][d]: the 4-bit codes in -7..7 that the walk over the bit rows uses for the queries Q
        under set_option("bit_query_bits", 4) (the rule: the C header; a COSINE index normalises Q first).  Needs "bit_rows" on, not
        "bit_query_bits"""
        Q = _np.ascontiguousarray(_np.atleast_2d(_np.asarray(Q, _np.float32)))
        if Q.shape[1] != self.d:
            raise InvalidArgument("bit_query_codes: queries of %d dimensions, the index has %d" % (Q.shape[1], self.d))
        out = _np.empty((Q.shape[0], self.d), _np.int8)
        _check(load().hnsw_index_bit_query_codes(self.handle, _ptr(Q), Q.shape[0], Q.shape[1], _ptr(out)))
        return out

    def filter(self, allow):
        """hnsw_filter_create -> Filter: an allow-mask over this index's nodes.  allow: a boolean array of length n (entry v = node
        v + id_base may be returned), or an array of node ids (id_base-based).  Valid until the index grows or shrinks (insert_batch,
        remove_batch)."""
        return Filter(self, allow)

    def filters_by_label(self, labels, n_labels=None):
        """hnsw_filter_create_by_label -> [Filter] * n_labels: filter l allows node v (0-based position in `labels`, one integer per
        node) iff labels[v] == l; a label of -1 puts the node in no filter.  n_labels defaults to max label + 1.  One upload of the
        labels and one pass over them on the device, not n_labels host-built masks."""
        lab = _np.asarray(labels)
        if lab.dtype.kind not in "iu" or lab.ndim != 1:
            raise InvalidArgument("labels must be a vector of integers, one per node")
        if lab.size and (lab.min() < -(2 ** 31) or lab.max() >= 2 ** 31):
            raise InvalidArgument("labels must fit 32 bits")
        lab = _np.ascontiguousarray(lab, _np.int32)
        if n_labels is None:
            n_labels = int(lab.max()) + 1 if lab.size else 0
        if n_labels < 1:
            raise InvalidArgument("n_labels must be >= 1")
        out = (_C.c_void_p * n_labels)()
        _check(load().hnsw_filter_create_by_label(self.handle, _ptr(lab) if lab.size else None, lab.size, n_labels, out))
        return [Filter._adopt(self, _C.c_void_p(out[l]), lab.size) for l in range(n_labels)]

    def labels(self, labels, n_labels=None):
        """hnsw_labels_create -> Labels: one label per node (0-based position in `labels`; -1: the node is in no group), uploaded once:
        the groups of Ohnsw.knn_batch_grouped.  n_labels defaults to max label + 1.  Valid until the index changes (insert_batch,
        remove_batch, mark_deleted, unmark_deleted)."""
        return Labels(self, labels, n_labels)

    def mark_deleted(self, ids):
        """hnsw_index_mark_deleted: soft deletion.  The stored nodes `ids` (id_base-based, distinct) stay in the graph -- every walk
        still goes through them -- but no search returns them any more: while any node is marked, the knn, brute-force and range
        searches answer under the mask of the live nodes, and new filters are ANDed with it.  Filters made before are refused
        afterwards.  Cheap (a few bits on the device); compact() pays for the repair later."""
        ids = _np.ascontiguousarray(ids, dtype=_np.int64).reshape(-1)
        _check(load().hnsw_index_mark_deleted(self.handle, _ptr(ids) if len(ids) else None, len(ids)))

    def unmark_deleted(self, ids):
        """hnsw_index_unmark_deleted: the nodes `ids` are live again (a node that is not marked stays as it is)"""
        ids = _np.ascontiguousarray(ids, dtype=_np.int64).reshape(-1)
        _check(load().hnsw_index_unmark_deleted(self.handle, _ptr(ids) if len(ids) else None, len(ids)))

    def deleted_count(self):
        """hnsw_index_deleted_count: how many nodes are marked"""
        c = _C.c_int64(0)
        _check(load().hnsw_index_deleted_count(self.handle, _C.byref(c)))
        return c.value

    def deleted_mask(self):
        """hnsw_index_deleted_bits -> a boolean array of length n: entry v = node v + id_base is marked"""
        n = self.info().n
        words = _np.zeros(max((n + 31) // 32, 1), _np.uint32)
        _check(load().hnsw_index_deleted_bits(self.handle, _ptr(words)))
        return _np.unpackbits(words.view(_np.uint8), bitorder="little")[:n].astype(bool)

    def compact(self):
        """hnsw_index_compact: hnsw_index_remove of the marked nodes (see Ohnsw.remove_batch) -> the new id of every old node
        (np.int32 [n_old], id_base - 1 for a removed one).  Afterwards nothing is marked."""
        n_old = self.info().n
        gone = self.deleted_count()
        new_id = _np.empty(n_old, _np.int32)
        _check(load().hnsw_index_compact(self.handle, _ptr(new_id)))
        if gone:
            X = self.vectors
            if X is not None:
                self.vectors = _np.ascontiguousarray(_np.asarray(X, dtype=_np.float32)[new_id >= self.id_base])
                self.row_stride = self.d
            self._adopt(self.info())
        return new_id

    def _shrunk(self, new_id):
        """after a removal: the host vectors (if any) lose the removed rows, n and the widths follow the device index"""
        X = self.vectors
        if X is not None:
            self.vectors = _np.ascontiguousarray(_np.asarray(X, dtype=_np.float32)[new_id >= self.id_base])
            self.row_stride = self.d
        self._adopt(self.info())

    # ---- keys the index owns (hnsw_index_set_keys ...): stable int64 names that survive remove_batch and compact ----
    def set_keys(self, keys):
        """hnsw_index_set_keys: one caller-chosen int64 key per stored node, in row order, pairwise distinct (a duplicate is refused
        naming the smallest duplicated key; the handle then keeps the keys it had).  The index keeps them on the device and moves
        them with their nodes through insert_batch_keyed, remove_batch and compact.  Filters and labels stay valid."""
        k = _keys(keys)
        _check(load().hnsw_index_set_keys(self.handle, _ptr(k) if k.size else None, k.size))

    def clear_keys(self):
        """hnsw_index_clear_keys: afterwards the index is one that never had keys"""
        _check(load().hnsw_index_clear_keys(self.handle))

    def keys_info(self):
        """hnsw_index_keys_info -> (has_keys, bytes on the device: not part of info().device_bytes)"""
        has, b = _C.c_int32(0), _C.c_int64(0)
        _check(load().hnsw_index_keys_info(self.handle, _C.byref(has), _C.byref(b)))
        return bool(has.value), b.value

    def keys(self, ids=None, missing=MISSING_KEY):
        """hnsw_index_keys_of: the keys of the nodes `ids` (id_base-based, any shape; None: all n in row order) as int64 of that
        shape; `missing` where an id names no node -- the searches' fill id -1 included.  What turns the ids of ANY search form
        (range, grouped, per-query filters, layer operators) into keys."""
        if ids is None:
            n = self.info().n
            out = _np.empty(n, _np.int64)
            _check(load().hnsw_index_keys_of(self.handle, None, n, int(missing), _ptr(out) if n else None))
            return out
        a = _np.asarray(ids)
        if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
            a = _np.where((a < -(2 ** 31)) | (a >= 2 ** 31), self.id_base - 1, a)        # (no node either way)
        a = _np.ascontiguousarray(a, dtype=_np.int32)
        out = _np.empty(a.shape, _np.int64)
        if a.size:
            _check(load().hnsw_index_keys_of(self.handle, _ptr(a), a.size, int(missing), _ptr(out)))
        return out

    def find_keys(self, keys):
        """hnsw_index_find_keys -> int64 ids (id_base-based) of the nodes with these keys, id_base - 1 where no node has the key"""
        k = _keys(keys)
        out = _np.empty(k.size, _np.int64)
        _check(load().hnsw_index_find_keys(self.handle, _ptr(k) if k.size else None, k.size, _ptr(out) if k.size else None))
        return out

    def remove_keys(self, keys):
        """hnsw_index_remove_keys: Ohnsw.remove_batch of the nodes with these keys (an absent key is refused, nothing changed)
        -> the new id of every old node, as remove_batch"""
        k = _keys(keys)
        new_id = _np.empty(self.n, _np.int32)
        _check(load().hnsw_index_remove_keys(self.handle, _ptr(k) if k.size else None, k.size, _ptr(new_id)))
        if k.size:
            self._shrunk(new_id)
        return new_id

    def upsert(self, batch, keys, num_connections, num_nodes_search_construction, **build_args):
        """Ohnsw.upsert_batch_keyed(self, ...): replace the vectors under the stored keys, add the others, in one all-or-nothing
        call -> (replaced bool[m], new_id int32[n_old])"""
        return Ohnsw.upsert_batch_keyed(self, batch, keys, num_connections, num_nodes_search_construction, **build_args)

    def mark_deleted_keys(self, keys):
        """hnsw_index_mark_deleted_keys: mark_deleted of the nodes with these keys (an absent key is refused, nothing changed)"""
        k = _keys(keys)
        _check(load().hnsw_index_mark_deleted_keys(self.handle, _ptr(k) if k.size else None, k.size))

    def unmark_deleted_keys(self, keys):
        """hnsw_index_unmark_deleted_keys: unmark_deleted of the nodes with these keys"""
        k = _keys(keys)
        _check(load().hnsw_index_unmark_deleted_keys(self.handle, _ptr(k) if k.size else None, k.size))

    def filter_by_keys(self, keys):
        """hnsw_filter_create_by_keys -> Filter: allows exactly the nodes with these keys (repeats are fine, an absent key is
        refused), ANDed with the live mask as Hgraph.filter's is"""
        k = _keys(keys)
        f = _C.c_void_p()
        _check(load().hnsw_filter_create_by_keys(self.handle, _ptr(k) if k.size else None, k.size, _C.byref(f)))
        return Filter._adopt(self, f, self.info().n)

    def kernel_times(self):
        """(search kernel ms, ordering pre-pass ms, calls) averaged over the device-entry calls since the
        last call (needs set_option("time_kernels", 1)); waits for them."""
        s_, p_, n_ = _C.c_double(0), _C.c_double(0), _C.c_int32(0)
        _check(load().hnsw_index_kernel_times(self.handle, _C.byref(s_), _C.byref(p_), _C.byref(n_)))
        return s_.value, p_.value, n_.value

    def release(self):
        if self._index is not None:
            if self.__dict__.get("_owner") is None:      # (a shard borrowed from a ShardedHgraph is destroyed with it)
                load().hnsw_index_destroy(self._index)
            self._index = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class _HostBlock:
    """page-locked memory from hnsw_host_alloc, exposed through the array interface; freed with its last numpy view"""

    def __init__(self, shape, dtype):
        dt = _np.dtype(dtype)
        self.shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.nbytes = max(1, int(_np.prod(self.shape, dtype=_np.int64)) * dt.itemsize)
        p = _C.c_void_p()
        _check(load().hnsw_host_alloc(_C.byref(p), self.nbytes))
        self.ptr = p.value
        self.__array_interface__ = {"data": (self.ptr, False), "shape": self.shape, "typestr": dt.str, "version": 3}

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                load().hnsw_host_free(_C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def host_empty(shape, dtype=_np.float32):
    """A numpy array in page-locked memory the library allocates (hnsw_host_alloc): the host-buffer entry points read such
    query matrices and write such result matrices directly from the device, without copies.  Freed with the array."""
    return _np.asarray(_HostBlock(shape, dtype))


def pin(array):
    """hnsw_host_register: page-lock a host array the caller keeps alive (its query or result matrix of a benchmark
    loop): the host-buffer entry points then access it directly from the device.  Undo with unpin() BEFORE the array is
    freed (host_empty() gives memory the library owns instead)."""
    a = _np.asarray(array)
    if not a.flags["C_CONTIGUOUS"]:
        raise InvalidArgument("pin: array must be C-contiguous")
    _check(load().hnsw_host_register(_ptr(a), a.nbytes))
    return array


def unpin(array):
    """hnsw_host_unregister"""
    _check(load().hnsw_host_unregister(_ptr(_np.asarray(array))))


STAGE_EXACT = 0xFFFFFFFF   # out_stage of a query hnsw_search_batch_filtered answered by the masked exact scan


def pack_allow(allow, n, id_base=0):
    """The words hnsw_filter_create takes (uint32 [ceil(n / 32)], bit v & 31 of word v >> 5 = 0-based node v) from a boolean array
    of length n, or from an array of node ids (id_base-based; an id twice is not an error)."""
    a = _np.asarray(allow)
    if a.dtype == _np.bool_:
        if a.shape != (n,):
            raise InvalidArgument("a boolean mask must have the index's n = %d entries" % n)
        mask = a
    else:
        ids = a.astype(_np.int64).reshape(-1) - id_base
        if a.size and (a.dtype.kind not in "iu" or ids.min() < 0 or ids.max() >= n):
            raise InvalidArgument("allowed ids must be integers in id_base .. id_base + n - 1")
        mask = _np.zeros(n, _np.bool_)
        mask[ids] = True
    words = (n + 31) // 32
    padded = _np.zeros(words * 32, _np.uint8)
    padded[:n] = mask
    return _np.packbits(padded, bitorder="little").view("<u4").astype(_np.uint32) if words else _np.zeros(0, _np.uint32)


class _Owner:
    """What every class that owns one library handle shares: the handle is kept in the attribute _slot names (None once released),
    _destroy names the call that gives it back, _gone is what `handle` says afterwards."""
    _slot = _destroy = _gone = None

    @property
    def handle(self):
        h = getattr(self, self._slot, None)
        if h is None:
            raise InvalidArgument(self._gone)
        return h

    def release(self):
        h = getattr(self, self._slot, None)
        if h is not None:
            getattr(load(), self._destroy)(h)
            setattr(self, self._slot, None)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Filter(_Owner):
    """An allow-mask over the nodes of one index, resident on its device (hnsw_filter_create); see Hgraph.filter."""
    _slot, _destroy, _gone = "_f", "hnsw_filter_destroy", "filter already released"

    def __init__(self, hgraph, allow):
        self._f = None
        n = hgraph.info().n
        bits = pack_allow(allow, n, hgraph.id_base)
        f = _C.c_void_p()
        _check(load().hnsw_filter_create(hgraph.handle, _ptr(bits) if len(bits) else None, n, _C.byref(f)))
        self._f, self._hg, self.n = f, hgraph, n

    @classmethod
    def _adopt(cls, hgraph, f, n):
        """a Filter around a handle the library made (hnsw_filter_create_by_label)"""
        self = cls.__new__(cls)
        self._f, self._hg, self.n = f, hgraph, n
        return self

    def count(self):
        """hnsw_filter_count: the number of allowed nodes"""
        c = _C.c_int64(0)
        _check(load().hnsw_filter_count(self.handle, _C.byref(c)))
        return c.value

    def bits(self):
        """hnsw_filter_bits: the mask as the device holds it, in pack_allow's layout (uint32 [ceil(n / 32)], bits past n clear)"""
        out = _np.zeros((self.n + 31) // 32, _np.uint32)
        _check(load().hnsw_filter_bits(self.handle, _ptr(out) if len(out) else _C.byref(_C.c_uint32())))
        return out


class Labels(_Owner):
    """One label per node of one index, resident on its device (hnsw_labels_create); see Hgraph.labels."""
    _slot, _destroy, _gone = "_l", "hnsw_labels_destroy", "labels already released"

    def __init__(self, hgraph, labels, n_labels=None):
        self._l = None
        lab = _np.asarray(labels)
        if lab.dtype.kind not in "iu" or lab.ndim != 1:
            raise InvalidArgument("labels must be a vector of integers, one per node")
        if lab.size and (lab.min() < -(2 ** 31) or lab.max() >= 2 ** 31):
            raise InvalidArgument("labels must fit 32 bits")
        lab = _np.ascontiguousarray(lab, _np.int32)
        if n_labels is None:
            n_labels = max(int(lab.max()) + 1, 1) if lab.size else 1
        if n_labels < 1:
            raise InvalidArgument("n_labels must be >= 1")
        h = _C.c_void_p()
        _check(load().hnsw_labels_create(hgraph.handle, _ptr(lab) if lab.size else None, lab.size, int(n_labels), _C.byref(h)))
        self._l, self._hg, self.n = h, hgraph, lab.size

    def info(self):
        """hnsw_labels_info -> (n_labels, n_labelled, n_groups): nodes with a label >= 0, labels at least one node carries"""
        a, b, c = _C.c_int32(0), _C.c_int64(0), _C.c_int64(0)
        _check(load().hnsw_labels_info(self.handle, _C.byref(a), _C.byref(b), _C.byref(c)))
        return a.value, b.value, c.value

    def get(self):
        """hnsw_labels_get: the n labels as the device holds them (-1 where the node was marked deleted at creation)"""
        out = _np.zeros(self.n, _np.int32)
        _check(load().hnsw_labels_get(self.handle, _ptr(out) if self.n else _C.byref(_C.c_int32())))
        return out


def _grouped_args(hgraph, labels, flt):
    if not isinstance(labels, Labels):
        raise InvalidArgument("labels must be a Labels object (Hgraph.labels)")
    own = None if flt is None or isinstance(flt, Filter) else Filter(hgraph, flt)
    return own, (None if flt is None else (own or flt).handle)


def _search_grouped(hgraph, labels, batch, ef, k, fill, counters=False, sem=0, flt=None):
    """hnsw_search_batch_grouped; labels: a Labels; flt: None, a Filter, or what Hgraph.filter takes
    -> (ids, dist, labels), with counters (ids, dist, labels, ndist, nhops, stage)."""
    own, fh = _grouped_args(hgraph, labels, flt)
    try:
        Q, qs, nq = _batch(hgraph.d, batch)
        ids, dist = _out_pair(nq, k, None)
        lab = _np.empty((nq, max(k, 0)), _np.int32)
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        stage = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_search_batch_grouped(hgraph.handle, labels.handle, fh, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist), _ptr(lab),
                                                _ptr(nd), _ptr(nh), _ptr(stage)))
    finally:
        if own is not None:
            own.release()
    return (ids, dist, lab, nd, nh, stage) if counters else (ids, dist, lab)


def _search_filtered(hgraph, flt, batch, ef, k, fill, counters=False, sem=0, out=None):
    """hnsw_search_batch_filtered; flt: a Filter, or what Hgraph.filter takes (a mask made for this call)
    -> (ids, dist), with counters (ids, dist, ndist, nhops, stage)."""
    own = None if isinstance(flt, Filter) else Filter(hgraph, flt)
    try:
        Q, qs, nq = _batch(hgraph.d, batch)
        ids, dist = _out_pair(nq, k, out)
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        stage = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_search_batch_filtered(hgraph.handle, (own or flt).handle, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist),
                                                 _ptr(nd), _ptr(nh), _ptr(stage)))
    finally:
        if own is not None:
            own.release()
    return (ids, dist, nd, nh, stage) if counters else (ids, dist)


CURSOR_DTYPE = _np.dtype([("dist", "<f4"), ("id", "<i4")])     # hnsw_cursor: the (distance, id) a page ends at
CURSOR_START = _np.array((-_np.inf, -2 ** 31), dtype=CURSOR_DTYPE)[()]   # HNSW_CURSOR_START: before every node


def _cursors(after, nq):
    """the cursors of a paged call as the library reads them: None (the start cursor for every query), one cursor for all, or [nq]"""
    if after is None:
        return None
    a = _np.asarray(after, dtype=CURSOR_DTYPE)
    if a.ndim == 0:
        a = _np.full(nq, a, dtype=CURSOR_DTYPE)
    if a.shape != (nq,):
        raise InvalidArgument("after must be one cursor per query: [nq] of dtype CURSOR_DTYPE")
    return _np.ascontiguousarray(a)


def _search_after(hgraph, batch, after, ef, k, fill, counters=False, sem=0, flt=None):
    """hnsw_search_batch_after (ef None: hnsw_brute_force_batch_after); flt: None, a Filter, or what Hgraph.filter takes
    -> (ids, dist, next), with counters (ids, dist, next, ndist, nhops, stage)."""
    own = None if flt is None or isinstance(flt, Filter) else Filter(hgraph, flt)
    try:
        f = None if flt is None else (own or flt).handle
        Q, qs, nq = _batch(hgraph.d, batch)
        cur = _cursors(after, nq)
        ids, dist = _out_pair(nq, int(k), None)
        nxt = _np.empty(nq, CURSOR_DTYPE)
        if ef is None:
            if counters:
                raise InvalidArgument("the brute-force form has no counters")
            _check(load().hnsw_brute_force_batch_after(hgraph.handle, f, _ptr(cur), _ptr(Q), nq, qs, int(k), fill, _ptr(ids), _ptr(dist), _ptr(nxt)))
            return ids, dist, nxt
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        stage = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_search_batch_after(hgraph.handle, f, _ptr(cur), _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist), _ptr(nxt),
                                              _ptr(nd), _ptr(nh), _ptr(stage)))
    finally:
        if own is not None:
            own.release()
    return (ids, dist, nxt, nd, nh, stage) if counters else (ids, dist, nxt)


def _search_diverse(hgraph, batch, ef, k, pool, lam, fill, counters=False, sem=0, flt=None):
    """hnsw_search_batch_diverse (ef None: hnsw_brute_force_batch_diverse); flt: None, a Filter, or what Hgraph.filter takes
    -> (ids, dist, div), with counters (ids, dist, div, ndist, nhops, status)."""
    own = None if flt is None or isinstance(flt, Filter) else Filter(hgraph, flt)
    try:
        Q, qs, nq = _batch(hgraph.d, batch)
        ids, dist = _out_pair(nq, int(k), None)
        div = _np.empty((nq, max(int(k), 0)), _np.float32)
        if ef is None:
            if counters or flt is not None:
                raise InvalidArgument("the brute-force form has no counters and takes no filter")
            _check(load().hnsw_brute_force_batch_diverse(hgraph.handle, _ptr(Q), nq, qs, int(k), int(pool), float(lam), fill, _ptr(ids), _ptr(dist),
                                                         _ptr(div)))
            return ids, dist, div
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        status = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_search_batch_diverse(hgraph.handle, None if flt is None else (own or flt).handle, _ptr(Q), nq, qs, _C.byref(p), int(pool),
                                                float(lam), _ptr(ids), _ptr(dist), _ptr(div), _ptr(nd), _ptr(nh), _ptr(status)))
    finally:
        if own is not None:
            own.release()
    return (ids, dist, div, nd, nh, status) if counters else (ids, dist, div)


def _search_keyed(hgraph, batch, ef, k, fill, counters=False, sem=0, flt=None, missing=MISSING_KEY):
    """hnsw_search_batch_keyed; flt: None, a Filter, or what Hgraph.filter takes
    -> (keys, dist), with counters (keys, dist, ndist, nhops, stage)."""
    own = None if flt is None or isinstance(flt, Filter) else Filter(hgraph, flt)
    try:
        Q, qs, nq = _batch(hgraph.d, batch)
        keys = _np.empty((nq, max(k, 0)), _np.int64)
        dist = _np.empty((nq, max(k, 0)), _np.float32)
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        stage = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_search_batch_keyed(hgraph.handle, None if flt is None else (own or flt).handle, _ptr(Q), nq, qs, _C.byref(p),
                                              int(missing), _ptr(keys), _ptr(dist), _ptr(nd), _ptr(nh), _ptr(stage)))
    finally:
        if own is not None:
            own.release()
    return (keys, dist, nd, nh, stage) if counters else (keys, dist)


def _search_filtered_each(hgraph, filters, which, batch, ef, k, fill, counters=False, sem=0, out=None):
    """hnsw_search_batch_filtered_each; filters: a sequence of Filter, which: per query the position of its filter in it
    -> (ids, dist), with counters (ids, dist, ndist, nhops, stage)."""
    filters = list(filters)
    for f in filters:
        if not isinstance(f, Filter):
            raise InvalidArgument("filters must be Filter objects (Hgraph.filter, Hgraph.filters_by_label)")
    Q, qs, nq = _batch(hgraph.d, batch)
    w = _np.asarray(which)
    if w.shape != (nq,) or (nq and w.dtype.kind not in "iu"):
        raise InvalidArgument("which must hold one filter position per query")
    if nq and (w.min() < 0 or w.max() >= len(filters)):
        raise InvalidArgument("which must name positions 0 .. %d of filters" % (len(filters) - 1))
    w = _np.ascontiguousarray(w, _np.int32)
    table = (_C.c_void_p * max(len(filters), 1))(*[f.handle for f in filters])
    ids, dist = _out_pair(nq, k, out)
    nd = _np.zeros(nq, _np.uint32) if counters else None
    nh = _np.zeros(nq, _np.uint32) if counters else None
    stage = _np.zeros(nq, _np.uint32) if counters else None
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch_filtered_each(hgraph.handle, table, len(filters), _ptr(w) if nq else None, _ptr(Q), nq, qs, _C.byref(p),
                                                  _ptr(ids), _ptr(dist), _ptr(nd), _ptr(nh), _ptr(stage)))
    return (ids, dist, nd, nh, stage) if counters else (ids, dist)


class RangeResult(_Owner):
    """What a range call returns, resident on the index's device (hnsw_range_result): lims [nq + 1], ids and distances [total];
    query q's segment is [lims[q], lims[q + 1]).  For callers who keep the result on the device (device_pointers) or fetch parts
    of it; Ohnsw.range_search and its kin fetch everything and release it."""
    _prefix, _id = "hnsw_range_result_", _np.int32             # the ABI functions' common prefix; what an id is
    _slot, _destroy, _gone = "_r", _prefix + "destroy", "range result already released"

    def __init__(self, handle):
        self._r = handle

    def _call(self, name, *args):
        _check(getattr(load(), self._prefix + name)(self.handle, *args))

    def size(self):
        """hnsw_range_result_size -> (nq, total)"""
        nq, total = _C.c_int64(0), _C.c_int64(0)
        self._call("size", _C.byref(nq), _C.byref(total))
        return nq.value, total.value

    def fetch(self, counters=False):
        """hnsw_range_result_fetch -> (lims int64 [nq + 1], ids [total] (int32; ShardedRangeResult: int64), distances float32
        [total]), with counters also (ndist, nhops, stage), uint32 [nq] each"""
        nq, total = self.size()
        lims, ids, dist = _np.zeros(nq + 1, _np.int64), _np.empty(total, self._id), _np.empty(total, _np.float32)
        cnt = [_np.zeros(nq, _np.uint32) for _ in range(3)] if counters else [None] * 3
        self._call("fetch", _ptr(lims), _ptr(ids), _ptr(dist), _ptr(cnt[0]), _ptr(cnt[1]), _ptr(cnt[2]))
        return (lims, ids, dist) + tuple(cnt) if counters else (lims, ids, dist)

    def device_pointers(self):
        """hnsw_range_result_device -> the device addresses (lims, ids, distances) as integers, valid until release"""
        p = [_C.c_void_p() for _ in range(3)]
        self._call("device", _C.byref(p[0]), _C.byref(p[1]), _C.byref(p[2]))
        return tuple(x.value or 0 for x in p)

    def _take(self, counters, keep):
        """the result itself (keep), or everything fetched and the device copy released"""
        if keep:
            return self
        try:
            return self.fetch(counters)
        finally:
            self.release()


def _range_search(hgraph, batch, radius, ef, sem=0, counters=False, keep=False, filter=None):
    """hnsw_range_search_batch (ef None: hnsw_range_brute_force_batch) -> what RangeResult.fetch gives; keep: the RangeResult.
    filter: a Filter, or what Hgraph.filter takes (a mask made for this call): the _filtered forms of the two calls"""
    Q, qs, nq = _batch(hgraph.d, batch)
    r = _C.c_void_p()
    own = None if filter is None or isinstance(filter, Filter) else Filter(hgraph, filter)
    try:
        f = None if filter is None else (own or filter).handle
        if ef is None and f is None:
            _check(load().hnsw_range_brute_force_batch(hgraph.handle, _ptr(Q), nq, qs, float(radius), _C.byref(r)))
        elif ef is None:
            _check(load().hnsw_range_brute_force_batch_filtered(hgraph.handle, f, _ptr(Q), nq, qs, float(radius), _C.byref(r)))
        else:
            p = _RangeParams(float(radius), int(ef), sem)
            if f is None:
                _check(load().hnsw_range_search_batch(hgraph.handle, _ptr(Q), nq, qs, _C.byref(p), _C.byref(r)))
            else:
                _check(load().hnsw_range_search_batch_filtered(hgraph.handle, f, _ptr(Q), nq, qs, _C.byref(p), _C.byref(r)))
    finally:
        if own is not None:
            own.release()
    return RangeResult(r)._take(counters, keep)


def _ids32(ids):
    """the ids of a call by stored item as the library reads them: contiguous int32, id_base-based (a search's output fits as it is)"""
    a = _np.asarray(ids)
    if a.size and a.dtype.kind not in "iu":
        raise InvalidArgument("ids must be integers")
    if a.size and (int(a.max()) > 2 ** 31 - 1 or int(a.min()) < -2 ** 31):
        raise InvalidArgument("ids must fit a signed 32-bit integer")
    return _np.ascontiguousarray(a, dtype=_np.int32).reshape(-1)


def _search_by_id(hgraph, ids, ef, k, fill, exclude_self=True, counters=False, sem=0, out=None):
    """hnsw_search_batch_by_id: the stored rows `ids` as the queries -> (ids, dist), with counters (ids, dist, ndist, nhops)"""
    q = _ids32(ids)
    nq = q.size
    oi, od = _out_pair(nq, k, out)
    nd = _np.zeros(nq, _np.uint32) if counters else None
    nh = _np.zeros(nq, _np.uint32) if counters else None
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch_by_id(hgraph.handle, _ptr(q), nq, _C.byref(p), int(exclude_self), _ptr(oi), _ptr(od), _ptr(nd), _ptr(nh)))
    return (oi, od, nd, nh) if counters else (oi, od)


def _search_by_key(hgraph, keys, ef, k, fill, exclude_self=True, counters=False, sem=0, missing=MISSING_KEY):
    """hnsw_search_batch_by_key: the stored rows under `keys` as the queries -> (keys, dist), with counters (keys, dist, ndist, nhops)"""
    q = _keys(keys)
    nq = q.size
    ok = _np.empty((nq, max(k, 0)), _np.int64)
    od = _np.empty((nq, max(k, 0)), _np.float32)
    nd = _np.zeros(nq, _np.uint32) if counters else None
    nh = _np.zeros(nq, _np.uint32) if counters else None
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch_by_key(hgraph.handle, _ptr(q), nq, _C.byref(p), int(exclude_self), int(missing), _ptr(ok), _ptr(od),
                                           _ptr(nd), _ptr(nh)))
    return (ok, od, nd, nh) if counters else (ok, od)


def _search(hgraph, batch, ef, k, fill, counters=False, sem=0, out=None):
    Q, qs, nq = _batch(hgraph.d, batch)
    ids, dist = _out_pair(nq, k, out)
    nd = _np.zeros(nq, _np.uint32) if counters else None
    nh = _np.zeros(nq, _np.uint32) if counters else None
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch(hgraph.handle, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist), _ptr(nd), _ptr(nh)))
    return (ids, dist, nd, nh) if counters else (ids, dist)


class Request:
    """A batch in flight (hnsw_search_submit): `wait()` returns what the synchronous call would have.
    Lets a caller overlap consecutive batches (the next one fills the drain of the previous one):
        r1 = submit(hg, b1, ef, k); r2 = submit(hg, b2, ef, k); ids1, d1 = r1.wait(); ..."""

    def __init__(self, hgraph, handle, nq, k, keep):
        self._hg, self._h, self.nq, self.k, self._keep = hgraph, handle, nq, k, keep

    def wait(self, counters=False, out=None):
        if self._h is None:
            raise InvalidArgument("request already waited for")
        ids, dist = _out_pair(self.nq, self.k, out)
        nd = _np.zeros(self.nq, _np.uint32) if counters else None
        nh = _np.zeros(self.nq, _np.uint32) if counters else None
        h, self._h, self._keep = self._h, None, None
        _check(load().hnsw_search_wait(h, _ptr(ids), _ptr(dist), _ptr(nd), _ptr(nh)))
        return (ids, dist, nd, nh) if counters else (ids, dist)


def submit(hgraph, batch, ef, k, fill=FILL_OHNSW, sem=SEM_OHNSW):
    """hnsw_search_submit: copy the batch in, start the search, return at once."""
    Q, qs, nq = _batch(hgraph.d, batch, 1)
    p = _SearchParams(ef, k, fill, sem)
    h = _C.c_void_p()
    _check(load().hnsw_search_submit(hgraph.handle, _ptr(Q), nq, qs, _C.byref(p), _C.byref(h)))
    return Request(hgraph, h, nq, k, Q)


def search_batch_device(hgraph, d_queries, nq, q_stride, ef, k, d_ids, d_dist, d_ndist=0, d_nhops=0,
                        d_status=0, stream=0, fill=FILL_OHNSW, sem=SEM_OHNSW):
    """Asynchronous search on device pointers (ints), on HIP stream `stream` (int handle)."""
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch_device(hgraph.handle, d_queries, nq, q_stride, _C.byref(p), d_ids,
                                           d_dist, d_ndist or None, d_nhops or None,
                                           d_status or None, stream or None))


def brute_force_device(hgraph, d_queries, nq, q_stride, k, d_ids, d_dist, fill=FILL_OHNSW, stream=0):
    """hnsw_brute_force_batch_device: the exact scan on device pointers (ints), asynchronous on HIP stream `stream`."""
    _check(load().hnsw_brute_force_batch_device(hgraph.handle, d_queries, nq, q_stride, k, fill, d_ids, d_dist, stream or None))


def rows_device(hgraph, d_ids, m, d_out, out_stride, stream=0):
    """hnsw_index_get_rows_device: the stored float32 rows of the nodes d_ids (device int32, id_base-based) into the device matrix
    d_out, rows out_stride floats apart (pointers as ints), asynchronous on HIP stream `stream`; an id outside the index gives a
    row of zeros.  With search_batch_device a device-resident caller composes its own search by id."""
    _check(load().hnsw_index_get_rows_device(hgraph.handle, d_ids or None, m, d_out or None, out_stride, stream or None))


def rerank_device(hgraph, d_queries, nq, q_stride, d_cand, cand_stride, k, d_ids, d_dist, fill=FILL_OHNSW, stream=0):
    """hnsw_rerank_batch_device: the exact re-rank of given candidates on device pointers (ints), asynchronous on HIP stream
    `stream`."""
    _check(load().hnsw_rerank_batch_device(hgraph.handle, d_queries, nq, q_stride, d_cand, cand_stride, k, fill, d_ids, d_dist,
                                           stream or None))


def diversify_device(hgraph, d_queries, nq, q_stride, d_cand, cand_stride, k, lam, d_ids, d_dist, d_div=0, fill=FILL_OHNSW, stream=0):
    """hnsw_diversify_batch_device: the greedy MMR selection among given candidates on device pointers (ints), asynchronous on HIP
    stream `stream`; d_div optional."""
    _check(load().hnsw_diversify_batch_device(hgraph.handle, d_queries, nq, q_stride, d_cand, cand_stride, k, float(lam), fill, d_ids, d_dist,
                                              d_div or None, stream or None))


def search_batch_h2d(hgraph, batch, ef, k, d_ids, d_dist, d_ndist=0, d_nhops=0, d_status=0, stream=0,
                     fill=FILL_OHNSW, sem=SEM_OHNSW):
    """hnsw_search_batch_h2d: queries from a HOST matrix (read by the device directly when it was registered with pin()),
    results left in device buffers (pointers as ints), asynchronous on HIP stream `stream`.  The matrix must stay alive
    until the stream has passed the call."""
    Q, qs, nq = _batch(hgraph.d, batch, 1)
    p = _SearchParams(ef, k, fill, sem)
    _check(load().hnsw_search_batch_h2d(hgraph.handle, _ptr(Q), nq, qs, _C.byref(p), d_ids, d_dist,
                                        d_ndist or None, d_nhops or None, d_status or None, stream or None))
    return Q          # the array the device reads: keep it alive until the stream is synchronised


class Ohnsw:
    """lib/ohnsw.ml -- the imperative API, 0-based ids, ef == k unless `ef` is given."""

    @staticmethod
    def knn(hgraph, k, target, ef=None):
        """Ohnsw.knn hgraph visited ~k target (lib/ohnsw.ml:859-875) -> [(node, distance)] ascending
        (the reference returns a MinQueue popped in that order, :886-893)."""
        ids, dist = _search(hgraph, _np.asarray(target, _np.float32)[None, :], k if ef is None else ef, k, FILL_OHNSW)
        return [(int(i), float(d)) for i, d in zip(ids[0], dist[0]) if i >= hgraph.id_base]

    @staticmethod
    def knn_batch_bigarray(hgraph, k, batch, ef=None, counters=False, out=None):
        """Ohnsw.knn_batch_bigarray hgraph ~k batch (lib/ohnsw.ml:877-897) -> (ids, distances):
        ids [nq][k] (-1 where fewer than k were found), distances [nq][k] fp32 (NaN there).
        out = (ids, distances): write into the caller's matrices instead of fresh ones."""
        return _search(hgraph, batch, k if ef is None else ef, k, FILL_OHNSW, counters, out=out)

    @staticmethod
    def knn_batch_filtered(hgraph, k, batch, allow, ef=None, counters=False, out=None):
        """knn_batch_bigarray among the nodes `allow` names (hnsw_search_batch_filtered) -> (ids, distances), with counters
        (ids, distances, ndist, nhops, stage).  allow: a Filter (Hgraph.filter: uploaded once, reused), a boolean array of length
        n or an array of ids.  W grows ef, 2 ef, ... 1024 until it holds k allowed nodes (stage = how often it doubled); a query
        still short gets the exact scan over the allowed nodes (stage = STAGE_EXACT).  Distances are over the float32 vectors
        whatever rows the index searches; ids -1 / NaN where fewer than k nodes are allowed."""
        return _search_filtered(hgraph, allow, batch, k if ef is None else ef, k, FILL_OHNSW, counters, out=out)

    @staticmethod
    def knn_batch_filtered_each(hgraph, k, batch, filters, which, ef=None, counters=False, out=None):
        """knn_batch_filtered with one filter per query (hnsw_search_batch_filtered_each): query q is answered under
        filters[which[q]], and its row is the row knn_batch_filtered gives it under that filter.  filters: Filter objects
        (Hgraph.filter, Hgraph.filters_by_label); which: one position in `filters` per query.  A mixed batch of many tenants is ONE
        call: every ladder stage walks all queries still short in one launch, whatever their filters."""
        return _search_filtered_each(hgraph, filters, which, batch, k if ef is None else ef, k, FILL_OHNSW, counters, out=out)

    @staticmethod
    def range_search(hgraph, radius, batch, ef=64, counters=False, keep=False, filter=None):
        """EVERY node within `radius` of each query (hnsw_range_search_batch) -> (lims, ids, distances), with counters (lims, ids,
        distances, ndist, nhops, stage): query q's segment is ids / distances [lims[q], lims[q + 1]), ascending under (distance,
        id).  A query is served by the first search of the ladder e = ef, 2 ef, ... 1024 whose W is not saturated (fewer than e
        members, or the last one out of range): W's in-range prefix; a query saturated at 1024 gets the exact range scan (stage =
        STAGE_EXACT).  Distances are over the float32 vectors whatever rows the index searches.  keep: the RangeResult itself,
        left on the device.  filter (a Filter, or what Hgraph.filter takes): hnsw_range_search_batch_filtered -- each segment is the
        unfiltered one with the nodes the filter does not allow left out; stage and hops are the unfiltered call's."""
        return _range_search(hgraph, batch, radius, ef, SEM_OHNSW, counters, keep, filter)

    @staticmethod
    def brute_force_range(hgraph, radius, batch, counters=False, keep=False, filter=None):
        """The exact range search (hnsw_range_brute_force_batch) -> (lims, ids, distances): per query the in-range prefix of the
        full order (distance, id) over all n vectors.  Needs no graph.  filter: over the allowed vectors only
        (hnsw_range_brute_force_batch_filtered)."""
        return _range_search(hgraph, batch, radius, None, SEM_OHNSW, counters, keep, filter)

    @staticmethod
    def brute_force_knn(hgraph, k, batch, fill=FILL_OHNSW, out=None):
        """brute_force_knn_l2 (benchmark/dataset.ml:15-30) over the vectors the index holds, with its metric
        (hnsw_brute_force_batch) -> (ids, distances): for each query the k smallest of all n vectors under (distance, id),
        ascending; ids [nq][k] (-1 where k > n), distances [nq][k] fp32 (NaN there; FILL_BA: +inf).  Needs no graph.
        out = (ids, distances): write into the caller's matrices instead of fresh ones."""
        Q, qs, nq = _batch(hgraph.d, batch)
        ids, dist = _out_pair(nq, int(k), out)
        _check(load().hnsw_brute_force_batch(hgraph.handle, _ptr(Q), nq, qs, int(k), fill, _ptr(ids), _ptr(dist)))
        return ids, dist

    @staticmethod
    def knn_batch_grouped(hgraph, k, batch, labels, ef=None, filter=None, counters=False):
        """The k nearest GROUPS, one node per label (hnsw_search_batch_grouped) -> (ids, distances, labels), with counters (ids,
        distances, labels, ndist, nhops, stage).  labels: a Labels (Hgraph.labels).  W grows ef, 2 ef, ... 1024 until it holds nodes
        of k distinct labels (stage = how often it doubled), each label represented by its first member of W; a query still short
        gets the exact grouped scan (stage = STAGE_EXACT).  filter (a Filter, or what Hgraph.filter takes): only allowed nodes
        count.  Distances are over the float32 vectors whatever rows the index searches; id -1 / label -1 / NaN where there are
        fewer than k groups."""
        return _search_grouped(hgraph, labels, batch, k if ef is None else ef, k, FILL_OHNSW, counters, flt=filter)

    @staticmethod
    def knn_batch_keyed(hgraph, k, batch, ef=None, filter=None, counters=False, missing=MISSING_KEY):
        """knn_batch_bigarray answered in the index's keys (hnsw_search_batch_keyed; Hgraph.set_keys) -> (keys, distances), with
        counters (keys, distances, ndist, nhops, stage): keys [nq][k] int64, `missing` where fewer than k were found.  filter (a
        Filter, or what Hgraph.filter takes): the rows of knn_batch_filtered instead.  Distances and counters are those calls'."""
        return _search_keyed(hgraph, batch, k if ef is None else ef, k, FILL_OHNSW, counters, flt=filter, missing=missing)

    @staticmethod
    def knn_batch_after(hgraph, k, batch, after=None, ef=None, filter=None, counters=False):
        """The NEXT k: knn_batch_bigarray's results that come after a cursor (hnsw_search_batch_after) -> (ids, distances, next), with
        counters (ids, distances, next, ndist, nhops, stage).  after: one (distance, id) per query (CURSOR_DTYPE; None: CURSOR_START,
        the first page) -- feed `next` back for the page after.  The order is (distance, id) over the returned float distances.  W
        grows ef, 2 ef, ... 1024 until it holds k nodes after the cursor; a query still short gets the exact paged scan (stage =
        STAGE_EXACT), so a row with fewer than k real entries means "exhausted".  filter (a Filter, or what Hgraph.filter takes):
        only allowed nodes count.  Cursors do not survive remove_batch, compact or an upsert: those renumber the nodes."""
        return _search_after(hgraph, batch, after, k if ef is None else ef, k, FILL_OHNSW, counters, flt=filter)

    @staticmethod
    def brute_force_after(hgraph, k, batch, after=None, filter=None, fill=FILL_OHNSW):
        """The exact form of knn_batch_after (hnsw_brute_force_batch_after) -> (ids, distances, next): per query the first k nodes
        after its cursor under (distance, id) over all n vectors, allowed by `filter` if given.  Needs no graph; each page is one
        pass over the table."""
        return _search_after(hgraph, batch, after, None, k, fill, flt=filter)

    @staticmethod
    def knn_pages(hgraph, k, batch, ef=None, filter=None, exact=False):
        """A generator over the pages of knn_batch_after (exact=True: of brute_force_after), from the start cursor on: yields (ids,
        distances, next) and stops after the page on which every row is exhausted (has fewer than k real entries)."""
        own = None if filter is None or isinstance(filter, Filter) else Filter(hgraph, filter)
        try:
            cur = None
            while True:
                if exact:
                    page = Ohnsw.brute_force_after(hgraph, k, batch, cur, filter=own or filter)
                else:
                    page = Ohnsw.knn_batch_after(hgraph, k, batch, cur, ef=ef, filter=own or filter)
                yield page
                if ((page[0] >= hgraph.id_base).sum(axis=1) < k).all():
                    return
                cur = page[2]
        finally:
            if own is not None:
                own.release()

    @staticmethod
    def knn_batch_by_id(hgraph, k, ids, ef=None, exclude_self=True, counters=False, out=None):
        """knn_batch_bigarray with the stored vectors of the nodes `ids` as the queries (hnsw_search_batch_by_id) -> (ids, distances),
        with counters (ids, distances, ndist, nhops).  Only the ids cross the link: the rows are gathered on the device.
        exclude_self=False: exactly knn_batch_bigarray(hgraph, k, hgraph.rows(ids), ef).  exclude_self=True ("more like this"): the
        search runs k + 1 wide with ef' = max(ef, k + 1) and each row has the node's own id removed -- the first k entries if the
        node is not among them.  ids: int32, id_base-based: a search's output can be fed straight back."""
        return _search_by_id(hgraph, ids, k if ef is None else ef, k, FILL_OHNSW, exclude_self, counters, out=out)

    @staticmethod
    def knn_batch_by_key(hgraph, k, keys, ef=None, exclude_self=True, counters=False, missing=MISSING_KEY):
        """knn_batch_by_id for the nodes stored under `keys`, answered in keys (hnsw_search_batch_by_key) -> (keys, distances), with
        counters (keys, distances, ndist, nhops).  An absent key is refused.  Distances and counters are the by-id call's."""
        return _search_by_key(hgraph, keys, k if ef is None else ef, k, FILL_OHNSW, exclude_self, counters, missing=missing)

    @staticmethod
    def brute_force_by_id(hgraph, k, ids, exclude_self=True, fill=FILL_OHNSW):
        """brute_force_knn with the stored vectors of the nodes `ids` as the queries (hnsw_brute_force_batch_by_id) -> (ids,
        distances); exclude_self as in knn_batch_by_id.  Needs no graph."""
        q = _ids32(ids)
        oi, od = _out_pair(q.size, int(k), None)
        _check(load().hnsw_brute_force_batch_by_id(hgraph.handle, _ptr(q), q.size, int(k), fill, int(exclude_self), _ptr(oi), _ptr(od)))
        return oi, od

    @staticmethod
    def brute_force_grouped(hgraph, k, batch, labels, filter=None, fill=FILL_OHNSW):
        """The exact grouped search (hnsw_brute_force_batch_grouped) -> (ids, distances, labels): per label its nearest node under
        (distance, id) over all n float32 vectors, of those the k nearest, ascending.  Needs no graph."""
        own, fh = _grouped_args(hgraph, labels, filter)
        try:
            Q, qs, nq = _batch(hgraph.d, batch)
            ids, dist = _out_pair(nq, int(k), None)
            lab = _np.empty((nq, max(int(k), 0)), _np.int32)
            _check(load().hnsw_brute_force_batch_grouped(hgraph.handle, labels.handle, fh, _ptr(Q), nq, qs, int(k), fill, _ptr(ids), _ptr(dist),
                                                         _ptr(lab)))
        finally:
            if own is not None:
                own.release()
        return ids, dist, lab

    @staticmethod
    def rerank(hgraph, k, batch, cand, fill=FILL_OHNSW, out=None):
        """hnsw_rerank_batch -> (ids, distances): for each query the k nearest of ITS candidates cand[q] (int32 [nq][cand_stride],
        entries below id_base are padding) over the float32 vectors, under (distance, id), ascending; ids [nq][k] (-1 past the
        real candidates), distances [nq][k] fp32 (NaN there; FILL_BA: +inf).  What option "refine" does to the half-row
        searches' candidates.  Needs no graph.  out = (ids, distances): write into the caller's matrices instead of fresh ones."""
        Q, qs, nq = _batch(hgraph.d, batch)
        C = _np.ascontiguousarray(cand, _np.int32)
        if C.ndim != 2 or C.shape[0] != nq:
            raise InvalidArgument("cand must be [nq][cand_stride]")
        ids, dist = _out_pair(nq, int(k), out)
        _check(load().hnsw_rerank_batch(hgraph.handle, _ptr(Q), nq, qs, _ptr(C), C.shape[1], int(k), fill, _ptr(ids), _ptr(dist)))
        return ids, dist

    @staticmethod
    def diversify(hgraph, k, batch, cand, lam=0.5, fill=FILL_OHNSW):
        """hnsw_diversify_batch -> (ids, distances, div): greedy maximal marginal relevance among ITS candidates cand[q] (int32
        [nq][cand_stride], entries below id_base are padding, as rerank's).  Pick 1 is the nearest candidate; every further pick
        minimises lam * distance to the query - (1 - lam) * distance to the nearest node already picked, three float32 operations,
        ties to the candidate rerank ranks first.  Rows are in SELECTION order: ids [nq][k] (-1 past the real candidates),
        distances to the query (NaN there; FILL_BA: +inf) and div, the distance to the nearest earlier pick at the moment of
        selection (+inf for pick 1).  lam = 1 is rerank.  Needs no graph; only [nq][k] comes back."""
        Q, qs, nq = _batch(hgraph.d, batch)
        C = _np.ascontiguousarray(cand, _np.int32)
        if C.ndim != 2 or C.shape[0] != nq:
            raise InvalidArgument("cand must be [nq][cand_stride]")
        ids, dist = _out_pair(nq, int(k), None)
        div = _np.empty((nq, max(int(k), 0)), _np.float32)
        _check(load().hnsw_diversify_batch(hgraph.handle, _ptr(Q), nq, qs, _ptr(C), C.shape[1], int(k), float(lam), fill, _ptr(ids), _ptr(dist),
                                           _ptr(div)))
        return ids, dist, div

    @staticmethod
    def knn_batch_diverse(hgraph, k, batch, pool, lam=0.5, ef=None, filter=None, counters=False):
        """k DIVERSE neighbours (hnsw_search_batch_diverse) -> (ids, distances, div), with counters (ids, distances, div, ndist, nhops,
        status): knn_batch_bigarray at k := pool (knn_batch_filtered under `filter`: a Filter, or what Hgraph.filter takes), then
        diversify over its rows -- the pool never leaves the device.  k <= pool <= ef (ef defaults to pool)."""
        return _search_diverse(hgraph, batch, pool if ef is None else ef, k, pool, lam, FILL_OHNSW, counters, flt=filter)

    @staticmethod
    def brute_force_diverse(hgraph, k, batch, pool, lam=0.5, fill=FILL_OHNSW):
        """The exact form of knn_batch_diverse (hnsw_brute_force_batch_diverse) -> (ids, distances, div): brute_force_knn at k := pool
        (k <= pool <= 1024), then diversify over its rows.  Needs no graph."""
        return _search_diverse(hgraph, batch, None, k, pool, lam, fill)

    @staticmethod
    def search_k(hgraph, layer, start_nodes, targets, k, ef=None, sem=SEM_OHNSW, counters=False):
        """Batched Ohnsw.search_k layer distance value visited start_nodes target k ... (lib/ohnsw.ml:
        543-588) on one layer: start_nodes = one id list per target (the start MinQueue; distances
        are recomputed), W bounded by ef (= k, the reference's only shape, unless given).
        -> list per target of [(node, distance)] nearest first (result_minq order)."""
        T, ts = _rows(_np.atleast_2d(_np.asarray(targets, _np.float32)))
        nq = T.shape[0]
        if len(start_nodes) != nq:
            raise InvalidArgument("one start list per target")
        ef = k if ef is None else ef
        ns = max([len(c) for c in start_nodes] + [1])
        st = _np.full((nq, ns), hgraph.id_base - 1, _np.int64)
        for i, c in enumerate(start_nodes):
            st[i, :len(c)] = c
        ids = _np.empty((nq, k), _np.int32)
        dist = _np.empty((nq, k), _np.float32)
        cnt = _np.empty(nq, _np.int32)
        nd = _np.zeros(nq, _np.uint32)
        nh = _np.zeros(nq, _np.uint32)
        p = _SearchParams(ef, k, FILL_OHNSW, sem)
        _check(load().hnsw_search_layer_batch(hgraph.handle, layer, _ptr(T), nq, max(ts, hgraph.d), _ptr(st), ns,
                                              _C.byref(p), _ptr(ids), _ptr(dist), _ptr(cnt), _ptr(nd), _ptr(nh)))
        res = [[(int(ids[i, j]), float(dist[i, j])) for j in range(cnt[i])] for i in range(nq)]
        return (res, nd, nh) if counters else res

    @staticmethod
    def search_one(hgraph, layer, start, targets, with_distance=False):
        """Batched Ohnsw.search_one layer distance value visited start_node target (lib/ohnsw.ml:492-512):
        -> node per target (and its distance)."""
        T, ts = _rows(_np.atleast_2d(_np.asarray(targets, _np.float32)))
        nq = T.shape[0]
        st = _np.ascontiguousarray(_np.broadcast_to(_np.asarray(start, _np.int64), (nq,)))
        node = _np.empty(nq, _np.int64)
        dist = _np.empty(nq, _np.float32)
        _check(load().hnsw_search_one_batch(hgraph.handle, layer, _ptr(T), nq, max(ts, hgraph.d), _ptr(st),
                                            _ptr(node), _ptr(dist)))
        return (node, dist) if with_distance else node

    @staticmethod
    def build_batch_bigarray(batch, num_connections, num_nodes_search_construction, seed=0,
                             metric=METRIC_L2, device=0, max_batch=0, batch_div=0, expected_ef=0, expected_sem=SEM_OHNSW):
        """Ohnsw.build_batch_bigarray distance batch ~num_connections ~num_nodes_search_construction
        (lib/ohnsw.ml:840-857), batched on the device (the OCaml builder itself stays OCaml; this
        is for hosts without one).  -> Hgraph resident in HBM.  expected_ef (optional): the finished index
        is also prepared for searches with that ef (hnsw_build_params.expected_ef)."""
        X = _np.ascontiguousarray(batch, dtype=_np.float32)
        if X.ndim != 2 or X.shape[0] < 1:
            raise InvalidArgument("batch must be [n][d], n >= 1")
        p = _BuildParams(num_connections, num_nodes_search_construction, metric, 0, seed, max_batch, batch_div, expected_ef, expected_sem)
        h = _C.c_void_p()
        _check(load().hnsw_build(_ptr(X), X.shape[0], X.shape[1], X.shape[1], _C.byref(p), device, _C.byref(h)))
        return Hgraph._from_handle(h, device, X)

    @staticmethod
    def insert_batch(hgraph, batch, num_connections, num_nodes_search_construction, seed=0, max_batch=0, batch_div=0,
                     expected_ef=0, expected_sem=SEM_OHNSW, metric=None):
        """Ohnsw.insert (lib/ohnsw.ml:766-837) for every row of `batch`, in order, on the device (hnsw_index_insert): the
        index grows in place (metric: None = the index's own; another one is refused; a METRIC_COSINE index normalises the new
        rows itself).  -> the new ids (np.int64, n_old + id_base onwards).  Levels are the draws hnsw_build with
        the same seed gives those positions.  Afterwards the Hgraph follows the device index: n, widths, max_layer and
        entry_point are refreshed, the host vectors (if any) grow by the batch, and deg0 / nbr0 / upper are None until
        export()."""
        X, xs = _rows(batch)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != hgraph.d):
            raise InvalidArgument("batch must be [m][d] with the index's d = %d" % hgraph.d)
        m = X.shape[0]
        n_old = hgraph.n
        p = _BuildParams(num_connections, num_nodes_search_construction, hgraph.metric if metric is None else int(metric), hgraph.id_base, seed, max_batch,
                         batch_div, expected_ef, expected_sem)
        _check(load().hnsw_index_insert(hgraph.handle, _ptr(X), m, max(xs, hgraph.d), _C.byref(p)))
        if m == 0:
            return _np.arange(0, dtype=_np.int64)
        hgraph._append_vectors(X)
        hgraph._adopt(hgraph.info())
        return _np.arange(n_old + hgraph.id_base, n_old + m + hgraph.id_base, dtype=_np.int64)

    @staticmethod
    def insert_batch_keyed(hgraph, batch, keys, num_connections, num_nodes_search_construction, seed=0, max_batch=0, batch_div=0,
                           expected_ef=0, expected_sem=SEM_OHNSW, metric=None):
        """insert_batch into an index that owns keys (hnsw_index_insert_keyed): the same graph, with keys[i] the key of row i of
        `batch`.  A key that is stored already, or twice in `keys`, refuses the call before anything is built; so does an index
        that has nodes and no keys (Hgraph.set_keys first; an EMPTY one starts its keys here).  -> the new ids."""
        X, xs = _rows(batch)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != hgraph.d):
            raise InvalidArgument("batch must be [m][d] with the index's d = %d" % hgraph.d)
        kk = _keys(keys)
        m = X.shape[0]
        if kk.size != m:
            raise InvalidArgument("%d keys for %d vectors" % (kk.size, m))
        n_old = hgraph.n
        p = _BuildParams(num_connections, num_nodes_search_construction, hgraph.metric if metric is None else int(metric), hgraph.id_base, seed, max_batch,
                         batch_div, expected_ef, expected_sem)
        _check(load().hnsw_index_insert_keyed(hgraph.handle, _ptr(X), m, max(xs, hgraph.d), _ptr(kk) if m else None, _C.byref(p)))
        if m == 0:
            return _np.arange(0, dtype=_np.int64)
        hgraph._append_vectors(X)
        hgraph._adopt(hgraph.info())
        return _np.arange(n_old + hgraph.id_base, n_old + m + hgraph.id_base, dtype=_np.int64)

    @staticmethod
    def upsert_batch_keyed(hgraph, batch, keys, num_connections, num_nodes_search_construction, seed=0, max_batch=0, batch_div=0,
                           expected_ef=0, expected_sem=SEM_OHNSW, metric=None):
        """Replace or add vectors by key in one all-or-nothing call (hnsw_index_upsert_keyed): row i of `batch` becomes the vector
        under keys[i], whether that key is stored or not.  The index afterwards is exactly what Hgraph.remove_keys(the stored ones
        among keys) followed by insert_batch_keyed(batch, keys) leaves, with one table swap and one epoch step instead of two; on
        any error it is exactly as before.  Two equal keys in the call are refused.  -> (replaced: bool [m], keys[i] was stored;
        new_id: int32 [n_old] as remove_batch returns it, id_base - 1 for a replaced node).  The rows of the call are the nodes
        n_old - replaced.sum() + i + id_base."""
        X, xs = _rows(batch)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != hgraph.d):
            raise InvalidArgument("batch must be [m][d] with the index's d = %d" % hgraph.d)
        kk = _keys(keys)
        m = X.shape[0]
        if kk.size != m:
            raise InvalidArgument("%d keys for %d vectors" % (kk.size, m))
        p = _BuildParams(num_connections, num_nodes_search_construction, hgraph.metric if metric is None else int(metric), hgraph.id_base, seed, max_batch,
                         batch_div, expected_ef, expected_sem)
        replaced = _np.zeros(m, _np.uint8)
        new_id = _np.empty(hgraph.n, _np.int32)
        _check(load().hnsw_index_upsert_keyed(hgraph.handle, _ptr(X) if m else None, _ptr(kk) if m else None, m, max(xs, hgraph.d), _C.byref(p),
                                              _ptr(replaced) if m else None, _ptr(new_id) if new_id.size else None))
        if m:
            hgraph._shrunk(new_id)
            hgraph._append_vectors(X)
        return replaced.astype(bool), new_id

    @staticmethod
    def update_batch(hgraph, ids, batch, num_connections, num_nodes_search_construction, seed=0, max_batch=0, batch_div=0,
                     expected_ef=0, expected_sem=SEM_OHNSW, metric=None):
        """upsert_batch_keyed for an index without keys (hnsw_index_update): the stored nodes `ids` (id_base-based, distinct) are
        replaced by the rows of `batch`: exactly remove_batch(ids) followed by insert_batch(batch), in one all-or-nothing call.
        An index with keys is refused (upsert_batch_keyed updates it).  -> new_id as remove_batch returns it."""
        X, xs = _rows(batch)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != hgraph.d):
            raise InvalidArgument("batch must be [m][d] with the index's d = %d" % hgraph.d)
        ids = _np.ascontiguousarray(ids, dtype=_np.int64).reshape(-1)
        m = X.shape[0]
        if ids.size != m:
            raise InvalidArgument("%d ids for %d vectors" % (ids.size, m))
        p = _BuildParams(num_connections, num_nodes_search_construction, hgraph.metric if metric is None else int(metric), hgraph.id_base, seed, max_batch,
                         batch_div, expected_ef, expected_sem)
        new_id = _np.empty(hgraph.n, _np.int32)
        _check(load().hnsw_index_update(hgraph.handle, _ptr(ids) if m else None, _ptr(X) if m else None, m, max(xs, hgraph.d), _C.byref(p),
                                        _ptr(new_id) if new_id.size else None))
        if m:
            hgraph._shrunk(new_id)
            hgraph._append_vectors(X)
        return new_id

    @staticmethod
    def remove_batch(hgraph, ids):
        """Hard deletion on the device (hnsw_index_remove): the stored nodes `ids` (id_base-based, distinct) leave the index, the
        others keep their order and are renumbered, and the graph is repaired by the three-pass rule the header defines.  -> the
        new id of every old node (np.int32 [n_old], id_base - 1 for a removed one).  Afterwards the Hgraph follows the device
        index as after insert_batch; the host vectors (if any) lose the removed rows."""
        ids = _np.ascontiguousarray(ids, dtype=_np.int64).reshape(-1)
        n_old = hgraph.n
        new_id = _np.empty(n_old, _np.int32)
        _check(load().hnsw_index_remove(hgraph.handle, _ptr(ids), len(ids), _ptr(new_id)))
        if len(ids) == 0:
            return new_id
        X = hgraph.vectors
        if X is not None:
            hgraph.vectors = _np.ascontiguousarray(_np.asarray(X, dtype=_np.float32)[new_id >= hgraph.id_base])
            hgraph.row_stride = hgraph.d
        hgraph._adopt(hgraph.info())
        return new_id

    @staticmethod
    def select_neighbours(hgraph, targets, candidates, num_neighbours, keep_all_if_few=False, degrees=None):
        """Batched Ohnsw.select_neighbours distance value queue num_neighbours (lib/ohnsw.ml:647-663):
        candidates = list of id lists (one per target); returns the kept ids per target in selection
        order.  keep_all_if_few=True gives Hnsw_algo.SelectNeighbours' shortcut (hnsw_algo.ml:596-599)."""
        T = _np.ascontiguousarray(targets, dtype=_np.float32)
        nb = T.shape[0]
        stride = max([len(c) for c in candidates] + [1])
        cand = _np.zeros((nb, stride), _np.int32)
        cnt = _np.zeros(nb, _np.int32)
        for i, c in enumerate(candidates):
            cand[i, :len(c)] = c
            cnt[i] = len(c)
        deg = None
        if degrees is not None:   # ~do_not_isolate:true (lib/hnsw_algo.ml:591-592)
            deg = _np.full((nb, stride), 2, _np.int32)
            for i, dg in enumerate(degrees):
                deg[i, :len(dg)] = dg
        out = _np.empty((nb, num_neighbours), _np.int32)
        ocnt = _np.empty(nb, _np.int32)
        _check(load().hnsw_select_neighbours_batch(hgraph.handle, _ptr(T), nb, T.shape[1], _ptr(cand), _ptr(cnt),
                                                   stride, num_neighbours, int(keep_all_if_few), _ptr(deg),
                                                   _ptr(out), _ptr(ocnt)))
        return [out[i, :ocnt[i]].tolist() for i in range(nb)]

    @staticmethod
    def distance_l2(hgraph, queries, ids):
        """Batched Ohnsw.distance_l2 (lib/ohnsw.ml:899): out[q][j] = distance(queries[q], value ids[q][j])."""
        Q = _np.ascontiguousarray(queries, dtype=_np.float32)
        I = _np.ascontiguousarray(ids, dtype=_np.int32)
        out = _np.empty(I.shape, _np.float32)
        _check(load().hnsw_distance_batch(hgraph.handle, _ptr(Q), Q.shape[0], Q.shape[1], _ptr(I),
                                          I.shape[1], _ptr(out)))
        return out


class Ba:
    """Hnsw.Ba = MakeBatch(EuclideanBa) (lib/hnsw.ml:729-778, 817-819): 1-based ids, separate
    ~num_neighbours_search (ef) and ~num_neighbours (k)."""

    @staticmethod
    def knn(hgraph, point, num_neighbours_search, num_neighbours, nearest_k_compat=False):
        """-> [{node; distance_to_target}] nearest first (lib/hnsw.ml:763-767).  nearest_k_compat=True
        reproduces Nearest.nearest_k (lib/hnsw.ml:522-525): the k FARTHEST of W when ef > k."""
        ids, dist = _search(hgraph, _np.asarray(point, _np.float32)[None, :], num_neighbours_search,
                            num_neighbours, FILL_BA, sem=SEM_FUNCTOR_NEAREST_K if nearest_k_compat else SEM_FUNCTOR)
        return [(int(i), float(d)) for i, d in zip(ids[0], dist[0]) if i >= hgraph.id_base]

    @staticmethod
    def knn_batch(hgraph, batch, num_neighbours_search, num_neighbours, nearest_k_compat=False):
        """-> distances [nq][k] fp32, +inf where fewer than k were found (lib/hnsw.ml:769-777)."""
        return _search(hgraph, batch, num_neighbours_search, num_neighbours, FILL_BA,
                       sem=SEM_FUNCTOR_NEAREST_K if nearest_k_compat else SEM_FUNCTOR)[1]

    @staticmethod
    def knn_batch_filtered(hgraph, batch, num_neighbours_search, num_neighbours, allow, counters=False):
        """knn_batch among the nodes `allow` names (see Ohnsw.knn_batch_filtered; the functor accept rule, 1-based ids in a
        1-based index, +inf / -1 where fewer than k nodes are allowed) -> (ids, distances), with counters (..., ndist, nhops, stage)."""
        return _search_filtered(hgraph, allow, batch, num_neighbours_search, num_neighbours, FILL_BA, counters, sem=SEM_FUNCTOR)

    @staticmethod
    def knn_batch_filtered_each(hgraph, batch, num_neighbours_search, num_neighbours, filters, which, counters=False):
        """knn_batch_filtered with one filter per query (see Ohnsw.knn_batch_filtered_each; the functor accept rule, +inf fill)."""
        return _search_filtered_each(hgraph, filters, which, batch, num_neighbours_search, num_neighbours, FILL_BA, counters, sem=SEM_FUNCTOR)

    @staticmethod
    def knn_batch_grouped(hgraph, batch, num_neighbours_search, num_neighbours, labels, filter=None, counters=False):
        """knn_batch over groups (see Ohnsw.knn_batch_grouped; the functor accept rule, 1-based ids in a 1-based index, +inf / -1
        where there are fewer than k groups) -> (ids, distances, labels), with counters (..., ndist, nhops, stage)."""
        return _search_grouped(hgraph, labels, batch, num_neighbours_search, num_neighbours, FILL_BA, counters, sem=SEM_FUNCTOR, flt=filter)

    @staticmethod
    def knn_batch_keyed(hgraph, batch, num_neighbours_search, num_neighbours, filter=None, counters=False, missing=MISSING_KEY):
        """knn_batch answered in the index's keys (see Ohnsw.knn_batch_keyed; the functor accept rule, +inf / `missing` where fewer
        than k were found) -> (keys, distances), with counters (..., ndist, nhops, stage)."""
        return _search_keyed(hgraph, batch, num_neighbours_search, num_neighbours, FILL_BA, counters, sem=SEM_FUNCTOR, flt=filter, missing=missing)

    @staticmethod
    def knn_batch_after(hgraph, batch, num_neighbours_search, num_neighbours, after=None, filter=None, counters=False):
        """knn_batch's results that come after a cursor (see Ohnsw.knn_batch_after; the functor accept rule, +inf where a row is
        exhausted) -> (ids, distances, next)."""
        return _search_after(hgraph, batch, after, num_neighbours_search, num_neighbours, FILL_BA, counters, sem=SEM_FUNCTOR, flt=filter)

    @staticmethod
    def knn_batch_diverse(hgraph, batch, num_neighbours_search, num_neighbours, pool, lam=0.5, filter=None, counters=False):
        """knn_batch's results diversified (see Ohnsw.knn_batch_diverse; the functor accept rule, +inf where a row is short)
        -> (ids, distances, div)"""
        return _search_diverse(hgraph, batch, num_neighbours_search, num_neighbours, pool, lam, FILL_BA, counters, sem=SEM_FUNCTOR, flt=filter)

    @staticmethod
    def knn_batch_by_id(hgraph, ids, num_neighbours_search, num_neighbours, exclude_self=True, counters=False):
        """knn_batch with the stored vectors of the nodes `ids` as the queries (see Ohnsw.knn_batch_by_id; the functor accept rule,
        1-based ids in a 1-based index, +inf / -1 where fewer than k were found) -> (ids, distances), with counters (..., ndist, nhops)."""
        return _search_by_id(hgraph, ids, num_neighbours_search, num_neighbours, FILL_BA, exclude_self, counters, sem=SEM_FUNCTOR)

    @staticmethod
    def knn_batch_by_key(hgraph, keys, num_neighbours_search, num_neighbours, exclude_self=True, counters=False, missing=MISSING_KEY):
        """knn_batch_by_id for the nodes stored under `keys`, answered in keys (see Ohnsw.knn_batch_by_key; the functor accept rule)
        -> (keys, distances), with counters (..., ndist, nhops)."""
        return _search_by_key(hgraph, keys, num_neighbours_search, num_neighbours, FILL_BA, exclude_self, counters, sem=SEM_FUNCTOR, missing=missing)

    @staticmethod
    def range_search(hgraph, batch, num_neighbours_search, radius, counters=False, filter=None):
        """Ohnsw.range_search under the functor accept rule (1-based ids in a Hnsw.Ba-style index), the ladder starting at
        ~num_neighbours_search; filter: as Ohnsw.range_search"""
        return _range_search(hgraph, batch, radius, num_neighbours_search, SEM_FUNCTOR, counters, filter=filter)

    @staticmethod
    def search(hgraph, layer, start_nodes, targets, size_nearest):
        """Batched Hnsw_algo.Search.search hgraph layer visited ~start_nodes target ~size_nearest
        (lib/hnsw_algo.ml:350-391) -> Nearest.t per target as [(node, distance)] nearest first."""
        return Ohnsw.search_k(hgraph, layer, start_nodes, targets, size_nearest, sem=SEM_FUNCTOR)

    @staticmethod
    def search_one(hgraph, layer, start, targets):
        """Batched Hnsw_algo.Search.search_one (lib/hnsw_algo.ml:393-437) -> (node, distance) arrays
        (the value_distance it returns)."""
        return Ohnsw.search_one(hgraph, layer, start, targets, with_distance=True)


class MultiHgraph(_Owner):
    """One host process, several GPUs: the flattened graph replicated on every listed
    device; knn_batch_bigarray / knn_batch split the batch into contiguous shards, one device each,
    and return the same arrays as the single-device calls."""
    _slot, _destroy, _gone = "_h", "hnsw_multi_destroy", "multi index already released"

    def __init__(self, hgraph, devices):
        self.hgraph = hgraph
        self.devices = [int(x) for x in devices]
        d, _keep = hgraph._desc()
        dev = _np.asarray(self.devices, _np.int32)
        h = _C.c_void_p()
        _check(load().hnsw_multi_create(_C.byref(d), _ptr(dev), len(dev), _C.byref(h)))
        self._h = h
        self._last = None            # (nq, k) of the last search_device, for copy_result

    def num_replicas(self):
        c = _C.c_int32(0)
        _check(load().hnsw_multi_num_replicas(self._h, _C.byref(c)))
        return c.value

    def set_option(self, name, value):
        """hnsw_index_set_option on every replica's handle (hnsw_multi_replica): the options that change results ("half_rows",
        "sq8_rows", "refine") reach the sharded search this way"""
        for g in range(self.num_replicas()):
            h = _C.c_void_p()
            _check(load().hnsw_multi_replica(self._h, g, _C.byref(h)))
            _check(load().hnsw_index_set_option(h, name.encode(), int(value)))

    def _search(self, batch, ef, k, fill, sem, counters=False):
        Q, qs, nq = _batch(self.hgraph.d, batch)
        ids, dist = _out_pair(nq, k, None)
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_multi_search_batch(self._h, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist), _ptr(nd), _ptr(nh)))
        return (ids, dist, nd, nh) if counters else (ids, dist)

    def knn_batch_bigarray(self, k, batch, ef=None, counters=False):
        """Ohnsw.knn_batch_bigarray over all replicas (lib/ohnsw.ml:877-897)."""
        return self._search(batch, k if ef is None else ef, k, FILL_OHNSW, SEM_OHNSW, counters)

    def search_device(self, batch, ef, k, fill=FILL_OHNSW, sem=SEM_OHNSW):
        """hnsw_multi_search_batch_device: sharded search + RCCL all-gather, results left on the devices.
        -> (d_ids, d_dist): per-device pointers (ints) to each device's full [nq][k] table."""
        Q, qs, nq = _batch(self.hgraph.d, batch, 1)
        G = len(self.devices)
        pi = (_C.c_void_p * G)()
        pd = (_C.c_void_p * G)()
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_multi_search_batch_device(self._h, _ptr(Q), nq, qs, _C.byref(p), pi, pd))
        self._last = (nq, k)
        return [int(x or 0) for x in pi], [int(x or 0) for x in pd]

    def debug_counters(self):
        """hnsw_multi_debug_counters -> {allgather, broadcast, peer_copies, repaired_shards}"""
        out = (_C.c_int64 * 4)()
        _check(load().hnsw_multi_debug_counters(self._h, out))
        return dict(zip(("allgather", "broadcast", "peer_copies", "repaired_shards"), [int(x) for x in out]))

    def copy_result(self, g):
        """device g's copy of the last search_device result -> (ids, dist) host arrays"""
        ids, dist = _out_pair(*self._last, None)
        _check(load().hnsw_multi_copy_result(self._h, int(g), _ptr(ids), _ptr(dist)))
        return ids, dist

    def knn_batch(self, batch, num_neighbours_search, num_neighbours):
        """Hnsw.Ba.knn_batch over all replicas (lib/hnsw.ml:769-777)."""
        return self._search(batch, num_neighbours_search, num_neighbours, FILL_BA, SEM_FUNCTOR)[1]



def merge_lists(ids, dist, first_row, k_out, id_base=0, fill=FILL_OHNSW, device=0):
    """hnsw_merge_lists: the merge of per-shard result lists as an operator of its own (no index needed).  ids int32 and dist float32
    [n_lists][nq][k_in]: each list ascending under (distance, id) with its padding (id < id_base) at the end; first_row [n_lists],
    non-decreasing.  -> (ids int64 [nq][k_out], distances float32 [nq][k_out]): the first k_out real entries of the union under
    (distance, first_row[list] + id), the rest filled (id -1; NaN, FILL_BA: +inf)."""
    I = _np.ascontiguousarray(ids, _np.int32)
    D = _np.ascontiguousarray(dist, _np.float32)
    F = _np.ascontiguousarray(first_row, _np.int64).reshape(-1)
    if I.ndim != 3 or D.shape != I.shape or F.shape != (I.shape[0],):
        raise InvalidArgument("ids and dist must be [n_lists][nq][k_in], first_row [n_lists]")
    n_lists, nq, k_in = I.shape
    out_ids = _np.empty((nq, max(int(k_out), 0)), _np.int64)
    out_dist = _np.empty((nq, max(int(k_out), 0)), _np.float32)
    _check(load().hnsw_merge_lists(int(device), _ptr(I), _ptr(D), _ptr(F), n_lists, nq, k_in, int(k_out), int(id_base), int(fill),
                                   _ptr(out_ids), _ptr(out_dist)))
    return out_ids, out_dist


class ShardedRangeResult(RangeResult):
    """What a sharded range call and merge_segments return (hnsw_sharded_range_result): as RangeResult, with int64 global ids, on
    the first device of the sharded index; it outlives that index."""
    _prefix, _id = "hnsw_sharded_range_result_", _np.int64
    _destroy = _prefix + "destroy"


def merge_segments(lims, ids, dist, first_row, id_base=0, device=0, keep=False):
    """hnsw_merge_segments: the merge of per-list range results as an operator of its own (no index needed).  lims[g] int64
    [nq + 1] (from 0, non-decreasing), ids[g] int32 and dist[g] float32 [lims[g][nq]]: each segment ascending under (distance, id);
    first_row [n_lists], non-decreasing.  -> (lims, ids int64, distances): per query the union of its segments under (distance,
    first_row[list] + id), the same global id in two lists: the lower list first; keep: the ShardedRangeResult."""
    L = [_np.ascontiguousarray(x, _np.int64).reshape(-1) for x in lims]
    I = [_np.ascontiguousarray(x, _np.int32).reshape(-1) for x in ids]
    D = [_np.ascontiguousarray(x, _np.float32).reshape(-1) for x in dist]
    F = _np.ascontiguousarray(first_row, _np.int64).reshape(-1)
    n = len(L)
    if len(I) != n or len(D) != n or len(F) != n or any(len(x) != len(L[0]) or len(x) < 1 for x in L):
        raise InvalidArgument("lims, ids, dist and first_row must list the same lists; every lims has nq + 1 entries")
    if any(len(I[g]) != len(D[g]) or (len(I[g]) != L[g][-1]) for g in range(n)):
        raise InvalidArgument("ids[g] and dist[g] must have lims[g][nq] entries")

    def table(arrays):
        return (_C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrays])

    r = _C.c_void_p()
    _check(load().hnsw_merge_segments(int(device), n, (len(L[0]) - 1) if n else 0, table(L), table(I), table(D), _ptr(F) if n else None,
                                      int(id_base), _C.byref(r)))
    return ShardedRangeResult(r)._take(False, keep)


class ShardedFilter(_Owner):
    """An allow-mask over the GLOBAL rows of one ShardedHgraph (hnsw_sharded_filter): one ordinary filter per shard, each on its
    shard's device; see ShardedHgraph.filter.  Release it before its index."""
    _slot, _destroy, _gone = "_f", "hnsw_sharded_filter_destroy", "filter already released"

    def __init__(self, sharded, allow):
        self._f = None
        bits = pack_allow(allow, sharded.n, sharded.id_base)
        f = _C.c_void_p()
        _check(load().hnsw_sharded_filter_create(sharded.handle, _ptr(bits) if len(bits) else None, sharded.n, _C.byref(f)))
        self._f, self._s, self.n = f, sharded, sharded.n

    def count(self):
        """hnsw_sharded_filter_count: the allowed rows, summed over the shards"""
        c = _C.c_int64(0)
        _check(load().hnsw_sharded_filter_count(self.handle, _C.byref(c)))
        return c.value

    def part_bits(self, g):
        """shard g's part as its device holds it (hnsw_sharded_filter_part, hnsw_filter_bits): uint32 [ceil(n_g / 32)], bit v = the
        shard's local node v"""
        p = _C.c_void_p()
        _check(load().hnsw_sharded_filter_part(self.handle, int(g), _C.byref(p)))
        n_g = self._s.shard(g)[0].info().n
        out = _np.zeros((n_g + 31) // 32, _np.uint32)
        _check(load().hnsw_filter_bits(p, _ptr(out) if len(out) else _C.byref(_C.c_uint32())))
        return out



class ShardedHgraph(_Owner):
    """One data set PARTITIONED over several GPUs (hnsw_sharded): shard g holds the rows [first_row(g), first_row(g + 1)) with a graph
    of its own on devices[g], every query visits all shards, and the per-shard answers are merged on devices[0] under (distance,
    global id).  Global ids are int64: first_row(g) + local node + id_base.  A device may be listed several times.  Capacity, where
    MultiHgraph (the index replicated, the batch split) is rate."""
    _slot, _destroy, _gone = "_h", "hnsw_sharded_destroy", "sharded index already released"

    def __init__(self, handle, devices):
        self._h, self.devices = handle, [int(x) for x in devices]
        self.n, self.d, self.metric, self.id_base, _ = self.info()

    @staticmethod
    def _devices(devices):
        dev = _np.ascontiguousarray(devices, _np.int32).reshape(-1)
        return dev, (_ptr(dev) if len(dev) else None)

    @classmethod
    def build(cls, batch, num_connections, num_nodes_search_construction, devices, seed=0, metric=METRIC_L2, id_base=0, max_batch=0,
              batch_div=0, expected_ef=0, expected_sem=SEM_OHNSW):
        """hnsw_sharded_build: shard g = Ohnsw.build_batch_bigarray of the rows [floor(n g / G), floor(n (g + 1) / G)) on devices[g]
        with seed + g, built one after another"""
        X, xs = _rows(batch)
        if X.ndim != 2:
            raise InvalidArgument("batch must be [n][d]")
        p = _BuildParams(num_connections, num_nodes_search_construction, metric, id_base, seed, max_batch, batch_div, expected_ef, expected_sem)
        dev, pdev = cls._devices(devices)
        h = _C.c_void_p()
        _check(load().hnsw_sharded_build(_ptr(X), X.shape[0], X.shape[1], max(xs, X.shape[1]), _C.byref(p), pdev, len(dev), _C.byref(h)))
        return cls(h, dev)

    @classmethod
    def create(cls, hgraphs, devices):
        """hnsw_sharded_create: adopt graphs built elsewhere, one Hgraph (host copy, LOCAL ids) per shard; the shards need not be
        equal in size but must agree on d, metric and id_base"""
        hgraphs = list(hgraphs)
        keep = [hg._desc() for hg in hgraphs]
        table = (_C.c_void_p * max(len(keep), 1))(*[_C.addressof(d) for d, _ in keep])
        dev, pdev = cls._devices(devices)
        if len(dev) != len(hgraphs):
            raise InvalidArgument("one device per shard")
        h = _C.c_void_p()
        _check(load().hnsw_sharded_create(table, pdev, len(dev), _C.byref(h)))
        return cls(h, dev)

    @classmethod
    def load(cls, paths, devices):
        """hnsw_sharded_load: one index file per shard (what save() wrote)"""
        paths = [str(p).encode() for p in paths]
        table = (_C.c_char_p * max(len(paths), 1))(*paths)
        dev, pdev = cls._devices(devices)
        if len(dev) != len(paths):
            raise InvalidArgument("one device per path")
        h = _C.c_void_p()
        _check(load().hnsw_sharded_load(table, pdev, len(dev), _C.byref(h)))
        return cls(h, dev)

    def num_shards(self):
        c = _C.c_int32(0)
        _check(load().hnsw_sharded_num_shards(self.handle, _C.byref(c)))
        return c.value

    def shard(self, g):
        """hnsw_sharded_shard -> (Hgraph, first_row): shard g's index, BORROWED (valid until this object's release(); its own
        release() only forgets the handle), for the read-only calls: searches, filters, range calls, stats, export, save"""
        h, lo = _C.c_void_p(), _C.c_int64(0)
        _check(load().hnsw_sharded_shard(self.handle, int(g), _C.byref(h), _C.byref(lo)))
        hg = Hgraph._from_handle(h, self.devices[int(g)])
        hg._owner = self
        return hg, lo.value

    def save(self, paths):
        """hnsw_index_save of every shard, in order, into `paths` (one per shard): the files load() reads"""
        paths = list(paths)
        if len(paths) != self.num_shards():
            raise InvalidArgument("one path per shard")
        for g, p in enumerate(paths):
            self.shard(g)[0].save(p)

    def info(self):
        """hnsw_sharded_get_info -> (n, d, metric, id_base, device_bytes): the shards' rows and device bytes summed"""
        n, b = _C.c_int64(0), _C.c_int64(0)
        d, m, ib = _C.c_int32(0), _C.c_int32(0), _C.c_int32(0)
        _check(load().hnsw_sharded_get_info(self.handle, _C.byref(n), _C.byref(d), _C.byref(m), _C.byref(ib), _C.byref(b)))
        return n.value, d.value, m.value, ib.value, b.value

    def set_option(self, name, value):
        """hnsw_sharded_set_option: hnsw_index_set_option on every shard; a refusal leaves every shard as it was"""
        _check(load().hnsw_sharded_set_option(self.handle, name.encode(), int(value)))

    def knn_batch(self, batch, ef, k, fill=FILL_OHNSW, sem=SEM_OHNSW, counters=False):
        """hnsw_sharded_search_batch -> (ids int64 [nq][k], distances [nq][k]), with counters (ids, distances, ndist, nhops -- sums
        over the shards): the first k under (distance, global id) of the shards' own knn rows for (ef, k)"""
        Q, qs, nq = _batch(self.d, batch)
        ids, dist = _np.empty((nq, max(k, 0)), _np.int64), _np.empty((nq, max(k, 0)), _np.float32)
        nd = _np.zeros(nq, _np.uint32) if counters else None
        nh = _np.zeros(nq, _np.uint32) if counters else None
        p = _SearchParams(ef, k, fill, sem)
        _check(load().hnsw_sharded_search_batch(self.handle, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist), _ptr(nd), _ptr(nh)))
        return (ids, dist, nd, nh) if counters else (ids, dist)

    def brute_force_knn(self, k, batch, fill=FILL_OHNSW):
        """hnsw_sharded_brute_force_batch -> (ids int64 [nq][k], distances [nq][k]): the exact k nearest of all rows, the
        distance bits of Ohnsw.brute_force_knn over one index holding them all"""
        Q, qs, nq = _batch(self.d, batch)
        ids, dist = _np.empty((nq, max(int(k), 0)), _np.int64), _np.empty((nq, max(int(k), 0)), _np.float32)
        _check(load().hnsw_sharded_brute_force_batch(self.handle, _ptr(Q), nq, qs, int(k), fill, _ptr(ids), _ptr(dist)))
        return ids, dist

    def filter(self, allow):
        """hnsw_sharded_filter_create: allow = a boolean array over the n GLOBAL rows, or an array of global ids (id_base-based)
        -> ShardedFilter, cut into one filter per shard"""
        return ShardedFilter(self, allow)

    def _filter(self, flt):
        """(a ShardedFilter, whether it was made for this call) from a ShardedFilter or what filter() takes"""
        return (flt, False) if isinstance(flt, ShardedFilter) else (ShardedFilter(self, flt), True)

    def knn_batch_filtered(self, batch, ef, k, filter, fill=FILL_OHNSW, sem=SEM_OHNSW, counters=False):
        """hnsw_sharded_search_batch_filtered -> (ids int64 [nq][k], distances [nq][k]), with counters (ids, distances, ndist, nhops
        -- sums over the shards --, stage -- the unsigned maximum over the shards): the first k under (distance, global id) of the
        shards' own filtered rows"""
        f, own = self._filter(filter)
        try:
            Q, qs, nq = _batch(self.d, batch)
            ids, dist = _np.empty((nq, max(k, 0)), _np.int64), _np.empty((nq, max(k, 0)), _np.float32)
            cnt = [_np.zeros(nq, _np.uint32) for _ in range(3)] if counters else [None] * 3
            p = _SearchParams(ef, k, fill, sem)
            _check(load().hnsw_sharded_search_batch_filtered(self.handle, f.handle, _ptr(Q), nq, qs, _C.byref(p), _ptr(ids), _ptr(dist),
                                                             _ptr(cnt[0]), _ptr(cnt[1]), _ptr(cnt[2])))
        finally:
            if own:
                f.release()
        return (ids, dist) + tuple(cnt) if counters else (ids, dist)

    def _range(self, batch, radius, ef, sem, filter, counters, keep):
        Q, qs, nq = _batch(self.d, batch)
        f, own = (None, False) if filter is None else self._filter(filter)
        r = _C.c_void_p()
        try:
            fh = None if f is None else f.handle
            if ef is None:
                _check(load().hnsw_sharded_range_brute_force_batch(self.handle, fh, _ptr(Q), nq, qs, float(radius), _C.byref(r)))
            else:
                p = _RangeParams(float(radius), int(ef), sem)
                _check(load().hnsw_sharded_range_search_batch(self.handle, fh, _ptr(Q), nq, qs, _C.byref(p), _C.byref(r)))
        finally:
            if own:
                f.release()
        return ShardedRangeResult(r)._take(counters, keep)

    def range_search(self, batch, radius, ef=64, sem=SEM_OHNSW, filter=None, counters=False, keep=False):
        """hnsw_sharded_range_search_batch -> (lims int64 [nq + 1], ids int64, distances), with counters also (ndist, nhops, stage):
        per query the union of the shards' own range_search segments under (distance, global id); filter: a ShardedFilter or what
        filter() takes; keep: the ShardedRangeResult instead"""
        return self._range(batch, radius, ef, sem, filter, counters, keep)

    def brute_force_range(self, batch, radius, filter=None, counters=False, keep=False):
        """hnsw_sharded_range_brute_force_batch: the exact form -- the set Ohnsw.brute_force_range gives over one index of all rows"""
        return self._range(batch, radius, None, SEM_OHNSW, filter, counters, keep)

