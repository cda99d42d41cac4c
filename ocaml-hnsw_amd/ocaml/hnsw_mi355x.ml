(* hnsw_mi355x.ml -- OCaml side of the drop-in: ctypes-foreign binding of libhnsw_mi355x.so
   (include/hnsw_mi355x.h) plus the flatten shims that turn the reference's own graph containers
   into the tables the C ABI takes.

   SOURCE ONLY in this repository: the build image has no OCaml toolchain (no ocaml / opam / dune),
   so this file is not compiled or tested here; the identical ABI is exercised from Python ctypes
   (tests/) and C++ (host/hnsw_front.hpp).  It is written against the reference's modules as they
   are: Ohnsw (lib/ohnsw.ml) and Hnsw.Ba (lib/hnsw.ml:817-819).

   What stays OCaml: the graph builder (Ohnsw.build_batch_bigarray, Hnsw.Ba.build) and every
   signature.  What moves: the bodies of knn / knn_batch*, i.e. the search_one + search_k loops. *)
open Ctypes
open Foreign

let lib = Dl.dlopen ~filename:"libhnsw_mi355x.so" ~flags:[ Dl.RTLD_NOW ]

(* ---- C structs ---------------------------------------------------------------------------- *)
type layer_desc
let layer_desc : layer_desc structure typ = structure "hnsw_layer_desc"
let ld_n_nodes = field layer_desc "n_nodes" int64_t
let ld_nodes = field layer_desc "nodes" (ptr int64_t)
let ld_deg = field layer_desc "deg" (ptr int32_t)
let ld_nbr = field layer_desc "nbr" (ptr int32_t)
let () = seal layer_desc

type index_desc
let index_desc : index_desc structure typ = structure "hnsw_index_desc"
let d_vectors = field index_desc "vectors" (ptr float)
let d_n = field index_desc "n" int64_t
let d_d = field index_desc "d" int32_t
let d_row_stride = field index_desc "row_stride" int64_t
let d_metric = field index_desc "metric" int32_t
let d_id_base = field index_desc "id_base" int32_t
let d_max_degree0 = field index_desc "max_degree0" int32_t
let d_max_degree = field index_desc "max_degree" int32_t
let d_max_layer = field index_desc "max_layer" int32_t
let d_entry_point = field index_desc "entry_point" int64_t
let d_deg0 = field index_desc "deg0" (ptr int32_t)
let d_nbr0 = field index_desc "nbr0" (ptr int32_t)
let d_upper = field index_desc "upper" (ptr layer_desc)
let d_expected_ef = field index_desc "expected_ef" int32_t
let d_expected_semantics = field index_desc "expected_semantics" int32_t
let () = seal index_desc

type search_params
let search_params : search_params structure typ = structure "hnsw_search_params"
let p_ef = field search_params "ef" int32_t
let p_k = field search_params "k" int32_t
let p_fill = field search_params "fill" int32_t
let p_semantics = field search_params "semantics" int32_t
let () = seal search_params

type index = unit ptr
let index : index typ = ptr void

(* ---- entry points (the OCaml 4.x runtime lock is released around the blocking calls) -------- *)
let hnsw_last_error = foreign ~from:lib "hnsw_last_error" (void @-> returning string)
let hnsw_index_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_create"
    (ptr index_desc @-> int32_t @-> ptr index @-> returning int32_t)
let hnsw_index_destroy = foreign ~from:lib "hnsw_index_destroy" (index @-> returning int32_t)
let hnsw_search_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float
     @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_search_layer_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_layer_batch"
    (index @-> int32_t @-> ptr float @-> int64_t @-> int64_t @-> ptr int64_t @-> int32_t
     @-> ptr search_params @-> ptr int32_t @-> ptr float @-> ptr int32_t @-> ptr uint32_t
     @-> ptr uint32_t @-> returning int32_t)
let hnsw_search_one_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_one_batch"
    (index @-> int32_t @-> ptr float @-> int64_t @-> int64_t @-> ptr int64_t @-> ptr int64_t
     @-> ptr float @-> returning int32_t)
let hnsw_index_set_option =
  foreign ~from:lib "hnsw_index_set_option" (index @-> string @-> int64_t @-> returning int32_t)
(* bytes of one vector as the knn searches read it: d when the library serves byte-valued data (SIFT: float32
   values that are all integers 0..255) from its lossless byte copy of the rows, 4 d otherwise.  Nothing to do on
   this side: the copy is built by hnsw_index_create itself and is invisible to knn_batch* (same results, bit for
   bit); `hnsw_index_set_option idx "byte_rows" 0L` reads the float32 rows again.  2 d after
   `hnsw_index_set_option idx "half_rows" 1L` (the vectors rounded to fp16: results change, see the C header). *)
let hnsw_index_row_bytes =
  foreign ~from:lib "hnsw_index_row_bytes" (index @-> ptr int64_t @-> returning int32_t)
(* the sq8 copy (`hnsw_index_set_option idx "sq8_rows" 1L`: the knn searches walk 8-bit codes of the vectors and answer from the
   float32 rows, see the C header): its parameters lo and scale (x ~ lo + scale * code), and its codes, [n][d] bytes *)
let hnsw_index_sq8_params =
  foreign ~from:lib "hnsw_index_sq8_params" (index @-> ptr float @-> ptr float @-> returning int32_t)
let hnsw_index_sq8_codes =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_sq8_codes" (index @-> ptr void @-> returning int32_t)
(* the per-dimension sq8 copy (`hnsw_index_set_option idx "sq8_dim_rows" 1L`: one affine map per dimension, a weighted L2 walk, see
   the C header): its parameters lo and scale, [d] floats each (x_i ~ lo_i + scale_i * code_i), and its codes, [n][d] bytes *)
let hnsw_index_sq8_dim_params =
  foreign ~from:lib "hnsw_index_sq8_dim_params" (index @-> ptr float @-> ptr float @-> returning int32_t)
let hnsw_index_sq8_dim_codes =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_sq8_dim_codes" (index @-> ptr void @-> returning int32_t)
(* the 1-bit copy (`hnsw_index_set_option idx "bit_rows" 1L` -- thresholds at the column means -- or `2L` -- at zero: a Hamming walk,
   re-ranked over the float32 rows, see the C header): its thresholds, [d] floats, and its codes, [n][ceil(d/32)] uint32 words *)
let hnsw_index_bit_params =
  foreign ~from:lib "hnsw_index_bit_params" (index @-> ptr float @-> returning int32_t)
let hnsw_index_bit_codes =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_bit_codes" (index @-> ptr void @-> returning int32_t)
(* the 4-bit query codes of option "bit_query_bits" (`hnsw_index_set_option idx "bit_query_bits" 4L`: the walk over the bit rows keeps
   the query at 4 bits a dimension, see the C header): [nq][d] int8 in -7..7 for nq host queries *)
let hnsw_index_bit_query_codes =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_bit_query_codes"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr void @-> returning int32_t)
(* cosine distance (metric_cosine below; the twin contract of the C header): the normaliser N as an operator of its own, and the
   float32 rows an index holds -- for a cosine index N(X), not the vectors it was handed *)
let hnsw_normalise_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_normalise_batch"
    (int32_t @-> ptr float @-> int64_t @-> int32_t @-> int64_t @-> ptr float @-> int64_t @-> ptr float @-> returning int32_t)
let hnsw_index_get_rows =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_get_rows"
    (index @-> ptr int64_t @-> int64_t @-> ptr float @-> int64_t @-> returning int32_t)
let hnsw_index_kernel_times =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_kernel_times"
    (index @-> ptr double @-> ptr double @-> ptr int32_t @-> returning int32_t)
type request = unit ptr
let request : request typ = ptr void
let hnsw_search_submit =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_submit"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr request @-> returning int32_t)
let hnsw_search_wait =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_wait"
    (request @-> ptr int32_t @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
type multi = unit ptr
let multi : multi typ = ptr void
let hnsw_multi_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_multi_create"
    (ptr index_desc @-> ptr int32_t @-> int32_t @-> ptr multi @-> returning int32_t)
let hnsw_multi_destroy = foreign ~from:lib "hnsw_multi_destroy" (multi @-> returning int32_t)
let hnsw_multi_search_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_multi_search_batch"
    (multi @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float
     @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
(* sharded search + RCCL all-gather, results left on every device: d_ids / d_dist are arrays of
   n_devices device pointers written by the library *)
let hnsw_multi_search_batch_device =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_multi_search_batch_device"
    (multi @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr (ptr int32_t) @-> ptr (ptr float)
     @-> returning int32_t)
let hnsw_multi_debug_counters =
  foreign ~from:lib "hnsw_multi_debug_counters" (multi @-> ptr int64_t @-> returning int32_t)
let hnsw_multi_copy_result =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_multi_copy_result"
    (multi @-> int32_t @-> ptr int32_t @-> ptr float @-> returning int32_t)

(* the rest of include/hnsw_mi355x.h: single query, gathered distances, select_neighbours, the device builder,
   save / load, per-layer statistics, host-array registration *)
let hnsw_knn =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_knn"
    (index @-> ptr float @-> ptr search_params @-> ptr int32_t @-> ptr float @-> ptr int32_t @-> returning int32_t)
let hnsw_distance_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_distance_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> ptr float @-> returning int32_t)
let hnsw_brute_force_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_brute_force_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float @-> returning int32_t)
let hnsw_rerank_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_rerank_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float
     @-> returning int32_t)
(* filtered search (see the C header): an allow-mask over the nodes, uploaded once, and the batch search among the nodes it names *)
type filter_handle = unit ptr
let filter_handle : filter_handle typ = ptr void
let hnsw_filter_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_filter_create"
    (index @-> ptr uint32_t @-> int64_t @-> ptr filter_handle @-> returning int32_t)
let hnsw_filter_destroy = foreign ~from:lib "hnsw_filter_destroy" (filter_handle @-> returning int32_t)
let hnsw_filter_count = foreign ~from:lib "hnsw_filter_count" (filter_handle @-> ptr int64_t @-> returning int32_t)
let hnsw_search_batch_filtered =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_filtered"
    (index @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float
     @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
(* ... with one filter per query; the filters of n_labels labels from one label per node; a filter's mask back on the host *)
let hnsw_search_batch_filtered_each =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_filtered_each"
    (index @-> ptr filter_handle @-> int32_t @-> ptr int32_t @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params
     @-> ptr int32_t @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_filter_create_by_label =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_filter_create_by_label"
    (index @-> ptr int32_t @-> int64_t @-> int32_t @-> ptr filter_handle @-> returning int32_t)
let hnsw_filter_bits = foreign ~from:lib "hnsw_filter_bits" (filter_handle @-> ptr uint32_t @-> returning int32_t)
(* range search (see the C header): every node within a radius of the query; the result is an object that owns its device buffers *)
type range_params
let range_params : range_params structure typ = structure "hnsw_range_params"
let r_radius = field range_params "radius" float
let r_ef = field range_params "ef" int32_t
let r_semantics = field range_params "semantics" int32_t
let () = seal range_params
type range_handle = unit ptr
let range_handle : range_handle typ = ptr void
let hnsw_range_search_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_range_search_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr range_params @-> ptr range_handle @-> returning int32_t)
let hnsw_range_brute_force_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_range_brute_force_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> float @-> ptr range_handle @-> returning int32_t)
(* grouped search (see the C header): one label per node, uploaded once, and the k nearest groups, one node per label *)
type labels_handle = unit ptr
let labels_handle : labels_handle typ = ptr void
let hnsw_labels_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_labels_create"
    (index @-> ptr int32_t @-> int64_t @-> int32_t @-> ptr labels_handle @-> returning int32_t)
let hnsw_labels_destroy = foreign ~from:lib "hnsw_labels_destroy" (labels_handle @-> returning int32_t)
let hnsw_labels_info =
  foreign ~from:lib "hnsw_labels_info" (labels_handle @-> ptr int32_t @-> ptr int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_labels_get = foreign ~from:lib "hnsw_labels_get" (labels_handle @-> ptr int32_t @-> returning int32_t)
let hnsw_search_batch_grouped =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_grouped"
    (index @-> labels_handle @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t
     @-> ptr float @-> ptr int32_t @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_brute_force_batch_grouped =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_brute_force_batch_grouped"
    (index @-> labels_handle @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> ptr int32_t
     @-> ptr float @-> ptr int32_t @-> returning int32_t)
(* ... under an allow-mask: each segment is the unfiltered one with the nodes the filter does not allow left out *)
let hnsw_range_search_batch_filtered =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_range_search_batch_filtered"
    (index @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr range_params @-> ptr range_handle @-> returning int32_t)
let hnsw_range_brute_force_batch_filtered =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_range_brute_force_batch_filtered"
    (index @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> float @-> ptr range_handle @-> returning int32_t)
let hnsw_range_result_size =
  foreign ~from:lib "hnsw_range_result_size" (range_handle @-> ptr int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_range_result_fetch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_range_result_fetch"
    (range_handle @-> ptr int64_t @-> ptr int32_t @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t
     @-> returning int32_t)
let hnsw_range_result_device =
  foreign ~from:lib "hnsw_range_result_device"
    (range_handle @-> ptr (ptr int64_t) @-> ptr (ptr int32_t) @-> ptr (ptr float) @-> returning int32_t)
let hnsw_range_result_destroy = foreign ~from:lib "hnsw_range_result_destroy" (range_handle @-> returning int32_t)
let hnsw_select_neighbours_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_select_neighbours_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> ptr int32_t @-> int32_t @-> int32_t @-> int32_t
     @-> ptr int32_t @-> ptr int32_t @-> ptr int32_t @-> returning int32_t)
type build_params
let build_params : build_params structure typ = structure "hnsw_build_params"
let b_num_connections = field build_params "num_connections" int32_t
let b_efc = field build_params "num_nodes_search_construction" int32_t
let b_metric = field build_params "metric" int32_t
let b_id_base = field build_params "id_base" int32_t
let b_seed = field build_params "seed" uint64_t
let b_max_batch = field build_params "max_batch" int32_t
let b_batch_div = field build_params "batch_div" int32_t
let b_expected_ef = field build_params "expected_ef" int32_t
let b_expected_semantics = field build_params "expected_semantics" int32_t
let () = seal build_params
let hnsw_build =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_build"
    (ptr float @-> int64_t @-> int32_t @-> int64_t @-> ptr build_params @-> int32_t @-> ptr index @-> returning int32_t)
let hnsw_index_insert =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_insert"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr build_params @-> returning int32_t)
let hnsw_index_remove =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_remove"
    (index @-> ptr int64_t @-> int64_t @-> ptr int32_t @-> returning int32_t)
(* soft deletion owned by the index (see the C header): mark, search around, compact *)
let hnsw_index_mark_deleted =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_mark_deleted" (index @-> ptr int64_t @-> int64_t @-> returning int32_t)
let hnsw_index_unmark_deleted =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_unmark_deleted" (index @-> ptr int64_t @-> int64_t @-> returning int32_t)
(* keys the index owns (see the C header): one caller-chosen int64 per stored node, moved with the nodes *)
let hnsw_index_set_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_set_keys" (index @-> ptr int64_t @-> int64_t @-> returning int32_t)
let hnsw_index_clear_keys = foreign ~from:lib "hnsw_index_clear_keys" (index @-> returning int32_t)
let hnsw_index_keys_info = foreign ~from:lib "hnsw_index_keys_info" (index @-> ptr int32_t @-> ptr int64_t @-> returning int32_t)
let hnsw_index_keys_of =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_keys_of"
    (index @-> ptr int32_t @-> int64_t @-> int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_index_keys_of_device =
  foreign ~from:lib "hnsw_index_keys_of_device"
    (index @-> ptr int32_t @-> int64_t @-> int64_t @-> ptr int64_t @-> ptr void @-> returning int32_t)
let hnsw_index_find_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_find_keys"
    (index @-> ptr int64_t @-> int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_search_batch_keyed =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_keyed"
    (index @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> int64_t @-> ptr int64_t
     @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_index_insert_keyed =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_insert_keyed"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int64_t @-> ptr build_params @-> returning int32_t)
let hnsw_index_remove_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_remove_keys"
    (index @-> ptr int64_t @-> int64_t @-> ptr int32_t @-> returning int32_t)
let hnsw_index_upsert_keyed =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_upsert_keyed"
    (index @-> ptr float @-> ptr int64_t @-> int64_t @-> int64_t @-> ptr build_params @-> ptr uint8_t @-> ptr int32_t @-> returning int32_t)
let hnsw_index_update =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_update"
    (index @-> ptr int64_t @-> ptr float @-> int64_t @-> int64_t @-> ptr build_params @-> ptr int32_t @-> returning int32_t)
let hnsw_index_mark_deleted_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_mark_deleted_keys" (index @-> ptr int64_t @-> int64_t @-> returning int32_t)
let hnsw_index_unmark_deleted_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_unmark_deleted_keys" (index @-> ptr int64_t @-> int64_t @-> returning int32_t)
let hnsw_filter_create_by_keys =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_filter_create_by_keys"
    (index @-> ptr int64_t @-> int64_t @-> ptr filter_handle @-> returning int32_t)
(* search by stored item (see the C header, the last section): the queries are rows the index holds; only their ids cross the link *)
let hnsw_index_get_rows_device =
  foreign ~from:lib "hnsw_index_get_rows_device"
    (index @-> ptr int32_t @-> int64_t @-> ptr float @-> int64_t @-> ptr void @-> returning int32_t)
let hnsw_search_batch_by_id =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_by_id"
    (index @-> ptr int32_t @-> int64_t @-> ptr search_params @-> int32_t @-> ptr int32_t @-> ptr float @-> ptr uint32_t
     @-> ptr uint32_t @-> returning int32_t)
let hnsw_search_batch_by_key =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_by_key"
    (index @-> ptr int64_t @-> int64_t @-> ptr search_params @-> int32_t @-> int64_t @-> ptr int64_t @-> ptr float
     @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_brute_force_batch_by_id =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_brute_force_batch_by_id"
    (index @-> ptr int32_t @-> int64_t @-> int32_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float @-> returning int32_t)
let hnsw_knn_graph =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_knn_graph"
    (index @-> ptr search_params @-> int32_t @-> ptr int32_t @-> ptr float @-> returning int32_t)
(* paged search (see the C header, the last section): the next k after a (distance, id) cursor *)
type cursor
let cursor : cursor structure typ = structure "hnsw_cursor"
let cu_dist = field cursor "dist" float
let cu_id = field cursor "id" int32_t
let () = seal cursor
let hnsw_search_batch_after =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_after"
    (index @-> filter_handle @-> ptr cursor @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float
     @-> ptr cursor @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_brute_force_batch_after =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_brute_force_batch_after"
    (index @-> filter_handle @-> ptr cursor @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float
     @-> ptr cursor @-> returning int32_t)
(* diversified search (see the C header, the last section): greedy maximal marginal relevance over a pool of candidates *)
let hnsw_diversify_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_diversify_batch"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> int32_t @-> float @-> int32_t @-> ptr int32_t
     @-> ptr float @-> ptr float @-> returning int32_t)
let hnsw_search_batch_diverse =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_search_batch_diverse"
    (index @-> filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> int32_t @-> float @-> ptr int32_t
     @-> ptr float @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_brute_force_batch_diverse =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_brute_force_batch_diverse"
    (index @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> float @-> int32_t @-> ptr int32_t @-> ptr float
     @-> ptr float @-> returning int32_t)
let hnsw_index_deleted_count = foreign ~from:lib "hnsw_index_deleted_count" (index @-> ptr int64_t @-> returning int32_t)
let hnsw_index_deleted_bits = foreign ~from:lib "hnsw_index_deleted_bits" (index @-> ptr uint32_t @-> returning int32_t)
let hnsw_index_compact =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_compact" (index @-> ptr int32_t @-> returning int32_t)
let hnsw_index_save = foreign ~from:lib ~release_runtime_lock:true "hnsw_index_save" (index @-> string @-> returning int32_t)
let hnsw_index_load =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_load" (string @-> int32_t @-> ptr index @-> returning int32_t)
type layer_stats
let layer_stats : layer_stats structure typ = structure "hnsw_layer_stats"
let ls_num_nodes = field layer_stats "num_nodes" int64_t
let ls_min_degree = field layer_stats "min_degree" int32_t
let ls_max_degree = field layer_stats "max_degree" int32_t
let ls_mean_degree = field layer_stats "mean_degree" double
let ls_num_isolated = field layer_stats "num_isolated" int64_t
let () = seal layer_stats
let hnsw_index_layer_stats =
  foreign ~from:lib "hnsw_index_layer_stats" (index @-> int32_t @-> ptr layer_stats @-> returning int32_t)
let hnsw_index_layer_isolated =
  foreign ~from:lib "hnsw_index_layer_isolated"
    (index @-> int32_t @-> ptr int64_t @-> int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_index_locality_codes =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_locality_codes" (index @-> ptr int32_t @-> returning int32_t)
let hnsw_index_visited_blocks =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_visited_blocks" (index @-> ptr search_params @-> ptr int32_t @-> returning int32_t)
let hnsw_index_prepare =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_prepare" (index @-> ptr search_params @-> returning int32_t)
let hnsw_abi_version = foreign ~from:lib "hnsw_abi_version" (void @-> returning int32_t)
(* HNSW_ABI_VERSION of include/hnsw_mi355x.h this binding was written against: an older or newer library is refused at load
   time (version 2: hnsw_search_batch_h2d, hnsw_host_alloc / hnsw_host_free, hnsw_index_layer_isolated, hnsw_multi_debug_counters,
   hnsw_index_locality_codes; hnsw_index_info.row_format; the empty-layer values of hnsw_index_layer_stats; version 3:
   expected_ef / expected_semantics at the end of hnsw_index_desc and hnsw_build_params, hnsw_index_prepare, index file format 2) *)
let expected_abi_version = 3l
let () =
  let v = hnsw_abi_version () in
  if v <> expected_abi_version then
    failwith (Printf.sprintf "libhnsw_mi355x.so speaks ABI version %ld, this binding %ld" v expected_abi_version)
let hnsw_device_count = foreign ~from:lib "hnsw_device_count" (ptr int32_t @-> returning int32_t)
type index_info
let index_info : index_info structure typ = structure "hnsw_index_info"
let ii_n = field index_info "n" int64_t
let ii_d = field index_info "d" int32_t
let ii_metric = field index_info "metric" int32_t
let ii_id_base = field index_info "id_base" int32_t
let ii_max_degree0 = field index_info "max_degree0" int32_t
let ii_max_degree = field index_info "max_degree" int32_t
let ii_max_layer = field index_info "max_layer" int32_t
let ii_entry_point = field index_info "entry_point" int64_t
let ii_device_bytes = field index_info "device_bytes" int64_t
let ii_row_stride_bytes = field index_info "row_stride_bytes" int64_t
let ii_device = field index_info "device" int32_t
let ii_row_format = field index_info "row_format" int32_t
(* its values, HNSW_ROWS_*: float32 rows, byte rows, split rows, half rows (only after `hnsw_index_set_option idx
   "half_rows" 1L`: the search over the vectors rounded to fp16), sq8 rows (only after `hnsw_index_set_option idx "sq8_rows" 1L`:
   the walk over 8-bit codes, re-ranked over the float32 rows), per-dimension sq8 rows (only after `hnsw_index_set_option idx
   "sq8_dim_rows" 1L`: the same with one affine map per dimension) *)
let rows_f32 = 0l
let rows_bytes = 2l
let rows_split = 3l
let rows_half = 4l
let rows_sq8 = 5l
let rows_sq8_dim = 6l
(* bit rows (only after `hnsw_index_set_option idx "bit_rows" 1L` or `2L`: one bit per dimension, walked under Hamming distance) *)
let rows_bits = 7l
let () = seal index_info
let hnsw_index_get_info = foreign ~from:lib "hnsw_index_get_info" (index @-> ptr index_info @-> returning int32_t)
(* the flattened graph of a device index (built there by hnsw_build, or loaded from a file) back to the host *)
let hnsw_index_export_layer0 =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_export_layer0" (index @-> ptr int32_t @-> ptr int32_t @-> returning int32_t)
let hnsw_index_export_upper_count =
  foreign ~from:lib "hnsw_index_export_upper_count" (index @-> int32_t @-> ptr int64_t @-> returning int32_t)
let hnsw_index_export_upper =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_index_export_upper"
    (index @-> int32_t @-> ptr int64_t @-> ptr int32_t @-> ptr int32_t @-> returning int32_t)
let hnsw_multi_num_replicas = foreign ~from:lib "hnsw_multi_num_replicas" (multi @-> ptr int32_t @-> returning int32_t)
let hnsw_multi_replica = foreign ~from:lib "hnsw_multi_replica" (multi @-> int32_t @-> ptr index @-> returning int32_t)
(* device-pointer entry points (hnsw_search_batch_device, hnsw_distance_batch_device): for callers that already hold
   HIP device pointers and a stream; an OCaml program has neither, so they are bound as raw pointers only *)
let hnsw_search_batch_device =
  foreign ~from:lib "hnsw_search_batch_device"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float @-> ptr uint32_t
     @-> ptr uint32_t @-> ptr uint32_t @-> ptr void @-> returning int32_t)
let hnsw_search_batch_h2d =
  foreign ~from:lib "hnsw_search_batch_h2d"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int32_t @-> ptr float @-> ptr uint32_t
     @-> ptr uint32_t @-> ptr uint32_t @-> ptr void @-> returning int32_t)
let hnsw_distance_batch_device =
  foreign ~from:lib "hnsw_distance_batch_device"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> ptr float @-> ptr void @-> returning int32_t)
let hnsw_brute_force_batch_device =
  foreign ~from:lib "hnsw_brute_force_batch_device"
    (index @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float @-> ptr void @-> returning int32_t)
let hnsw_rerank_batch_device =
  foreign ~from:lib "hnsw_rerank_batch_device"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> int32_t @-> int32_t @-> ptr int32_t @-> ptr float
     @-> ptr void @-> returning int32_t)
let hnsw_diversify_batch_device =
  foreign ~from:lib "hnsw_diversify_batch_device"
    (index @-> ptr float @-> int64_t @-> int64_t @-> ptr int32_t @-> int32_t @-> int32_t @-> float @-> int32_t @-> ptr int32_t
     @-> ptr float @-> ptr float @-> ptr void @-> returning int32_t)
let hnsw_host_register = foreign ~from:lib "hnsw_host_register" (ptr void @-> int64_t @-> returning int32_t)
let hnsw_host_unregister = foreign ~from:lib "hnsw_host_unregister" (ptr void @-> returning int32_t)
let hnsw_host_alloc = foreign ~from:lib "hnsw_host_alloc" (ptr (ptr void) @-> int64_t @-> returning int32_t)
let hnsw_host_free = foreign ~from:lib "hnsw_host_free" (ptr void @-> returning int32_t)

(* Error convention -> the reference's exceptions (lib/ohnsw.ml:25,343,862) *)
let check rc =
  match Int32.to_int rc with
  | 0 -> ()
  | -1 | -2 | -3 -> invalid_arg (hnsw_last_error ())   (* BAD_ARG | EMPTY_INDEX | DEGREE_OVERFLOW *)
  | _ -> failwith (hnsw_last_error ())

(* ---- flatten ------------------------------------------------------------------------------- *)
module A1 = Bigarray.Array1
module A2 = Bigarray.Array2

type flat = {
  deg0 : (int32, Bigarray.int32_elt, Bigarray.c_layout) A1.t;
  nbr0 : (int32, Bigarray.int32_elt, Bigarray.c_layout) A2.t;   (* n x width0, iteration order *)
  upper : ((int64, Bigarray.int64_elt, Bigarray.c_layout) A1.t
           * (int32, Bigarray.int32_elt, Bigarray.c_layout) A1.t
           * (int32, Bigarray.int32_elt, Bigarray.c_layout) A2.t) array;
  entry_point : int;
  max_layer : int;
  width0 : int;          (* row width of layer 0: 2M, or the longest list found *)
  width_upper : int;     (* row width of the layers above: M, or the longest list found *)
}

(* Ohnsw.Hgraph.t (lib/ohnsw.ml:307-312): every layer is dense over all n nodes (:328-330);
   Graph.iter_neighbours (:176-180) walks nodes, Neighbours.iter (:127) walks a list head first --
   exactly the order search_k folds over (:570).  A list longer than its row raises: the C side
   would refuse it too (HNSW_ERR_DEGREE_OVERFLOW); nothing is ever truncated. *)
(* The row widths: with ~num_connections:m they are the caps the builder guarantees (2m on layer 0, m
   above, lib/ohnsw.ml:818-828); without it -- an Ohnsw.Hgraph.t does not record M -- they are the
   longest list found on layer 0 / on the layers above (one pass over the lists). *)
let ohnsw_widths (h : _ Ohnsw.Hgraph.t) =
  let n = Ohnsw.Hgraph.num_nodes h in
  let longest g =
    let w = ref 1 in
    for i = 0 to n - 1 do
      w := max !w (Ohnsw.Neighbours.length (Ohnsw.Graph.adjacent g i))
    done;
    !w in
  let w0 = longest (Ohnsw.Hgraph.layer h 0) in
  let wu = ref 1 in
  for l = 1 to Ohnsw.Hgraph.max_layer h do wu := max !wu (longest (Ohnsw.Hgraph.layer h l)) done;
  w0, !wu

let flatten_ohnsw ?num_connections (h : _ Ohnsw.Hgraph.t) : flat =
  let n = Ohnsw.Hgraph.num_nodes h in
  let max_layer = Ohnsw.Hgraph.max_layer h in
  let width0, width_upper = match num_connections with
    | Some m -> 2 * m, m
    | None -> ohnsw_widths h in
  let row g node width (dst : (int32, _, _) A2.t) r =
    let nb = Ohnsw.Graph.adjacent g node in
    if Ohnsw.Neighbours.length nb > width then invalid_arg "flatten: degree exceeds row width";
    let j = ref 0 in
    Ohnsw.Neighbours.iter nb ~f:(fun e -> dst.{r, !j} <- Int32.of_int e; incr j);
    !j
  in
  let deg0 = A1.create Bigarray.int32 Bigarray.c_layout n in
  let nbr0 = A2.create Bigarray.int32 Bigarray.c_layout n width0 in
  A2.fill nbr0 (-1l);
  let g0 = Ohnsw.Hgraph.layer h 0 in
  for i = 0 to n - 1 do deg0.{i} <- Int32.of_int (row g0 i width0 nbr0 i) done;
  let upper =
    Array.init max_layer (fun l ->
        let g = Ohnsw.Hgraph.layer h (l + 1) in
        (* nodes present on the layer: those with links there, plus the entry point *)
        let present i =
          Ohnsw.Neighbours.length (Ohnsw.Graph.adjacent g i) > 0
          || Ohnsw.Hgraph.entry_point h = Some i in
        let ids = List.filter present (List.init n (fun i -> i)) in
        let c = List.length ids in
        let nodes = A1.create Bigarray.int64 Bigarray.c_layout c in
        let deg = A1.create Bigarray.int32 Bigarray.c_layout c in
        let nbr = A2.create Bigarray.int32 Bigarray.c_layout c width_upper in
        A2.fill nbr (-1l);
        List.iteri (fun s i ->
            nodes.{s} <- Int64.of_int i;
            deg.{s} <- Int32.of_int (row g i width_upper nbr s)) ids;
        (nodes, deg, nbr))
  in
  { deg0; nbr0; upper; max_layer; width0; width_upper;
    entry_point = (match Ohnsw.Hgraph.entry_point h with Some e -> e | None -> -1) }

(* Hnsw.Ba.Hgraph.t (lib/hnsw.ml:342-348): layers = Map int -> MapGraph.t, a MapGraph holding
   connections = Map int -> NeighbourList.t ({list; length}, lib/hnsw.ml:33-45).  Node ids are the
   1-based matrix columns (lib/hnsw.ml:325); a node without an entry in a layer's map has no
   neighbours there (MapGraph.adjacent, lib/hnsw.ml:146-149).  NeighbourList.fold walks the list head
   first (lib/hnsw.ml:44-45), which is the order Search.search folds over (lib/hnsw_algo.ml:381-383).
   Pass the result to [create ~id_base:1]. *)
let ba_widths (h : Hnsw.Ba.Hgraph.t) =
  let module G = Hnsw.Ba.Hgraph in
  let longest (g : Hnsw.MapGraph.t) =
    Base.Map.fold g.Hnsw.MapGraph.connections ~init:1 ~f:(fun ~key:_ ~data w ->
        max w (Hnsw.NeighbourList.length data)) in
  let w0 = longest (G.layer h 0) in
  let wu = ref 1 in
  for l = 1 to G.max_layer h do wu := max !wu (longest (G.layer h l)) done;
  w0, !wu

let flatten_ba ?num_connections (h : Hnsw.Ba.Hgraph.t) : flat =
  let module G = Hnsw.Ba.Hgraph in
  let n = G.max_node_id h in                       (* = Values.length, lib/hnsw.ml:394 *)
  let max_layer = G.max_layer h in
  let width0, width_upper = match num_connections with
    | Some m -> 2 * m, m
    | None -> ba_widths h in
  let fill_row (nl : Hnsw.NeighbourList.t) width (dst : (int32, _, _) A2.t) r =
    if Hnsw.NeighbourList.length nl > width then invalid_arg "flatten: degree exceeds row width";
    let j = ref 0 in
    Hnsw.NeighbourList.fold nl ~init:() ~f:(fun () e -> dst.{r, !j} <- Int32.of_int e; incr j);
    !j
  in
  let deg0 = A1.create Bigarray.int32 Bigarray.c_layout n in
  let nbr0 = A2.create Bigarray.int32 Bigarray.c_layout n width0 in
  A1.fill deg0 0l; A2.fill nbr0 (-1l);
  let g0 = G.layer h 0 in
  Base.Map.iteri g0.Hnsw.MapGraph.connections ~f:(fun ~key ~data ->
      deg0.{key - 1} <- Int32.of_int (fill_row data width0 nbr0 (key - 1)));
  let upper =
    Array.init max_layer (fun l ->
        let g = G.layer h (l + 1) in
        let c = Base.Map.length g.Hnsw.MapGraph.connections in
        let nodes = A1.create Bigarray.int64 Bigarray.c_layout c in
        let deg = A1.create Bigarray.int32 Bigarray.c_layout c in
        let nbr = A2.create Bigarray.int32 Bigarray.c_layout c width_upper in
        A2.fill nbr (-1l);
        let s = ref 0 in
        Base.Map.iteri g.Hnsw.MapGraph.connections ~f:(fun ~key ~data ->
            nodes.{!s} <- Int64.of_int key;
            deg.{!s} <- Int32.of_int (fill_row data width_upper nbr !s);
            incr s);
        (nodes, deg, nbr))
  in
  { deg0; nbr0; upper; max_layer; width0; width_upper;
    entry_point = G.entry_point h (* -1 when empty, lib/hnsw.ml:391 *) }

(* The inverse for the functor path: rebuild a Hnsw.Ba.Hgraph.t (lib/hnsw.ml:342-348) over the value
   matrix from flattened tables with 1-based ids.  The record fields are the reference's own: layers is a
   Map from layer to MapGraph.t = { connections : NeighbourList.t Map.M(Int).t; max_node_id }
   (lib/hnsw.ml:122-135), a NeighbourList is { list; length } with the list in fold order (head first,
   lib/hnsw.ml:33-45) -- the row order.  Nodes without links on a layer get no map entry, as
   MapGraph.adjacent expects (lib/hnsw.ml:146-149); the tables hold symmetric links already. *)
let unflatten_ba (values : Lacaml.S.mat) (f : flat) : Hnsw.Ba.Hgraph.t =
  let n = Lacaml.S.Mat.dim2 values in
  let list_of_row (nbr : (int32, _, _) A2.t) r deg =
    let l = ref [] in
    for j = deg - 1 downto 0 do l := Int32.to_int nbr.{r, j} :: !l done;
    { Hnsw.NeighbourList.list = !l; length = deg } in
  let graph_of rows =
    { Hnsw.MapGraph.connections =
        List.fold_left (fun m (node, nl) -> Base.Map.set m ~key:node ~data:nl)
          (Base.Map.empty (module Base.Int)) rows;
      max_node_id = n } in
  let layer0 =
    let rows = ref [] in
    for i = A1.dim f.deg0 - 1 downto 0 do
      let deg = Int32.to_int f.deg0.{i} in
      if deg > 0 then rows := (i + 1, list_of_row f.nbr0 i deg) :: !rows
    done;
    graph_of !rows in
  let layers = ref (Base.Map.set (Base.Map.empty (module Base.Int)) ~key:0 ~data:layer0) in
  Array.iteri (fun l (nodes, deg, nbr) ->
      let rows = ref [] in
      for r = A1.dim nodes - 1 downto 0 do
        rows := (Int64.to_int nodes.{r}, list_of_row nbr r (Int32.to_int deg.{r})) :: !rows
      done;
      layers := Base.Map.set !layers ~key:(l + 1) ~data:(graph_of !rows)) f.upper;
  { Hnsw.Ba.Hgraph.layers = !layers; max_layer = f.max_layer; entry_point = f.entry_point; values }

(* The inverse: rebuild an Ohnsw.Hgraph.t from the flattened tables (e.g. an index built on the device by
   hnsw_build and fetched with hnsw_index_export_*), so that the OCaml builder can keep inserting into
   it.  Every Neighbours.t gets its list in the stored order (Neighbours.iter order = search_k's
   fold order, :127,:570): Neighbours.add conses (:116-118), so a row is pushed back to front.  The
   tables hold symmetric links already, so the rows are written with Vector.set, not with
   Graph.set_connections (which would add every link twice, :182-196). *)
let unflatten_ohnsw (distance : 'a Ohnsw.distance) (value : 'a Ohnsw.value) (f : flat) : 'a Ohnsw.Hgraph.t =
  let h = Ohnsw.Hgraph.create distance value in
  let n = A1.dim f.deg0 in
  for _ = 1 to n do ignore (Ohnsw.Hgraph.add_node h) done;          (* lib/ohnsw.ml:328-330 *)
  Ohnsw.Hgraph.set_max_layer h f.max_layer;                            (* :347-351 *)
  let neighbours_of_row (nbr : (int32, _, _) A2.t) r deg =
    let nb = Ohnsw.Neighbours.create () in
    for j = deg - 1 downto 0 do Ohnsw.Neighbours.add nb (Int32.to_int nbr.{r, j}) done;
    nb in
  let g0 = Ohnsw.Hgraph.layer h 0 in
  for i = 0 to n - 1 do
    Ohnsw.Vector.set g0 i (neighbours_of_row f.nbr0 i (Int32.to_int f.deg0.{i}))
  done;
  Array.iteri (fun l (nodes, deg, nbr) ->
      let g = Ohnsw.Hgraph.layer h (l + 1) in
      for r = 0 to A1.dim nodes - 1 do
        Ohnsw.Vector.set g (Int64.to_int nodes.{r}) (neighbours_of_row nbr r (Int32.to_int deg.{r}))
      done) f.upper;
  if f.entry_point >= 0 then Ohnsw.Hgraph.set_entry_point h f.entry_point;   (* :341-344 *)
  h

(* ---- device-resident index ------------------------------------------------------------------ *)
(* [scratch]: page-locked result matrices per (k, nq) shape, see [scratch_for]: they belong to the HANDLE, so two threads that
   search two different indices (one thread at a time per handle, INTEGRATION.md) never write into the same matrices *)
type result_scratch = (int * int, (int32, Bigarray.int32_elt, Bigarray.fortran_layout) A2.t * Lacaml.S.mat) Hashtbl.t
type t = { handle : index; k_base : int; dim : int; scratch : result_scratch }

(* ?expected_ef (and ?expected_semantics: 0 Ohnsw's accept rule, 1 the functor's): the upload also does, once, what the first
   search with these parameters would otherwise do inside the call (hnsw_index_prepare) *)
let create ?(device = 0) ?(metric = 0) ?(expected_ef = 0) ?(expected_semantics = 0) ~id_base (vectors : Lacaml.S.mat) (f : flat) : t =
  (* a Lacaml.S.mat is a Fortran-layout dim x n Bigarray: in memory, n rows of dim floats *)
  let dim = A2.dim1 vectors and n = A2.dim2 vectors in
  let layers = CArray.make layer_desc (max 1 f.max_layer) in
  Array.iteri (fun l (nodes, deg, nbr) ->
      let ld = CArray.get layers l in
      setf ld ld_n_nodes (Int64.of_int (A1.dim nodes));
      setf ld ld_nodes (bigarray_start array1 nodes);
      setf ld ld_deg (bigarray_start array1 deg);
      setf ld ld_nbr (bigarray_start array2 nbr)) f.upper;
  let d = make index_desc in
  setf d d_vectors (bigarray_start array2 vectors);
  setf d d_n (Int64.of_int n); setf d d_d (Int32.of_int dim);
  setf d d_row_stride (Int64.of_int dim);
  setf d d_metric (Int32.of_int metric); setf d d_id_base (Int32.of_int id_base);
  setf d d_max_degree0 (Int32.of_int f.width0); setf d d_max_degree (Int32.of_int f.width_upper);
  setf d d_max_layer (Int32.of_int f.max_layer);
  setf d d_entry_point (Int64.of_int f.entry_point);
  setf d d_deg0 (bigarray_start array1 f.deg0); setf d d_nbr0 (bigarray_start array2 f.nbr0);
  setf d d_upper (CArray.start layers);
  setf d d_expected_ef (Int32.of_int expected_ef); setf d d_expected_semantics (Int32.of_int expected_semantics);
  let out = allocate index null in
  check (hnsw_index_create (addr d) (Int32.of_int device) out);
  let t = { handle = !@out; k_base = id_base; dim; scratch = Hashtbl.create 4 } in
  Gc.finalise (fun t -> ignore (hnsw_index_destroy t.handle)) t;
  t

(* A Lacaml-shaped matrix (float32, Fortran layout, dim x n) in page-locked memory the LIBRARY allocates (hnsw_host_alloc):
   knn_batch* reads such a query matrix and writes such result matrices straight from the device, without copies.
   Freed by the finaliser of the returned Bigarray (keep using the memory only through the returned value). *)
let alloc_mat ~dim ~n : Lacaml.S.mat =
  let out = allocate (ptr void) null in
  check (hnsw_host_alloc out (Int64.of_int (4 * dim * (max n 1))));
  let p = !@out in
  let m = bigarray_of_ptr array2 (n, dim) Bigarray.float32 (from_voidp float p) in          (* n rows of dim floats in memory ... *)
  let m = Bigarray.Array2.change_layout m Bigarray.fortran_layout in                      (* ... = a dim x n Fortran matrix, as Lacaml's *)
  Gc.finalise (fun _ -> ignore (hnsw_host_free p)) m;
  m

(* the same for the int32 id table of a batch (k x nq Fortran = [nq][k] in memory) *)
let alloc_ids ~k ~nq : (int32, Bigarray.int32_elt, Bigarray.fortran_layout) A2.t =
  let out = allocate (ptr void) null in
  check (hnsw_host_alloc out (Int64.of_int (4 * k * (max nq 1))));
  let p = !@out in
  let m = bigarray_of_ptr array2 (nq, k) Bigarray.int32 (from_voidp int32_t p) in
  let m = Bigarray.Array2.change_layout m Bigarray.fortran_layout in
  Gc.finalise (fun _ -> ignore (hnsw_host_free p)) m;
  m

(* Page-locked result scratch, one pair per handle and (k, nq) shape seen (a benchmark or serving loop repeats its shape): the
   search kernel writes every query's results straight into it as the query finishes -- no download step -- and [search] hands
   fresh matrices to its caller, as the reference does (lib/ohnsw.ml:879-881), by two blits of 4 k nq bytes each.
   (Allocating page-locked memory costs far more than a batch takes, so the scratch is kept, not the results.)  The table is
   a field of the handle (round 4 kept ONE table for the process: two threads searching two indices with the same batch shape
   -- the call releases the runtime lock -- then had their kernels write into the same matrices); it dies with the handle,
   its blocks through their own finalisers (hnsw_host_free). *)
let scratch_for (t : t) ~k ~nq =
  match Hashtbl.find_opt t.scratch (k, nq) with
  | Some s -> s
  | None ->
    if Hashtbl.length t.scratch >= 8 then Hashtbl.reset t.scratch;   (* shapes keep changing: do not hoard *)
    let s = (alloc_ids ~k ~nq, alloc_mat ~dim:k ~n:nq) in
    Hashtbl.replace t.scratch (k, nq) s;
    s

let search ?(semantics = 0) t (batch : Lacaml.S.mat) ~ef ~k ~fill =
  let nq = A2.dim2 batch in
  (* results as the reference lays them out: k x nq Fortran = [nq][k] in memory; written by the device into the
     page-locked scratch, then copied into fresh matrices for the caller *)
  let ids_s, dist_s = scratch_for t ~k ~nq in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_search_batch t.handle (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int t.dim) (addr p) (bigarray_start array2 ids_s)
           (bigarray_start array2 dist_s) (from_voidp uint32_t null) (from_voidp uint32_t null));
  let distances = Lacaml.S.Mat.create k nq in
  let ids = A2.create Bigarray.int32 Bigarray.fortran_layout k nq in
  A2.blit dist_s distances;
  A2.blit ids_s ids;
  ids, distances

(* ---- from the reference's own index values, nothing else needed ----------------------------------- *)

(* of_ohnsw : Lacaml.S.vec Ohnsw.Hgraph.t -> t.  An Ohnsw.Hgraph.t (lib/ohnsw.ml:307-312) holds no
   matrix and no M: the vectors are gathered through its own [value : int -> Lacaml.S.vec] closure
   (for a graph from build_batch_bigarray that is [fun i -> Mat.col batch (i+1)], :842) into a fresh
   dim x n matrix, and the row widths are the longest lists found (ohnsw_widths). *)
let of_ohnsw ?device ?metric (h : Lacaml.S.vec Ohnsw.Hgraph.t) : t =
  let n = Ohnsw.Hgraph.num_nodes h in
  if n = 0 then invalid_arg "knn: empty hgraph";                        (* lib/ohnsw.ml:862 *)
  let value = Ohnsw.Hgraph.value h in
  let dim = Lacaml.S.Vec.dim (value 0) in
  let vectors = Lacaml.S.Mat.create dim n in
  for i = 0 to n - 1 do
    A1.blit (value i) (Lacaml.S.Mat.col vectors (i + 1))                (* node i <-> column i+1, :842 *)
  done;
  create ?device ?metric ~id_base:0 vectors (flatten_ohnsw h)

(* of_ba : Hnsw.Ba.Hgraph.t -> t.  The functor path's Hgraph carries its value matrix
   (values : BaValues.t = Lacaml.S.mat, lib/hnsw.ml:346 with :296-301); node ids are its columns (1-based). *)
let of_ba ?device ?metric (h : Hnsw.Ba.Hgraph.t) : t =
  if Hnsw.Ba.Hgraph.is_empty h then invalid_arg "knn: empty hgraph";
  create ?device ?metric ~id_base:1 h.Hnsw.Ba.Hgraph.values (flatten_ba h)

(* One device index per live hgraph: an association list of ephemerons keyed by the hgraph value itself
   (physical equality), so an index is destroyed (Gc.finalise in [create]) once its hgraph is collected.
   An Ohnsw.Hgraph.t is mutable -- the OCaml builder may keep inserting --, so an entry also records
   (number of nodes, entry point, max layer) and is rebuilt when they no longer match: every insert adds a
   node (lib/ohnsw.ml:766-772), so a changed graph always shows. *)
type cached = { index : t; stamp : int * int * int }
let cache : (Obj.t, cached) Ephemeron.K1.t list ref = ref []

let cached_index (key : Obj.t) ~(stamp : int * int * int) ~(make : unit -> t) : t =
  let live = List.filter (fun e -> Ephemeron.K1.check_key e) !cache in
  let hit = List.find_opt (fun e ->
      match Ephemeron.K1.get_key e with Some k -> k == key | None -> false) live in
  match hit with
  | Some e when (match Ephemeron.K1.get_data e with Some c -> c.stamp = stamp | None -> false) ->
    cache := live;
    (match Ephemeron.K1.get_data e with Some c -> c.index | None -> assert false)
  | _ ->
    let index = make () in
    let e = Ephemeron.K1.create () in
    Ephemeron.K1.set_key e key;
    Ephemeron.K1.set_data e { index; stamp };
    cache := e :: List.filter (fun e' -> match hit with Some h -> e' != h | None -> true) live;
    index

let index_of_ohnsw (h : Lacaml.S.vec Ohnsw.Hgraph.t) : t =
  let stamp = (Ohnsw.Hgraph.num_nodes h,
               (match Ohnsw.Hgraph.entry_point h with Some e -> e | None -> -1),
               Ohnsw.Hgraph.max_layer h) in
  cached_index (Obj.repr h) ~stamp ~make:(fun () -> of_ohnsw h)

let index_of_ba (h : Hnsw.Ba.Hgraph.t) : t =
  (* persistent structure: a modified graph is a different value, the stamp is only a cheap guard *)
  let stamp = (Hnsw.Ba.Hgraph.max_node_id h, Hnsw.Ba.Hgraph.entry_point h, Hnsw.Ba.Hgraph.max_layer h) in
  cached_index (Obj.repr h) ~stamp ~make:(fun () -> of_ba h)

(* ---- the drop-in bodies ---------------------------------------------------------------------- *)

(* on an explicit handle *)
let ohnsw_knn_batch_bigarray (t : t) ~k (batch : Lacaml.S.mat) =
  let ids32, distances = search t batch ~ef:k ~k ~fill:0 (* NaN / -1, :880-881 *) in
  let nq = A2.dim2 batch in
  let ids = Array.init nq (fun j -> Array.init k (fun i -> Int32.to_int ids32.{i + 1, j + 1})) in
  ids, distances

(* Ohnsw.knn_batch_bigarray (lib/ohnsw.ml:877-897) with its exact signature, at the value type the GPU
   path needs:
     Lacaml.S.vec Ohnsw.Hgraph.t -> k:int -> Lacaml.S.mat -> int array array * Lacaml.S.mat
   An empty batch returns empty results, as the reference's fold does; an empty hgraph raises
   Invalid_argument "knn: empty hgraph" (:862) as soon as there is a query. *)
let knn_batch_bigarray (hgraph : Lacaml.S.vec Ohnsw.Hgraph.t) ~k (batch : Lacaml.S.mat) :
  int array array * Lacaml.S.mat =
  if Lacaml.S.Mat.dim2 batch = 0 then [||], Lacaml.S.Mat.create k 0
  else ohnsw_knn_batch_bigarray (index_of_ohnsw hgraph) ~k batch

(* Hnsw.Ba.knn_batch : t -> Lacaml.S.mat -> num_neighbours_search:int -> num_neighbours:int
   -> Lacaml.S.mat (lib/hnsw.ml:769-777): distances only, +inf filled (:771).
   semantics 1 = Nearest.insert_distance's rule (lib/hnsw.ml:494-506: a neighbour tied with max(W) is
   Inserted and expanded, W keeps the incumbent) with (distance, id) order among equal keys; 2 = the same +
   Nearest.nearest_k's output (the k farthest of W when num_neighbours_search > num_neighbours,
   lib/hnsw.ml:522-525) for callers that want the reference's defect reproduced. *)
let ba_knn_batch ?(nearest_k_compat = false) (t : t) (batch : Lacaml.S.mat) ~num_neighbours_search ~num_neighbours =
  snd (search ~semantics:(if nearest_k_compat then 2 else 1) t batch ~ef:num_neighbours_search ~k:num_neighbours ~fill:1)

(* ... and with the reference's signature (the body of MakeBatch.knn_batch at Distance = EuclideanBa) *)
let knn_batch ?nearest_k_compat (hgraph : Hnsw.Ba.Hgraph.t) (batch : Lacaml.S.mat) ~num_neighbours_search ~num_neighbours :
  Lacaml.S.mat =
  if Lacaml.S.Mat.dim2 batch = 0 then Lacaml.S.Mat.create num_neighbours 0
  else ba_knn_batch ?nearest_k_compat (index_of_ba hgraph) batch ~num_neighbours_search ~num_neighbours

(* Hnsw.Make(Batch).knn_batch (lib/hnsw.ml:781-807): the generic front-end returns a Batch.Distances.t filled
   through Batch.Distances.set with one value_distance list per query.  A Batch whose values are
   Lacaml.S.vec (the only kind the device path can take: BATCH with type value = Lacaml.S.vec) is served
   by gathering the batch into a matrix, one device call, and feeding Distances.set row by row. *)
module MakeBatchGpu (Batch : Hnsw.BATCH with type value = Lacaml.S.vec) = struct
  let knn_batch (t : t) (batch : Batch.t) ~num_neighbours_search ~num_neighbours : Batch.Distances.t =
    let nq = Batch.length batch in
    let distances = Batch.Distances.create ~len_batch:nq ~num_neighbours in
    if nq > 0 then begin
      let m = Lacaml.S.Mat.create t.dim nq in
      ignore (Batch.fold batch ~init:1 ~f:(fun j (row : Lacaml.S.vec) ->
          A1.blit row (Lacaml.S.Mat.col m j); j + 1));
      let ids, dist = search ~semantics:1 t m ~ef:num_neighbours_search ~k:num_neighbours ~fill:1 in
      for j = 1 to nq do
        let l = ref [] in
        for i = num_neighbours downto 1 do
          let node = Int32.to_int ids.{i, j} in
          if node >= t.k_base then
            l := { Hnsw_algo.node; distance_to_target = dist.{i, j} } :: !l
        done;
        Batch.Distances.set distances j !l                     (* lib/hnsw.ml:803-804: i counts from 1 *)
      done
    end;
    distances
end

(* Ohnsw.search_k (lib/ohnsw.ml:543-588) on one layer for ONE target: the start MinQueue as a node
   list, the result MinQueue as an ascending (node, distance) list.  ~semantics:1 is
   Hnsw_algo.Search.search (lib/hnsw_algo.ml:350-391). *)
let search_k ?(semantics = 0) (t : t) ~layer ~(start_nodes : int list) (target : Lacaml.S.vec) ~k =
  let ns = List.length start_nodes in
  let st = CArray.of_list int64_t (List.map Int64.of_int start_nodes) in
  let ids = CArray.make int32_t k and dist = CArray.make float k in
  let cnt = allocate int32_t 0l in
  let p = make search_params in
  setf p p_ef (Int32.of_int k); setf p p_k (Int32.of_int k); setf p p_fill 0l;
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_search_layer_batch t.handle (Int32.of_int layer) (bigarray_start array1 target) 1L
           (Int64.of_int t.dim) (CArray.start st) (Int32.of_int ns) (addr p) (CArray.start ids)
           (CArray.start dist) cnt (from_voidp uint32_t null) (from_voidp uint32_t null));
  List.init (Int32.to_int !@cnt) (fun i -> Int32.to_int (CArray.get ids i), CArray.get dist i)

(* Ohnsw.search_one (lib/ohnsw.ml:492-512): the node the greedy walk on `layer` ends on *)
let search_one (t : t) ~layer ~start_node (target : Lacaml.S.vec) =
  let st = allocate int64_t (Int64.of_int start_node) and node = allocate int64_t 0L in
  check (hnsw_search_one_batch t.handle (Int32.of_int layer) (bigarray_start array1 target) 1L
           (Int64.of_int t.dim) st node (from_voidp float null));
  Int64.to_int !@node

(* Batches in flight: [submit] copies the batch in and starts the search, [wait] returns what
   [search] would have.  A caller with more than one batch overlaps them
   (let r1 = submit t b1 ... in let r2 = submit t b2 ... in wait r1; wait r2): the next batch fills
   the drain of the previous one (round 3, SIFT1M-shaped workload, registered matrices, PCIe copies included:
   36 M q/s with two requests in flight against 16.7 M q/s for back-to-back synchronous calls). *)
type pending = { req : request; p_k : int; p_nq : int; keep : Lacaml.S.mat }

let submit ?(semantics = 0) t (batch : Lacaml.S.mat) ~ef ~k ~fill : pending =
  let nq = A2.dim2 batch in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  let out = allocate request null in
  check (hnsw_search_submit t.handle (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int t.dim) (addr p) out);
  { req = !@out; p_k = k; p_nq = nq; keep = batch }

let wait (r : pending) =
  let distances = Lacaml.S.Mat.create r.p_k r.p_nq in
  let ids = A2.create Bigarray.int32 Bigarray.fortran_layout r.p_k r.p_nq in
  check (hnsw_search_wait r.req (bigarray_start array2 ids) (bigarray_start array2 distances)
           (from_voidp uint32_t null) (from_voidp uint32_t null));
  ids, distances

(* ---- single query ------------------------------------------------------------------------------ *)

(* one query through hnsw_knn: the (node, distance) pairs found, nearest first *)
let knn_on ?(semantics = 0) (t : t) (target : Lacaml.S.vec) ~ef ~k ~fill : (int * float) list =
  let ids = CArray.make int32_t k and dist = CArray.make float k in
  let cnt = allocate int32_t 0l in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_knn t.handle (bigarray_start array1 target) (addr p) (CArray.start ids) (CArray.start dist) cnt);
  List.init (Int32.to_int !@cnt) (fun i -> Int32.to_int (CArray.get ids i), CArray.get dist i)

(* Ohnsw.knn (lib/ohnsw.ml:859-875).  The reference's signature is
     'a Hgraph.t -> Visited.t -> k:int -> 'a -> 'a MinQueue.t
   whose result type is abstract outside lib/ohnsw.ml (:404-416; test/test.ml:122-125 no longer type-checks against
   it): what a caller can do with it is pop it nearest first (:886-893), so that list is what is returned, and the
   scratch Visited.t (device-side state here) is not taken.  An empty hgraph raises Invalid_argument
   "knn: empty hgraph" (:861-862). *)
let knn (hgraph : Lacaml.S.vec Ohnsw.Hgraph.t) ~k (target : Lacaml.S.vec) : (int * float) list =
  knn_on (index_of_ohnsw hgraph) target ~ef:k ~k ~fill:0

(* Hnsw.Ba.knn (lib/hnsw.ml:763-767):
     t -> Lacaml.S.vec -> num_neighbours_search:int -> num_neighbours:int -> int Hnsw_algo.value_distance list
   1-based node ids, the functor path's accept rule (semantics 1); ~nearest_k_compat:true reproduces
   Nearest.nearest_k's output (lib/hnsw.ml:522-525) as in [knn_batch]. *)
let ba_knn ?(nearest_k_compat = false) (hgraph : Hnsw.Ba.Hgraph.t) (target : Lacaml.S.vec) ~num_neighbours_search ~num_neighbours :
  int Hnsw_algo.value_distance list =
  knn_on ~semantics:(if nearest_k_compat then 2 else 1) (index_of_ba hgraph) target
    ~ef:num_neighbours_search ~k:num_neighbours ~fill:1
  |> List.map (fun (node, distance_to_target) -> { Hnsw_algo.node; distance_to_target })

(* ---- the other operators of the header ----------------------------------------------------------- *)

(* distances.(q).(j) = distance (query q) (value ids.(q).(j)): EuclideanBa.distance / Ohnsw.distance_l2 gathered on the
   device (lib/hnsw.ml:809-815, lib/ohnsw.ml:899; bench_dist/bench_dist.ml:22-33 times exactly this, one pair per call) *)
let distance_batch (t : t) (queries : Lacaml.S.mat) (ids : int array array) : float array array =
  let nq = A2.dim2 queries in
  if Array.length ids <> nq then invalid_arg "distance_batch: one id list per query";
  let m = if nq = 0 then 0 else Array.length ids.(0) in
  let flat_ids = CArray.make int32_t (max 1 (nq * m)) and out = CArray.make float (max 1 (nq * m)) in
  Array.iteri (fun q row ->
      if Array.length row <> m then invalid_arg "distance_batch: ragged id lists";
      Array.iteri (fun j v -> CArray.set flat_ids (q * m + j) (Int32.of_int v)) row) ids;
  check (hnsw_distance_batch t.handle (bigarray_start array2 queries) (Int64.of_int nq) (Int64.of_int t.dim)
           (CArray.start flat_ids) (Int32.of_int m) (CArray.start out));
  Array.init nq (fun q -> Array.init m (fun j -> CArray.get out (q * m + j)))

(* The exact scan (hnsw_brute_force_batch) over the vectors the index holds, with its metric: for each query (a column of
   [test]) the k smallest of all stored vectors under (distance, node id), ascending.  -> (ids, distances), both
   [nq][k]; where k exceeds the number of vectors: id -1, distance nan. *)
let brute_force_knn (t : t) (test : Lacaml.S.mat) ~k : int array array * float array array =
  let nq = A2.dim2 test in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  check (hnsw_brute_force_batch t.handle (bigarray_start array2 test) (Int64.of_int nq) (Int64.of_int t.dim)
           (Int32.of_int k) 0l (CArray.start ids) (CArray.start dist));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))

(* The exact re-rank (hnsw_rerank_batch): for each query (a column of [queries]) the k nearest of ITS candidates
   [candidates.(q)] (node ids; lists may differ in length) over the float32 vectors the index holds, under (distance, node id),
   ascending -- what `hnsw_index_set_option idx "refine" r` does to the half-row searches' candidates.  -> (ids, distances), both
   [nq][k]; past a query's candidates: id -1, distance nan. *)
let rerank (t : t) (queries : Lacaml.S.mat) ~(candidates : int array array) ~k : int array array * float array array =
  let nq = A2.dim2 queries in
  if Array.length candidates <> nq then invalid_arg "rerank: one candidate list per query";
  let stride = Array.fold_left (fun m row -> max m (Array.length row)) 1 candidates in
  let cand = CArray.make int32_t ~initial:(Int32.of_int (t.k_base - 1)) (max 1 (nq * stride)) in
  Array.iteri (fun q row -> Array.iteri (fun j v -> CArray.set cand (q * stride + j) (Int32.of_int v)) row) candidates;
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  check (hnsw_rerank_batch t.handle (bigarray_start array2 queries) (Int64.of_int nq) (Int64.of_int t.dim)
           (CArray.start cand) (Int32.of_int stride) (Int32.of_int k) 0l (CArray.start ids) (CArray.start dist));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))

(* Filtered search (hnsw_filter_create / hnsw_search_batch_filtered): the k nearest AMONG the nodes a mask allows.
   [filter_create t allow]: allow.(v) = node v + id_base may be returned; one entry per node of the index (the library refuses
   any other length).  The mask is uploaded once and reused; it is refused once the index has grown ([insert]).  The filter keeps
   its index alive; it is freed with the value. *)
type filter = { f_handle : filter_handle; f_index : t }

let filter_create (t : t) (allow : bool array) : filter =
  let n = Array.length allow in
  let words = (n + 31) / 32 in
  let bits = CArray.make uint32_t ~initial:Unsigned.UInt32.zero (max 1 words) in
  Array.iteri (fun v a ->
      if a then CArray.set bits (v lsr 5) (Unsigned.UInt32.logor (CArray.get bits (v lsr 5)) (Unsigned.UInt32.shift_left Unsigned.UInt32.one (v land 31))))
    allow;
  let out = allocate filter_handle null in
  check (hnsw_filter_create t.handle (CArray.start bits) (Int64.of_int n) out);
  let f = { f_handle = !@out; f_index = t } in
  Gc.finalise (fun f -> ignore (hnsw_filter_destroy f.f_handle)) f;
  f

(* the number of allowed nodes *)
let filter_count (f : filter) : int =
  let c = allocate int64_t 0L in
  check (hnsw_filter_count f.f_handle c);
  Int64.to_int !@c

(* [knn_batch_filtered f batch ~ef ~k]: for each query (a column of [batch]) the k nearest allowed nodes.  W grows ef, 2 ef, ...
   1024 until it holds k allowed nodes; a query still short is answered by the exact scan over the allowed nodes.  Distances are
   over the float32 vectors whatever rows the index searches.  -> (ids, distances, stages), ids and distances [nq][k] (id -1,
   distance nan -- ~fill:1: infinity -- where fewer than k nodes are allowed), stages.(q) = how often W doubled, -1 = exact scan.
   ~semantics: 0 Ohnsw's accept rule, 1 the functor's (2 is refused).
   After `hnsw_index_set_option idx "filter_collect" 1L` (off by default; k <= 128, float32 / byte / split rows) the answer comes from
   every node the layer-0 walk evaluates, not from the final W only: a query is served at the first stage whose walk evaluated k
   allowed nodes (the C header: WITH OPTION filter_collect). *)
let knn_batch_filtered ?(semantics = 0) ?(fill = 0) (f : filter) (batch : Lacaml.S.mat) ~ef ~k :
  int array array * float array array * int array =
  let t = f.f_index in
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_search_batch_filtered t.handle f.f_handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim)
           (addr p) (CArray.start ids) (CArray.start dist) (from_voidp uint32_t null) (from_voidp uint32_t null)
           (CArray.start stage));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s))

(* Grouped search (hnsw_labels_create / hnsw_search_batch_grouped): the k nearest GROUPS, one node per label.
   [labels_create t labels ~n_labels]: labels.(v) in -1 .. n_labels - 1 is node v's group, -1 = none; one entry per node of the
   index.  Uploaded once and reused; refused once the index has changed ([insert], [remove], marks).  Keeps its index alive. *)
type labels = { l_handle : labels_handle; l_index : t; l_n : int }

let labels_create (t : t) (labels : int array) ~n_labels : labels =
  let n = Array.length labels in
  let lab = CArray.make int32_t (max 1 n) in
  Array.iteri (fun v l -> CArray.set lab v (Int32.of_int l)) labels;
  let out = allocate labels_handle null in
  check (hnsw_labels_create t.handle (CArray.start lab) (Int64.of_int n) (Int32.of_int n_labels) out);
  let l = { l_handle = !@out; l_index = t; l_n = n } in
  Gc.finalise (fun l -> ignore (hnsw_labels_destroy l.l_handle)) l;
  l

(* (n_labels, n_labelled, n_groups): the nodes with a label >= 0, the labels at least one node carries *)
let labels_info (l : labels) : int * int * int =
  let a = allocate int32_t 0l and b = allocate int64_t 0L and c = allocate int64_t 0L in
  check (hnsw_labels_info l.l_handle a b c);
  (Int32.to_int !@a, Int64.to_int !@b, Int64.to_int !@c)

(* the labels as the device holds them: -1 where the node was marked deleted at creation *)
let labels_get (l : labels) : int array =
  let out = CArray.make int32_t (max 1 l.l_n) in
  check (hnsw_labels_get l.l_handle (CArray.start out));
  Array.init l.l_n (fun v -> Int32.to_int (CArray.get out v))

let grouped_rows nq k ids dist lab =
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get lab (q * k + j)))))

(* [knn_batch_grouped l batch ~ef ~k]: for each query (a column of [batch]) the k nearest distinct labels, each represented by its
   nearest node.  W grows ef, 2 ef, ... 1024 until it holds nodes of k labels; a query still short is answered by the exact
   grouped scan.  ?filter: only allowed nodes count.  -> (ids, distances, labels, stages), [nq][k] each (id -1, label -1,
   distance nan -- ~fill:1: infinity -- where there are fewer than k groups), stages.(q) = how often W doubled, -1 = exact. *)
let knn_batch_grouped ?(semantics = 0) ?(fill = 0) ?filter (l : labels) (batch : Lacaml.S.mat) ~ef ~k :
  int array array * float array array * int array array * int array =
  let t = l.l_index in
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let lab = CArray.make int32_t (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_search_batch_grouped t.handle l.l_handle fh (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim)
           (addr p) (CArray.start ids) (CArray.start dist) (CArray.start lab) (from_voidp uint32_t null) (from_voidp uint32_t null)
           (CArray.start stage));
  let i, d, g = grouped_rows nq k ids dist lab in
  (i, d, g, Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s))

(* [brute_force_grouped l batch ~k] (hnsw_brute_force_batch_grouped): the exact form -- per label its nearest node under (distance,
   id) over all stored vectors, of those the k nearest.  Needs no graph. *)
let brute_force_grouped ?(fill = 0) ?filter (l : labels) (batch : Lacaml.S.mat) ~k :
  int array array * float array array * int array array =
  let t = l.l_index in
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let lab = CArray.make int32_t (max 1 (nq * k)) in
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_brute_force_batch_grouped t.handle l.l_handle fh (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim)
           (Int32.of_int k) (Int32.of_int fill) (CArray.start ids) (CArray.start dist) (CArray.start lab));
  grouped_rows nq k ids dist lab

(* [filters_by_label t labels ~n_labels] (hnsw_filter_create_by_label): n_labels filters from one label per node of the index;
   filter l allows node v iff labels.(v) = l, a label of -1 puts the node in no filter.  The labels are uploaded once and one
   pass over them on the device builds every mask.  Each filter is an ordinary [filter], freed with its own value. *)
let filters_by_label (t : t) (labels : int array) ~n_labels : filter array =
  let n = Array.length labels in
  let lab = CArray.make int32_t (max 1 n) in
  Array.iteri (fun v l -> CArray.set lab v (Int32.of_int l)) labels;
  let out = CArray.make filter_handle ~initial:null (max 1 n_labels) in
  check (hnsw_filter_create_by_label t.handle (CArray.start lab) (Int64.of_int n) (Int32.of_int n_labels) (CArray.start out));
  Array.init n_labels (fun l ->
      let f = { f_handle = CArray.get out l; f_index = t } in
      Gc.finalise (fun f -> ignore (hnsw_filter_destroy f.f_handle)) f;
      f)

(* [filter_bits f ~n] (hnsw_filter_bits): the mask of a filter of an index of n nodes as the device holds it, one bool per node *)
let filter_bits (f : filter) ~n : bool array =
  let words = CArray.make uint32_t ~initial:Unsigned.UInt32.zero (max 1 ((n + 31) / 32)) in
  check (hnsw_filter_bits f.f_handle (CArray.start words));
  Array.init n (fun v ->
      Unsigned.UInt32.logand (Unsigned.UInt32.shift_right (CArray.get words (v lsr 5)) (v land 31)) Unsigned.UInt32.one
      <> Unsigned.UInt32.zero)

(* [knn_batch_filtered_each filters which batch ~ef ~k] (hnsw_search_batch_filtered_each): query q (column q of [batch]) is
   answered under filters.(which.(q)); its row is the row [knn_batch_filtered] gives it under that filter.  A mixed batch of many
   tenants is one call.  All filters belong to one index.  -> as [knn_batch_filtered]. *)
let knn_batch_filtered_each ?(semantics = 0) ?(fill = 0) (filters : filter array) (which : int array) (batch : Lacaml.S.mat)
    ~ef ~k : int array array * float array array * int array =
  if Array.length filters = 0 then invalid_arg "knn_batch_filtered_each: no filters";
  let t = filters.(0).f_index in
  let nq = A2.dim2 batch in
  if Array.length which <> nq then invalid_arg "knn_batch_filtered_each: one filter position per query";
  let table = CArray.make filter_handle ~initial:null (Array.length filters) in
  Array.iteri (fun l f -> CArray.set table l f.f_handle) filters;
  let w = CArray.make int32_t (max 1 nq) in
  Array.iteri (fun q l -> CArray.set w q (Int32.of_int l)) which;
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_search_batch_filtered_each t.handle (CArray.start table) (Int32.of_int (Array.length filters)) (CArray.start w)
           (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) (addr p) (CArray.start ids) (CArray.start dist)
           (from_voidp uint32_t null) (from_voidp uint32_t null) (CArray.start stage));
  ignore (Sys.opaque_identity filters);      (* (alive until the call has returned) *)
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s))

(* Range search (hnsw_range_search_batch / hnsw_range_brute_force_batch): EVERY node within [radius] of each query (a column of
   [batch]).  -> per query its (node id, distance) pairs, ascending under (distance, node id), and its stage: how often W doubled
   before it was no longer saturated, -1 = the exact range scan.  Distances are over the float32 vectors whatever rows the index
   searches.  The device-side result is fetched whole and freed before the call returns. *)
let fetch_range (r : range_handle) : (int * float) array array * int array =
  Fun.protect ~finally:(fun () -> ignore (hnsw_range_result_destroy r)) (fun () ->
      let nq = allocate int64_t 0L and total = allocate int64_t 0L in
      check (hnsw_range_result_size r nq total);
      let nq = Int64.to_int !@nq and total = Int64.to_int !@total in
      let lims = CArray.make int64_t (nq + 1) in
      let ids = CArray.make int32_t (max 1 total) and dist = CArray.make float (max 1 total) in
      let stage = CArray.make uint32_t (max 1 nq) in
      check (hnsw_range_result_fetch r (CArray.start lims) (CArray.start ids) (CArray.start dist) (from_voidp uint32_t null)
               (from_voidp uint32_t null) (CArray.start stage));
      (Array.init nq (fun q ->
           let a = Int64.to_int (CArray.get lims q) and b = Int64.to_int (CArray.get lims (q + 1)) in
           Array.init (b - a) (fun j -> (Int32.to_int (CArray.get ids (a + j)), CArray.get dist (a + j)))),
       Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s)))

(* ~semantics: 0 Ohnsw's accept rule, 1 the functor's (2 is refused); ~ef: the ladder's first stage, 1..1024; ?filter
   (hnsw_range_search_batch_filtered): each segment is the unfiltered one with the nodes the filter does not allow left out, the
   stages are the unfiltered call's *)
let range_search ?(semantics = 0) ?(filter : filter option) (t : t) (batch : Lacaml.S.mat) ~radius ~ef
    : (int * float) array array * int array =
  let nq = A2.dim2 batch in
  let p = make range_params in
  setf p r_radius radius; setf p r_ef (Int32.of_int ef); setf p r_semantics (Int32.of_int semantics);
  let out = allocate range_handle null in
  (match filter with
   | None ->
     check (hnsw_range_search_batch t.handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) (addr p) out)
   | Some f ->
     check (hnsw_range_search_batch_filtered t.handle f.f_handle (bigarray_start array2 batch) (Int64.of_int nq)
              (Int64.of_int t.dim) (addr p) out);
     ignore (Sys.opaque_identity f));      (* (alive until the call has returned) *)
  fetch_range !@out

(* the exact form: per query the in-range prefix of the full order over all stored vectors; needs no graph *)
let brute_force_range ?(filter : filter option) (t : t) (batch : Lacaml.S.mat) ~radius : (int * float) array array =
  let nq = A2.dim2 batch in
  let out = allocate range_handle null in
  (match filter with
   | None ->
     check (hnsw_range_brute_force_batch t.handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) radius out)
   | Some f ->
     check (hnsw_range_brute_force_batch_filtered t.handle f.f_handle (bigarray_start array2 batch) (Int64.of_int nq)
              (Int64.of_int t.dim) radius out);
     ignore (Sys.opaque_identity f));
  fst (fetch_range !@out)

(* brute_force_knn_l2 (benchmark/dataset.ml:15-30) with its body on the device: the distance matrix it returns
   (k x nq: column q = the ascending distances of test vector q's k nearest train vectors), for an index that holds the
   train vectors.  The distances are the float32 bits the searches return, so Recall.compute's epsilon (benchmark/dataset.ml:
   105-127) compares like with like. *)
let brute_force_knn_l2 (t : t) (test : Lacaml.S.mat) ~k : Lacaml.S.mat =
  let _, dist = brute_force_knn t test ~k in
  let out = Lacaml.S.Mat.create k (A2.dim2 test) in
  Array.iteri (fun q row -> Array.iteri (fun j v -> out.{j + 1, q + 1} <- v) row) dist;
  out

(* Ohnsw.select_neighbours (lib/ohnsw.ml:647-663) for ONE base value: candidates as node ids (their distances to the
   target are recomputed on the device), at most ~num_neighbours kept, in selection order (nearest first).
   ~keep_all_if_few:true adds Hnsw_algo.SelectNeighbours' shortcut (lib/hnsw_algo.ml:596-599); ~degrees gives
   ~do_not_isolate:true (candidates of degree <= 1 are kept unconditionally, :591-592). *)
let select_neighbours ?(keep_all_if_few = false) ?degrees (t : t) (target : Lacaml.S.vec) ~(candidates : int list) ~num_neighbours : int list =
  let nc = List.length candidates in
  let cand = CArray.of_list int32_t (List.map Int32.of_int candidates) in
  let cnt = allocate int32_t (Int32.of_int nc) in
  let deg = match degrees with
    | Some l -> CArray.start (CArray.of_list int32_t (List.map Int32.of_int l))
    | None -> from_voidp int32_t null in
  let out = CArray.make int32_t (max 1 num_neighbours) and out_cnt = allocate int32_t 0l in
  check (hnsw_select_neighbours_batch t.handle (bigarray_start array1 target) 1L (Int64.of_int t.dim)
           (CArray.start cand) cnt (Int32.of_int (max 1 nc)) (Int32.of_int num_neighbours)
           (if keep_all_if_few then 1l else 0l) deg (CArray.start out) out_cnt);
  List.init (Int32.to_int !@out_cnt) (fun i -> Int32.to_int (CArray.get out i))

(* the device builder: the body of Ohnsw.build_batch_bigarray (lib/ohnsw.ml:840-857) in batches on the GPU
   (~max_batch:1 = Ohnsw.insert link for link); the OCaml builder stays the reference path, this is the fast one *)
let build ?(device = 0) ?(metric = 0) ?(seed = 0) ?(max_batch = 0) ?(batch_div = 0) ?(expected_ef = 0) ?(expected_semantics = 0) ~id_base ~num_connections
    ~num_nodes_search_construction (vectors : Lacaml.S.mat) : t =
  let dim = A2.dim1 vectors and n = A2.dim2 vectors in
  let b = make build_params in
  setf b b_num_connections (Int32.of_int num_connections); setf b b_efc (Int32.of_int num_nodes_search_construction);
  setf b b_metric (Int32.of_int metric); setf b b_id_base (Int32.of_int id_base);
  setf b b_seed (Unsigned.UInt64.of_int seed); setf b b_max_batch (Int32.of_int max_batch);
  setf b b_batch_div (Int32.of_int batch_div);
  setf b b_expected_ef (Int32.of_int expected_ef); setf b b_expected_semantics (Int32.of_int expected_semantics);
  let out = allocate index null in
  check (hnsw_build (bigarray_start array2 vectors) (Int64.of_int n) (Int32.of_int dim) (Int64.of_int dim) (addr b)
           (Int32.of_int device) out);
  let t = { handle = !@out; k_base = id_base; dim; scratch = Hashtbl.create 4 } in
  Gc.finalise (fun t -> ignore (hnsw_index_destroy t.handle)) t;
  t

(* Ohnsw.insert (lib/ohnsw.ml:766-837) for every column of [batch], in order, on the device (hnsw_index_insert), into an
   index the device owns (from [build] or [load]); returns the first new id (the others follow).  Levels are the device RNG's
   draws for those positions (the ones [build] with the same seed gives them), not OCaml's Random: an OCaml hgraph and a device
   index grown by inserts are two graphs, not one mirrored.  An index made from an OCaml hgraph ([of_ohnsw] / [of_ba]) is not
   grown here: the handle cache makes it again when the OCaml side inserts. *)
let insert_batch t (batch : Lacaml.S.mat) ~num_connections ~num_nodes_search_construction ?(seed = 0) ?(max_batch = 0)
    ?(batch_div = 0) ?(expected_ef = 0) ?(expected_semantics = 0) () : int =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  if A2.dim1 batch <> t.dim then invalid_arg "insert_batch: vectors of another dimension";
  let b = make build_params in
  setf b b_num_connections (Int32.of_int num_connections); setf b b_efc (Int32.of_int num_nodes_search_construction);
  setf b b_metric (getf inf ii_metric); setf b b_id_base (getf inf ii_id_base);
  setf b b_seed (Unsigned.UInt64.of_int seed); setf b b_max_batch (Int32.of_int max_batch);
  setf b b_batch_div (Int32.of_int batch_div);
  setf b b_expected_ef (Int32.of_int expected_ef); setf b b_expected_semantics (Int32.of_int expected_semantics);
  check (hnsw_index_insert t.handle (bigarray_start array2 batch) (Int64.of_int (A2.dim2 batch)) (Int64.of_int t.dim) (addr b));
  Int64.to_int (getf inf ii_n) + Int32.to_int (getf inf ii_id_base)

(* Hard deletion on the device (hnsw_index_remove): the stored nodes [ids] (id_base-based, distinct) leave the index, the others
   keep their order and are renumbered, the graph is repaired by the three-pass rule the header defines.  Returns the new id of
   every old node (id_base - 1 for a removed one).  As [insert_batch], for an index the device owns. *)
let remove_batch t (ids : int array) : int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n_old = Int64.to_int (getf inf ii_n) and m = Array.length ids in
  let c_ids = CArray.make int64_t (max m 1) and c_new = CArray.make int32_t (max n_old 1) in
  Array.iteri (fun i v -> CArray.set c_ids i (Int64.of_int v)) ids;
  check (hnsw_index_remove t.handle (CArray.start c_ids) (Int64.of_int m) (CArray.start c_new));
  Array.init n_old (fun v -> Int32.to_int (CArray.get c_new v))

(* Soft deletion owned by the index (hnsw_index_mark_deleted ...): the stored nodes [ids] (id_base-based, distinct) stay in the
   graph -- every walk still goes through them -- but no search returns them any more: while any node is marked the knn,
   brute-force and range searches answer under the mask of the live nodes, and new filters are ANDed with it.  [unmark_deleted]
   makes them live again; [compact] is [remove_batch] of the marked nodes (the new id of every old node, nothing marked after). *)
let change_marks call t (ids : int array) =
  let m = Array.length ids in
  let c_ids = CArray.make int64_t (max m 1) in
  Array.iteri (fun i v -> CArray.set c_ids i (Int64.of_int v)) ids;
  check (call t.handle (CArray.start c_ids) (Int64.of_int m))
let mark_deleted t (ids : int array) = change_marks hnsw_index_mark_deleted t ids
let unmark_deleted t (ids : int array) = change_marks hnsw_index_unmark_deleted t ids
let deleted_count t : int =
  let c = allocate int64_t 0L in
  check (hnsw_index_deleted_count t.handle c);
  Int64.to_int !@c
(* one bool per node: node v + id_base is marked *)
let deleted_mask t : bool array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n = Int64.to_int (getf inf ii_n) in
  let words = CArray.make uint32_t ~initial:Unsigned.UInt32.zero (max 1 ((n + 31) / 32)) in
  check (hnsw_index_deleted_bits t.handle (CArray.start words));
  Array.init n (fun v ->
      Unsigned.UInt32.logand (Unsigned.UInt32.shift_right (CArray.get words (v lsr 5)) (v land 31)) Unsigned.UInt32.one
      <> Unsigned.UInt32.zero)
let compact t : int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n_old = Int64.to_int (getf inf ii_n) in
  let c_new = CArray.make int32_t (max n_old 1) in
  check (hnsw_index_compact t.handle (CArray.start c_new));
  Array.init n_old (fun v -> Int32.to_int (CArray.get c_new v))

(* Keys the index owns (hnsw_index_set_keys ...): one caller-chosen key per stored node -- an OCaml int, every value legal,
   pairwise distinct -- kept on the device in row order and moved with the nodes through [insert_batch_keyed], [remove_batch] and
   [compact]; row numbers change with every removal, keys do not.  [set_keys t keys]: one key per node (a duplicate is refused
   naming the smallest duplicated key, the index keeps the keys it had).  [keys_of t ids]: the keys of nodes (id_base-based;
   [missing] where an id names no node, the searches' fill id -1 included); [keys_all t]: all of them in row order.
   [find_keys t keys]: the ids of the nodes with these keys, id_base - 1 where there is none. *)
let c_keys (keys : int array) =
  let c = CArray.make int64_t (max 1 (Array.length keys)) in
  Array.iteri (fun i v -> CArray.set c i (Int64.of_int v)) keys;
  c
let set_keys t (keys : int array) = check (hnsw_index_set_keys t.handle (CArray.start (c_keys keys)) (Int64.of_int (Array.length keys)))
let clear_keys t = check (hnsw_index_clear_keys t.handle)
let keys_info t : bool * int =
  let has = allocate int32_t 0l and bytes = allocate int64_t 0L in
  check (hnsw_index_keys_info t.handle has bytes);
  (!@has <> 0l, Int64.to_int !@bytes)
let keys_of ?(missing = -1) t (ids : int array) : int array =
  let m = Array.length ids in
  let c_ids = CArray.make int32_t (max 1 m) and out = CArray.make int64_t (max 1 m) in
  Array.iteri (fun i v -> CArray.set c_ids i (Int32.of_int v)) ids;
  check (hnsw_index_keys_of t.handle (CArray.start c_ids) (Int64.of_int m) (Int64.of_int missing) (CArray.start out));
  Array.init m (fun i -> Int64.to_int (CArray.get out i))
let keys_all t : int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n = Int64.to_int (getf inf ii_n) in
  let out = CArray.make int64_t (max 1 n) in
  check (hnsw_index_keys_of t.handle (from_voidp int32_t null) (Int64.of_int n) 0L (CArray.start out));
  Array.init n (fun i -> Int64.to_int (CArray.get out i))
let find_keys t (keys : int array) : int array =
  let m = Array.length keys in
  let out = CArray.make int64_t (max 1 m) in
  check (hnsw_index_find_keys t.handle (CArray.start (c_keys keys)) (Int64.of_int m) (CArray.start out));
  Array.init m (fun i -> Int64.to_int (CArray.get out i))

(* [knn_batch_keyed t batch ~ef ~k]: [knn_batch] answered in keys (hnsw_search_batch_keyed) -> (keys, distances, stages), [nq][k]
   ([missing] / nan where fewer than k were found).  ?filter: the rows of [knn_batch_filtered] under it; stages as there, 0 for the
   plain path.  One translate launch over the ids on the device, no second pass on the host. *)
let knn_batch_keyed ?(semantics = 0) ?(fill = 0) ?filter ?(missing = -1) (t : t) (batch : Lacaml.S.mat) ~ef ~k :
  int array array * float array array * int array =
  let nq = A2.dim2 batch in
  let keys = CArray.make int64_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_search_batch_keyed t.handle fh (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) (addr p)
           (Int64.of_int missing) (CArray.start keys) (CArray.start dist) (from_voidp uint32_t null) (from_voidp uint32_t null)
           (CArray.start stage));
  (Array.init nq (fun q -> Array.init k (fun j -> Int64.to_int (CArray.get keys (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s))

(* Search by stored item (hnsw_search_batch_by_id ...): the stored vectors of the nodes [ids] (id_base-based: a search's output can be
   fed straight back) are the queries, gathered on the device -- only the ids cross the link.  [exclude_self] (the default): the
   search runs k + 1 wide with ef' = max(ef, k + 1) and each row loses the node's own id, the first k entries if it is not among
   them; [~exclude_self:false]: exactly [knn_batch] over the stored rows.  -> (ids, distances), [nq][k] (-1 / nan where fewer were
   found).  [knn_batch_by_key]: the same for the nodes stored under [keys], answered in keys; an absent key refuses the call.
   [brute_force_by_id]: the exact form.  [knn_graph t ~ef ~k]: the row of [knn_batch_by_id] (?exact: of [brute_force_by_id]) of
   every node, computed on the device in chunks (option "graph_chunk_rows"). *)
let by_id_params ~semantics ~fill ~ef ~k =
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  p
let c_ids32 (ids : int array) =
  let c = CArray.make int32_t (max 1 (Array.length ids)) in
  Array.iteri (fun i v -> CArray.set c i (Int32.of_int v)) ids;
  c
let knn_batch_by_id ?(semantics = 0) ?(fill = 0) ?(exclude_self = true) (t : t) (ids : int array) ~ef ~k :
  int array array * float array array =
  let nq = Array.length ids in
  let out = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let p = by_id_params ~semantics ~fill ~ef ~k in
  check (hnsw_search_batch_by_id t.handle (CArray.start (c_ids32 ids)) (Int64.of_int nq) (addr p) (if exclude_self then 1l else 0l)
           (CArray.start out) (CArray.start dist) (from_voidp uint32_t null) (from_voidp uint32_t null));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get out (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))
let knn_batch_by_key ?(semantics = 0) ?(fill = 0) ?(exclude_self = true) ?(missing = -1) (t : t) (keys : int array) ~ef ~k :
  int array array * float array array =
  let nq = Array.length keys in
  let out = CArray.make int64_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let p = by_id_params ~semantics ~fill ~ef ~k in
  check (hnsw_search_batch_by_key t.handle (CArray.start (c_keys keys)) (Int64.of_int nq) (addr p) (if exclude_self then 1l else 0l)
           (Int64.of_int missing) (CArray.start out) (CArray.start dist) (from_voidp uint32_t null) (from_voidp uint32_t null));
  (Array.init nq (fun q -> Array.init k (fun j -> Int64.to_int (CArray.get out (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))
let brute_force_by_id ?(fill = 0) ?(exclude_self = true) (t : t) (ids : int array) ~k : int array array * float array array =
  let nq = Array.length ids in
  let out = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  check (hnsw_brute_force_batch_by_id t.handle (CArray.start (c_ids32 ids)) (Int64.of_int nq) (Int32.of_int k) (Int32.of_int fill)
           (if exclude_self then 1l else 0l) (CArray.start out) (CArray.start dist));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get out (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))
let knn_graph ?(semantics = 0) ?(fill = 0) ?(exact = false) (t : t) ~ef ~k : int array array * float array array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n = Int64.to_int (getf inf ii_n) in
  let out = CArray.make int32_t (max 1 (n * k)) and dist = CArray.make float (max 1 (n * k)) in
  let p = by_id_params ~semantics ~fill ~ef ~k in
  check (hnsw_knn_graph t.handle (addr p) (if exact then 1l else 0l) (CArray.start out) (CArray.start dist));
  (Array.init n (fun v -> Array.init k (fun j -> Int32.to_int (CArray.get out (v * k + j)))),
   Array.init n (fun v -> Array.init k (fun j -> CArray.get dist (v * k + j))))

(* Paged search (hnsw_search_batch_after, hnsw_brute_force_batch_after): the NEXT k after a cursor.  A cursor is the (distance, id)
   of the last result the caller holds; [cursor_start] is before every node.  The order is (distance, id) over the returned float
   distances.  [knn_batch_after t batch ~ef ~k]: ?after one cursor per query (default: the first page) -> (ids, distances, next,
   stages): W grows ef, 2 ef, ... 1024 until it holds k nodes after the cursor (stages.(q) = how often it doubled), a query still
   short gets the exact paged scan (-1); next.(q) is the cursor to hand back for the page after, and a row with fewer than k real
   entries means "exhausted".  ?filter: only allowed nodes count.  [brute_force_after]: the exact form, one pass over the table per
   page, no graph needed.  Cursors do not survive [remove], [compact] or an upsert: those renumber the nodes. *)
let cursor_start : float * int = (neg_infinity, Int32.to_int Int32.min_int)
let c_cursors (after : (float * int) array option) nq =
  let c = CArray.make cursor (max 1 nq) in
  (match after with
   | Some a ->
     if Array.length a <> nq then invalid_arg "after: one cursor per query";
     Array.iteri (fun q (d, i) -> let e = CArray.get c q in setf e cu_dist d; setf e cu_id (Int32.of_int i); CArray.set c q e) a
   | None ->
     for q = 0 to nq - 1 do
       let e = CArray.get c q in
       setf e cu_dist (fst cursor_start); setf e cu_id Int32.min_int; CArray.set c q e
     done);
  c
let cursors_out c nq = Array.init nq (fun q -> let e = CArray.get c q in (getf e cu_dist, Int32.to_int (getf e cu_id)))
let knn_batch_after ?(semantics = 0) ?(fill = 0) ?filter ?after (t : t) (batch : Lacaml.S.mat) ~ef ~k :
  int array array * float array array * (float * int) array * int array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) and next = CArray.make cursor (max 1 nq) in
  let p = by_id_params ~semantics ~fill ~ef ~k in
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_search_batch_after t.handle fh (CArray.start (c_cursors after nq)) (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int t.dim) (addr p) (CArray.start ids) (CArray.start dist) (CArray.start next) (from_voidp uint32_t null)
           (from_voidp uint32_t null) (CArray.start stage));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   cursors_out next nq,
   Array.init nq (fun q -> let s = Unsigned.UInt32.to_int (CArray.get stage q) in if s = 0xFFFFFFFF then -1 else s))
let brute_force_after ?(fill = 0) ?filter ?after (t : t) (batch : Lacaml.S.mat) ~k :
  int array array * float array array * (float * int) array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let next = CArray.make cursor (max 1 nq) in
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_brute_force_batch_after t.handle fh (CArray.start (c_cursors after nq)) (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int t.dim) (Int32.of_int k) (Int32.of_int fill) (CArray.start ids) (CArray.start dist) (CArray.start next));
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   cursors_out next nq)

(* Diversified search (hnsw_diversify_batch, hnsw_search_batch_diverse, hnsw_brute_force_batch_diverse): greedy maximal marginal
   relevance.  [diversify t queries ~candidates ~k ~lambda]: k of ITS candidates per query ([rerank]'s lists); pick 1 is the nearest,
   every further pick minimises lambda * distance - (1 - lambda) * distance to the nearest node already picked, ties to the
   candidate [rerank] ranks first -> (ids, distances, diversities) in SELECTION order; past a query's candidates id -1, nan;
   diversities.(q).(j) is the distance to the nearest earlier pick at the moment of selection (infinity for pick 1).  lambda = 1.
   is [rerank].  [knn_batch_diverse t batch ~ef ~k ~pool ~lambda]: the search at k := pool (?filter: the filtered search), then
   [diversify] over its rows without leaving the device; k <= pool <= ef.  [brute_force_diverse]: the same over the exact scan,
   k <= pool <= 1024, no graph needed. *)
let rows3 nq k ids dist div =
  (Array.init nq (fun q -> Array.init k (fun j -> Int32.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get div (q * k + j))))
let diversify ?(fill = 0) (t : t) (queries : Lacaml.S.mat) ~(candidates : int array array) ~k ~lambda :
  int array array * float array array * float array array =
  let nq = A2.dim2 queries in
  if Array.length candidates <> nq then invalid_arg "diversify: one candidate list per query";
  let stride = Array.fold_left (fun m row -> max m (Array.length row)) 1 candidates in
  let cand = CArray.make int32_t ~initial:(Int32.of_int (t.k_base - 1)) (max 1 (nq * stride)) in
  Array.iteri (fun q row -> Array.iteri (fun j v -> CArray.set cand (q * stride + j) (Int32.of_int v)) row) candidates;
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let div = CArray.make float (max 1 (nq * k)) in
  check (hnsw_diversify_batch t.handle (bigarray_start array2 queries) (Int64.of_int nq) (Int64.of_int t.dim)
           (CArray.start cand) (Int32.of_int stride) (Int32.of_int k) lambda (Int32.of_int fill) (CArray.start ids) (CArray.start dist)
           (CArray.start div));
  rows3 nq k ids dist div
let knn_batch_diverse ?(semantics = 0) ?(fill = 0) ?filter (t : t) (batch : Lacaml.S.mat) ~ef ~k ~pool ~lambda :
  int array array * float array array * float array array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let div = CArray.make float (max 1 (nq * k)) in
  let p = by_id_params ~semantics ~fill ~ef ~k in
  let fh = match filter with Some (f : filter) -> f.f_handle | None -> null in
  check (hnsw_search_batch_diverse t.handle fh (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) (addr p)
           (Int32.of_int pool) lambda (CArray.start ids) (CArray.start dist) (CArray.start div) (from_voidp uint32_t null)
           (from_voidp uint32_t null) (from_voidp uint32_t null));
  rows3 nq k ids dist div
let brute_force_diverse ?(fill = 0) (t : t) (batch : Lacaml.S.mat) ~k ~pool ~lambda :
  int array array * float array array * float array array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int32_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let div = CArray.make float (max 1 (nq * k)) in
  check (hnsw_brute_force_batch_diverse t.handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int t.dim) (Int32.of_int k)
           (Int32.of_int pool) lambda (Int32.of_int fill) (CArray.start ids) (CArray.start dist) (CArray.start div));
  rows3 nq k ids dist div

(* [insert_batch_keyed t batch keys]: [insert_batch] into an index that owns keys (hnsw_index_insert_keyed), keys.(i) naming
   column i of [batch].  A stored or repeated key refuses the call before anything is built; an empty index without keys starts
   its keys here.  Plain [insert_batch] is refused on an index with keys.  Returns the first new id. *)
let insert_batch_keyed t (batch : Lacaml.S.mat) (keys : int array) ~num_connections ~num_nodes_search_construction ?(seed = 0)
    ?(max_batch = 0) ?(batch_div = 0) ?(expected_ef = 0) ?(expected_semantics = 0) () : int =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  if A2.dim1 batch <> t.dim then invalid_arg "insert_batch_keyed: vectors of another dimension";
  if Array.length keys <> A2.dim2 batch then invalid_arg "insert_batch_keyed: one key per vector";
  let b = make build_params in
  setf b b_num_connections (Int32.of_int num_connections); setf b b_efc (Int32.of_int num_nodes_search_construction);
  setf b b_metric (getf inf ii_metric); setf b b_id_base (getf inf ii_id_base);
  setf b b_seed (Unsigned.UInt64.of_int seed); setf b b_max_batch (Int32.of_int max_batch);
  setf b b_batch_div (Int32.of_int batch_div);
  setf b b_expected_ef (Int32.of_int expected_ef); setf b b_expected_semantics (Int32.of_int expected_semantics);
  check (hnsw_index_insert_keyed t.handle (bigarray_start array2 batch) (Int64.of_int (A2.dim2 batch)) (Int64.of_int t.dim)
           (CArray.start (c_keys keys)) (addr b));
  Int64.to_int (getf inf ii_n) + Int32.to_int (getf inf ii_id_base)

(* [upsert_batch_keyed t batch keys]: replace or add vectors by key in one all-or-nothing call (hnsw_index_upsert_keyed): column i of
   [batch] becomes the vector under keys.(i), stored or not.  The index afterwards is exactly what [remove_keys] of the stored ones
   among [keys] followed by [insert_batch_keyed t batch keys] leaves, with one table swap and one epoch step; on any error it is
   exactly as before.  Two equal keys in the call are refused.  Returns (replaced, new_id): replaced.(i) = keys.(i) was stored;
   new_id as [remove_batch] returns it (id_base - 1 for a replaced node). *)
let upsert_build_params inf ~num_connections ~num_nodes_search_construction ~seed ~max_batch ~batch_div ~expected_ef ~expected_semantics =
  let b = make build_params in
  setf b b_num_connections (Int32.of_int num_connections); setf b b_efc (Int32.of_int num_nodes_search_construction);
  setf b b_metric (getf inf ii_metric); setf b b_id_base (getf inf ii_id_base);
  setf b b_seed (Unsigned.UInt64.of_int seed); setf b b_max_batch (Int32.of_int max_batch);
  setf b b_batch_div (Int32.of_int batch_div);
  setf b b_expected_ef (Int32.of_int expected_ef); setf b b_expected_semantics (Int32.of_int expected_semantics);
  b
let upsert_batch_keyed t (batch : Lacaml.S.mat) (keys : int array) ~num_connections ~num_nodes_search_construction ?(seed = 0)
    ?(max_batch = 0) ?(batch_div = 0) ?(expected_ef = 0) ?(expected_semantics = 0) () : bool array * int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  if A2.dim1 batch <> t.dim then invalid_arg "upsert_batch_keyed: vectors of another dimension";
  let m = A2.dim2 batch in
  if Array.length keys <> m then invalid_arg "upsert_batch_keyed: one key per vector";
  let b = upsert_build_params inf ~num_connections ~num_nodes_search_construction ~seed ~max_batch ~batch_div ~expected_ef ~expected_semantics in
  let n_old = Int64.to_int (getf inf ii_n) in
  let c_rep = CArray.make uint8_t (max m 1) and c_new = CArray.make int32_t (max n_old 1) in
  check (hnsw_index_upsert_keyed t.handle (bigarray_start array2 batch) (CArray.start (c_keys keys)) (Int64.of_int m) (Int64.of_int t.dim)
           (addr b) (CArray.start c_rep) (CArray.start c_new));
  (Array.init m (fun i -> Unsigned.UInt8.to_int (CArray.get c_rep i) <> 0), Array.init n_old (fun v -> Int32.to_int (CArray.get c_new v)))

(* [update_batch t ids batch]: the same for an index without keys (hnsw_index_update): the stored nodes [ids] (id_base-based,
   distinct) are replaced by the columns of [batch]: exactly [remove_batch t ids] followed by [insert_batch t batch].  An index with
   keys is refused.  Returns new_id as [remove_batch] does. *)
let update_batch t (ids : int array) (batch : Lacaml.S.mat) ~num_connections ~num_nodes_search_construction ?(seed = 0)
    ?(max_batch = 0) ?(batch_div = 0) ?(expected_ef = 0) ?(expected_semantics = 0) () : int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  if A2.dim1 batch <> t.dim then invalid_arg "update_batch: vectors of another dimension";
  let m = A2.dim2 batch in
  if Array.length ids <> m then invalid_arg "update_batch: one id per vector";
  let b = upsert_build_params inf ~num_connections ~num_nodes_search_construction ~seed ~max_batch ~batch_div ~expected_ef ~expected_semantics in
  let n_old = Int64.to_int (getf inf ii_n) in
  let c_ids = CArray.make int64_t (max m 1) and c_new = CArray.make int32_t (max n_old 1) in
  Array.iteri (fun i v -> CArray.set c_ids i (Int64.of_int v)) ids;
  check (hnsw_index_update t.handle (CArray.start c_ids) (bigarray_start array2 batch) (Int64.of_int m) (Int64.of_int t.dim) (addr b)
           (CArray.start c_new));
  Array.init n_old (fun v -> Int32.to_int (CArray.get c_new v))

(* [remove_keys] / [mark_deleted_keys] / [unmark_deleted_keys]: [remove_batch] / [mark_deleted] / [unmark_deleted] of the nodes
   with these keys; an absent key refuses the call and nothing is changed.  [filter_by_keys]: an ordinary [filter] that allows
   exactly those nodes. *)
let remove_keys t (keys : int array) : int array =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n_old = Int64.to_int (getf inf ii_n) in
  let c_new = CArray.make int32_t (max n_old 1) in
  check (hnsw_index_remove_keys t.handle (CArray.start (c_keys keys)) (Int64.of_int (Array.length keys)) (CArray.start c_new));
  Array.init n_old (fun v -> Int32.to_int (CArray.get c_new v))
let mark_deleted_keys t (keys : int array) = change_marks hnsw_index_mark_deleted_keys t keys
let unmark_deleted_keys t (keys : int array) = change_marks hnsw_index_unmark_deleted_keys t keys
let filter_by_keys (t : t) (keys : int array) : filter =
  let out = allocate filter_handle null in
  check (hnsw_filter_create_by_keys t.handle (CArray.start (c_keys keys)) (Int64.of_int (Array.length keys)) out);
  let f = { f_handle = !@out; f_index = t } in
  Gc.finalise (fun f -> ignore (hnsw_filter_destroy f.f_handle)) f;
  f

(* flattened-index file (the reference has no persistence: lib/hnsw.ml:348, lib/ohnsw.ml:312 derive sexp with opaque values) *)
let save (t : t) (path : string) = check (hnsw_index_save t.handle path)
let load ?(device = 0) ~id_base ~dim (path : string) : t =
  let out = allocate index null in
  check (hnsw_index_load path (Int32.of_int device) out);
  let t = { handle = !@out; k_base = id_base; dim; scratch = Hashtbl.create 4 } in
  Gc.finalise (fun t -> ignore (hnsw_index_destroy t.handle)) t;
  t

(* Hgraph.Stats (lib/hnsw.ml:353-375) of one layer: (layer size, min, max, mean degree, number of isolated nodes) *)
let stats (t : t) ~layer : int * int * int * float * int =
  let s = make layer_stats in
  check (hnsw_index_layer_stats t.handle (Int32.of_int layer) (addr s));
  (Int64.to_int (getf s ls_num_nodes), Int32.to_int (getf s ls_min_degree), Int32.to_int (getf s ls_max_degree),
   getf s ls_mean_degree, Int64.to_int (getf s ls_num_isolated))

(* mima.isolated of one layer (lib/hnsw.ml:357,364-366): the nodes without a neighbour, in the reference's list order
   (descending: consed during the ascending Map.fold) *)
let isolated (t : t) ~layer : int list =
  let cnt = allocate int64_t 0L in
  check (hnsw_index_layer_isolated t.handle (Int32.of_int layer) (from_voidp int64_t null) 0L cnt);
  let c = Int64.to_int !@cnt in
  if c = 0 then [] else begin
    let ids = CArray.make int64_t c in
    check (hnsw_index_layer_isolated t.handle (Int32.of_int layer) (CArray.start ids) (Int64.of_int c) cnt);
    List.map Int64.to_int (CArray.to_list ids)
  end

(* the permutation of 0 .. n-1 behind the option "visited_blocks" (hnsw_index_locality_codes): introspection only.  The
   library writes the INDEX's n codes: the length comes from the handle, never from the caller *)
let locality_codes (t : t) : (int32, Bigarray.int32_elt, Bigarray.c_layout) A1.t =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let out = A1.create Bigarray.int32 Bigarray.c_layout (max 1 (Int64.to_int (getf inf ii_n))) in
  check (hnsw_index_locality_codes t.handle (bigarray_start array1 out));
  out

(* the sq8 copy of the index (option "sq8_rows"): (lo, scale) and the codes, one row of d bytes per node; Invalid_argument when
   the index has no such copy *)
let sq8_params (t : t) : float * float =
  let lo = allocate float 0.0 and scale = allocate float 0.0 in
  check (hnsw_index_sq8_params t.handle lo scale);
  (!@ lo, !@ scale)
let sq8_codes (t : t) : (int, Bigarray.int8_unsigned_elt, Bigarray.c_layout) Bigarray.Array2.t =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let out = Bigarray.Array2.create Bigarray.int8_unsigned Bigarray.c_layout (max 1 (Int64.to_int (getf inf ii_n))) t.dim in
  check (hnsw_index_sq8_codes t.handle (to_voidp (bigarray_start array2 out)));
  out

(* the per-dimension sq8 copy of the index (option "sq8_dim_rows"): (lo, scale), d values each, and the codes, one row of d bytes
   per node; Invalid_argument when the index has no such copy *)
let sq8_dim_params (t : t) : float array * float array =
  let lo = CArray.make float t.dim and scale = CArray.make float t.dim in
  check (hnsw_index_sq8_dim_params t.handle (CArray.start lo) (CArray.start scale));
  (Array.of_list (CArray.to_list lo), Array.of_list (CArray.to_list scale))
let sq8_dim_codes (t : t) : (int, Bigarray.int8_unsigned_elt, Bigarray.c_layout) Bigarray.Array2.t =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let out = Bigarray.Array2.create Bigarray.int8_unsigned Bigarray.c_layout (max 1 (Int64.to_int (getf inf ii_n))) t.dim in
  check (hnsw_index_sq8_dim_codes t.handle (to_voidp (bigarray_start array2 out)));
  out

(* the 1-bit copy of the index (option "bit_rows"): the d thresholds (bit i of a row is x_i > t_i), and the codes, one row of
   ceil(d/32) words per node, dimension i in bit (i mod 32) of word (i / 32); Invalid_argument while the option is off *)
let bit_params (t : t) : float array =
  let thr = CArray.make float t.dim in
  check (hnsw_index_bit_params t.handle (CArray.start thr));
  Array.of_list (CArray.to_list thr)
let bit_codes (t : t) : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array2.t =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let out = Bigarray.Array2.create Bigarray.int32 Bigarray.c_layout (max 1 (Int64.to_int (getf inf ii_n))) ((t.dim + 31) / 32) in
  check (hnsw_index_bit_codes t.handle (to_voidp (bigarray_start array2 out)));
  out

(* the codes in -7..7 that the walk over the bit rows uses for [queries] (one query per row, t.dim columns) under option
   "bit_query_bits" 4: one row of t.dim codes per query; Invalid_argument while option "bit_rows" is off *)
let bit_query_codes (t : t) (queries : (float, Bigarray.float32_elt, Bigarray.c_layout) Bigarray.Array2.t)
    : (int, Bigarray.int8_signed_elt, Bigarray.c_layout) Bigarray.Array2.t =
  let nq = Bigarray.Array2.dim1 queries in
  if Bigarray.Array2.dim2 queries <> t.dim then invalid_arg "Hnsw_mi355x.bit_query_codes: dimension mismatch";
  let out = Bigarray.Array2.create Bigarray.int8_signed Bigarray.c_layout (max 1 nq) t.dim in
  if nq > 0 then
    check (hnsw_index_bit_query_codes t.handle (bigarray_start array2 queries) (Int64.of_int nq) (Int64.of_int t.dim)
             (to_voidp (bigarray_start array2 out)));
  out

(* ?metric of [create], [build], [of_ohnsw], [of_ba] and [sharded_build]: HNSW_METRIC_L2, _IP, _COSINE.  A cosine index stores
   N(X) and normalises every query batch itself: callers hand it unnormalised vectors everywhere. *)
let metric_l2 = 0
let metric_ip = 1
let metric_cosine = 2

(* N(X) (hnsw_normalise_batch): the columns of [x] scaled to unit length by the normaliser the C header defines, as a fresh
   matrix, and their norms; a zero column stays zero, one whose sum of squares is not finite becomes nan *)
let normalise ?(device = 0) (x : Lacaml.S.mat) : Lacaml.S.mat * Lacaml.S.vec =
  let dim = A2.dim1 x and n = A2.dim2 x in
  let out = Lacaml.S.Mat.create dim n and norms = Lacaml.S.Vec.create (max 1 n) in
  check (hnsw_normalise_batch (Int32.of_int device) (bigarray_start array2 x) (Int64.of_int n) (Int32.of_int dim) (Int64.of_int dim)
           (bigarray_start array2 out) (Int64.of_int dim) (bigarray_start array1 norms));
  (out, norms)

(* the float32 vectors the index holds (hnsw_index_get_rows), one column per node in id order: for [metric_cosine] N(X) *)
let rows (t : t) : Lacaml.S.mat =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n = Int64.to_int (getf inf ii_n) in
  let out = Lacaml.S.Mat.create t.dim (max 1 n) in
  check (hnsw_index_get_rows t.handle (from_voidp int64_t null) (Int64.of_int n) (bigarray_start array2 out) (Int64.of_int t.dim));
  out

(* everything the first search with this ef (and accept rule) would do once -- the visited-structure decision, the kernel's
   residency, its code object -- now (hnsw_index_prepare); [create ~expected_ef] / [build ~expected_ef] call it themselves *)
let prepare ?(semantics = 0) (t : t) ~ef : unit =
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k 1l; setf p p_fill 0l; setf p p_semantics (Int32.of_int semantics);
  check (hnsw_index_prepare t.handle (addr p))

(* 0: searches at this ef use the tag cache; else log2 of the bitmap-block slots (hnsw_index_visited_blocks) *)
let visited_blocks ?(semantics = 0) (t : t) ~ef : int =
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k 1l; setf p p_fill 0l; setf p p_semantics (Int32.of_int semantics);
  let out = allocate int32_t 0l in
  check (hnsw_index_visited_blocks t.handle (addr p) out);
  Int32.to_int !@out

(* Hgraph.Stats.compute (lib/hnsw.ml:370-375) as the reference's record: per layer (size, {min; max; mean; isolated}) *)
let stats_compute (t : t) ~max_layer : (int * (int * int * float * int list)) list =
  List.init (max_layer + 1) (fun layer ->
      let (size, mi, ma, mean, _) = stats t ~layer in
      (size, (mi, ma, mean, isolated t ~layer)))

(* Page-lock a query or result matrix a benchmark loop passes again and again (benchmark/benchmark.ml:86-98): the
   copies of knn_batch* then run at PCIe speed.  The CALLER keeps the Bigarray reachable until [unpin] -- the library
   never registers memory on its own. *)
let pin (m : (_, _, _) A2.t) = check (hnsw_host_register (to_voidp (bigarray_start array2 m)) (Int64.of_int (A2.size_in_bytes m)))
let unpin (m : (_, _, _) A2.t) = check (hnsw_host_unregister (to_voidp (bigarray_start array2 m)))

(* the graph of a device index as a [flat] (the input of unflatten_ohnsw / unflatten_ba): e.g. an index built on the
   device with [build], handed back to the OCaml builder so that Ohnsw.insert can go on from there *)
let export (t : t) : flat =
  let inf = make index_info in
  check (hnsw_index_get_info t.handle (addr inf));
  let n = Int64.to_int (getf inf ii_n) and max_layer = Int32.to_int (getf inf ii_max_layer) in
  let width0 = Int32.to_int (getf inf ii_max_degree0) and width_upper = max 1 (Int32.to_int (getf inf ii_max_degree)) in
  let deg0 = A1.create Bigarray.int32 Bigarray.c_layout n in
  let nbr0 = A2.create Bigarray.int32 Bigarray.c_layout n width0 in
  check (hnsw_index_export_layer0 t.handle (bigarray_start array1 deg0) (bigarray_start array2 nbr0));
  let upper = Array.init max_layer (fun l ->
      let cnt = allocate int64_t 0L in
      check (hnsw_index_export_upper_count t.handle (Int32.of_int (l + 1)) cnt);
      let c = Int64.to_int !@cnt in
      let nodes = A1.create Bigarray.int64 Bigarray.c_layout c in
      let deg = A1.create Bigarray.int32 Bigarray.c_layout c in
      let nbr = A2.create Bigarray.int32 Bigarray.c_layout c width_upper in
      if c > 0 then
        check (hnsw_index_export_upper t.handle (Int32.of_int (l + 1)) (bigarray_start array1 nodes)
                 (bigarray_start array1 deg) (bigarray_start array2 nbr));
      (nodes, deg, nbr)) in
  { deg0; nbr0; upper; max_layer; width0; width_upper; entry_point = Int64.to_int (getf inf ii_entry_point) }

(* ---- sharded index (hnsw_sharded_*, see the C header): the ROWS partitioned over several GPUs, one graph per slice, every query
   on all slices, the per-slice answers merged on the first device under (distance, global id).  Global ids are 64-bit on the C
   side; an OCaml int holds them. *)
type sharded_handle = unit ptr
let sharded_handle : sharded_handle typ = ptr void
let hnsw_sharded_build =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_build"
    (ptr float @-> int64_t @-> int32_t @-> int64_t @-> ptr build_params @-> ptr int32_t @-> int32_t @-> ptr sharded_handle
     @-> returning int32_t)
let hnsw_sharded_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_create"
    (ptr (ptr index_desc) @-> ptr int32_t @-> int32_t @-> ptr sharded_handle @-> returning int32_t)
let hnsw_sharded_load =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_load"
    (ptr string @-> ptr int32_t @-> int32_t @-> ptr sharded_handle @-> returning int32_t)
let hnsw_sharded_destroy = foreign ~from:lib "hnsw_sharded_destroy" (sharded_handle @-> returning int32_t)
let hnsw_sharded_num_shards = foreign ~from:lib "hnsw_sharded_num_shards" (sharded_handle @-> ptr int32_t @-> returning int32_t)
let hnsw_sharded_shard =
  foreign ~from:lib "hnsw_sharded_shard" (sharded_handle @-> int32_t @-> ptr index @-> ptr int64_t @-> returning int32_t)
let hnsw_sharded_get_info =
  foreign ~from:lib "hnsw_sharded_get_info"
    (sharded_handle @-> ptr int64_t @-> ptr int32_t @-> ptr int32_t @-> ptr int32_t @-> ptr int64_t @-> returning int32_t)
let hnsw_sharded_set_option =
  foreign ~from:lib "hnsw_sharded_set_option" (sharded_handle @-> string @-> int64_t @-> returning int32_t)
let hnsw_sharded_search_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_search_batch"
    (sharded_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int64_t @-> ptr float
     @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_sharded_brute_force_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_brute_force_batch"
    (sharded_handle @-> ptr float @-> int64_t @-> int64_t @-> int32_t @-> int32_t @-> ptr int64_t @-> ptr float @-> returning int32_t)
let hnsw_merge_lists =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_merge_lists"
    (int32_t @-> ptr int32_t @-> ptr float @-> ptr int64_t @-> int32_t @-> int64_t @-> int32_t @-> int32_t @-> int32_t @-> int32_t
     @-> ptr int64_t @-> ptr float @-> returning int32_t)

type sharded = { s_handle : sharded_handle; s_dim : int; s_base : int }

(* hnsw_sharded_build: shard g = [build] of the columns [floor(n g / G), floor(n (g + 1) / G)) of [vectors] on devices.(g) with
   seed + g; a device may be listed more than once *)
let sharded_build ~(devices : int array) ?(metric = 0) ?(seed = 0) ?(max_batch = 0) ?(batch_div = 0) ?(expected_ef = 0)
    ?(expected_semantics = 0) ~id_base ~num_connections ~num_nodes_search_construction (vectors : Lacaml.S.mat) : sharded =
  let dim = A2.dim1 vectors and n = A2.dim2 vectors in
  let b = make build_params in
  setf b b_num_connections (Int32.of_int num_connections); setf b b_efc (Int32.of_int num_nodes_search_construction);
  setf b b_metric (Int32.of_int metric); setf b b_id_base (Int32.of_int id_base);
  setf b b_seed (Unsigned.UInt64.of_int seed); setf b b_max_batch (Int32.of_int max_batch);
  setf b b_batch_div (Int32.of_int batch_div);
  setf b b_expected_ef (Int32.of_int expected_ef); setf b b_expected_semantics (Int32.of_int expected_semantics);
  let dev = CArray.of_list int32_t (List.map Int32.of_int (Array.to_list devices)) in
  let out = allocate sharded_handle null in
  check (hnsw_sharded_build (bigarray_start array2 vectors) (Int64.of_int n) (Int32.of_int dim) (Int64.of_int dim) (addr b)
           (CArray.start dev) (Int32.of_int (Array.length devices)) out);
  let s = { s_handle = !@out; s_dim = dim; s_base = id_base } in
  Gc.finalise (fun s -> ignore (hnsw_sharded_destroy s.s_handle)) s;
  s

(* hnsw_sharded_set_option: the option on every shard; a refusal leaves every shard as it was *)
let sharded_set_option (s : sharded) name (value : int) = check (hnsw_sharded_set_option s.s_handle name (Int64.of_int value))

let sharded_rows nq k ids dist =
  (Array.init nq (fun q -> Array.init k (fun j -> Int64.to_int (CArray.get ids (q * k + j)))),
   Array.init nq (fun q -> Array.init k (fun j -> CArray.get dist (q * k + j))))

(* hnsw_sharded_search_batch: for each query (a column of [batch]) the first k under (distance, global id) of the shards' own knn
   rows for (ef, k).  -> (global ids, distances), both [nq][k]; past the real entries: id -1, distance nan. *)
let sharded_knn_batch (s : sharded) (batch : Lacaml.S.mat) ~ef ~k : int array array * float array array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int64_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill 0l; setf p p_semantics 0l;
  check (hnsw_sharded_search_batch s.s_handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int s.s_dim) (addr p)
           (CArray.start ids) (CArray.start dist) (from_voidp uint32_t null) (from_voidp uint32_t null));
  sharded_rows nq k ids dist

(* hnsw_sharded_brute_force_batch: the exact k nearest of ALL rows, the distance bits of [brute_force_knn] over one index of them *)
let sharded_brute_force (s : sharded) (batch : Lacaml.S.mat) ~k : int array array * float array array =
  let nq = A2.dim2 batch in
  let ids = CArray.make int64_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  check (hnsw_sharded_brute_force_batch s.s_handle (bigarray_start array2 batch) (Int64.of_int nq) (Int64.of_int s.s_dim)
           (Int32.of_int k) 0l (CArray.start ids) (CArray.start dist));
  sharded_rows nq k ids dist

(* hnsw_merge_lists: lists.(g).(q) = list g's (id, distance) pairs for query q, ascending under (distance, id), at most k_in of
   them; first_row.(g) = the global row of list g's local node 0 (non-decreasing).  -> the first k_out of the union under
   (distance, first_row.(g) + id) as (global ids, distances), both [nq][k_out]; past the real entries: id -1, distance nan. *)
let merge_lists ?(device = 0) ?(id_base = 0) ~(first_row : int array) ~k_in ~k_out (lists : (int * float) array array array)
  : int array array * float array array =
  let n_lists = Array.length lists in
  if n_lists <> Array.length first_row then invalid_arg "merge_lists: one first_row per list";
  let nq = if n_lists = 0 then 0 else Array.length lists.(0) in
  let ids = CArray.make int32_t ~initial:(Int32.of_int (id_base - 1)) (max 1 (n_lists * nq * k_in)) in
  let dist = CArray.make float ~initial:0.0 (max 1 (n_lists * nq * k_in)) in
  Array.iteri (fun g per_query ->
      if Array.length per_query <> nq then invalid_arg "merge_lists: every list answers the same queries";
      Array.iteri (fun q row ->
          if Array.length row > k_in then invalid_arg "merge_lists: a row longer than k_in";
          Array.iteri (fun j (v, d) ->
              CArray.set ids ((g * nq + q) * k_in + j) (Int32.of_int v); CArray.set dist ((g * nq + q) * k_in + j) d) row) per_query) lists;
  let first = CArray.of_list int64_t (List.map Int64.of_int (Array.to_list first_row)) in
  let out_ids = CArray.make int64_t (max 1 (nq * k_out)) and out_dist = CArray.make float (max 1 (nq * k_out)) in
  check (hnsw_merge_lists (Int32.of_int device) (CArray.start ids) (CArray.start dist) (CArray.start first) (Int32.of_int n_lists)
           (Int64.of_int nq) (Int32.of_int k_in) (Int32.of_int k_out) (Int32.of_int id_base) 0l (CArray.start out_ids)
           (CArray.start out_dist));
  sharded_rows nq k_out out_ids out_dist

(* ---- sharded index: a filter over the global rows, filtered search, range search (see the C header).  Not bound for a sharded
   index, because the library does not build them: filters from labels and one filter per query. *)
type sharded_filter_handle = unit ptr
let sharded_filter_handle : sharded_filter_handle typ = ptr void
type sharded_range_handle = unit ptr
let sharded_range_handle : sharded_range_handle typ = ptr void
let hnsw_sharded_filter_create =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_filter_create"
    (sharded_handle @-> ptr uint32_t @-> int64_t @-> ptr sharded_filter_handle @-> returning int32_t)
let hnsw_sharded_filter_destroy = foreign ~from:lib "hnsw_sharded_filter_destroy" (sharded_filter_handle @-> returning int32_t)
let hnsw_sharded_filter_count =
  foreign ~from:lib "hnsw_sharded_filter_count" (sharded_filter_handle @-> ptr int64_t @-> returning int32_t)
let hnsw_sharded_filter_part =
  foreign ~from:lib "hnsw_sharded_filter_part" (sharded_filter_handle @-> int32_t @-> ptr filter_handle @-> returning int32_t)
let hnsw_sharded_search_batch_filtered =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_search_batch_filtered"
    (sharded_handle @-> sharded_filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr search_params @-> ptr int64_t
     @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t @-> returning int32_t)
let hnsw_sharded_range_search_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_range_search_batch"
    (sharded_handle @-> sharded_filter_handle @-> ptr float @-> int64_t @-> int64_t @-> ptr range_params
     @-> ptr sharded_range_handle @-> returning int32_t)
let hnsw_sharded_range_brute_force_batch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_range_brute_force_batch"
    (sharded_handle @-> sharded_filter_handle @-> ptr float @-> int64_t @-> int64_t @-> float @-> ptr sharded_range_handle
     @-> returning int32_t)
let hnsw_sharded_range_result_size =
  foreign ~from:lib "hnsw_sharded_range_result_size" (sharded_range_handle @-> ptr int64_t @-> ptr int64_t @-> returning int32_t)
let hnsw_sharded_range_result_fetch =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_sharded_range_result_fetch"
    (sharded_range_handle @-> ptr int64_t @-> ptr int64_t @-> ptr float @-> ptr uint32_t @-> ptr uint32_t @-> ptr uint32_t
     @-> returning int32_t)
let hnsw_sharded_range_result_device =
  foreign ~from:lib "hnsw_sharded_range_result_device"
    (sharded_range_handle @-> ptr (ptr int64_t) @-> ptr (ptr int64_t) @-> ptr (ptr float) @-> returning int32_t)
let hnsw_sharded_range_result_destroy =
  foreign ~from:lib "hnsw_sharded_range_result_destroy" (sharded_range_handle @-> returning int32_t)
let hnsw_merge_segments =
  foreign ~from:lib ~release_runtime_lock:true "hnsw_merge_segments"
    (int32_t @-> int32_t @-> int64_t @-> ptr (ptr int64_t) @-> ptr (ptr int32_t) @-> ptr (ptr float) @-> ptr int64_t @-> int32_t
     @-> ptr sharded_range_handle @-> returning int32_t)

(* A mask over the GLOBAL rows of a sharded index (hnsw_sharded_filter_create): allow.(v) = global row v may be returned; one entry
   per row of the whole table.  The library cuts it into one filter per shard.  The filter keeps its index alive. *)
type sharded_filter = { sf_handle : sharded_filter_handle; sf_index : sharded }

let sharded_filter_create (s : sharded) (allow : bool array) : sharded_filter =
  let n = Array.length allow in
  let words = (n + 31) / 32 in
  let bits = CArray.make uint32_t ~initial:Unsigned.UInt32.zero (max 1 words) in
  Array.iteri (fun v a ->
      if a then CArray.set bits (v lsr 5) (Unsigned.UInt32.logor (CArray.get bits (v lsr 5)) (Unsigned.UInt32.shift_left Unsigned.UInt32.one (v land 31))))
    allow;
  let out = allocate sharded_filter_handle null in
  check (hnsw_sharded_filter_create s.s_handle (CArray.start bits) (Int64.of_int n) out);
  let f = { sf_handle = !@out; sf_index = s } in
  Gc.finalise (fun f -> ignore (hnsw_sharded_filter_destroy f.sf_handle)) f;
  f

(* the allowed rows, summed over the shards *)
let sharded_filter_count (f : sharded_filter) : int =
  let c = allocate int64_t 0L in
  check (hnsw_sharded_filter_count f.sf_handle c);
  Int64.to_int !@c

let stage_of s = let s = Unsigned.UInt32.to_int s in if s = 0xFFFFFFFF then -1 else s

(* hnsw_sharded_search_batch_filtered: the first k under (distance, global id) of the shards' own [knn_batch_filtered] rows.
   -> (global ids, distances, stages); stages.(q) = the maximum over the shards, -1 as soon as one shard took its exact scan. *)
let sharded_knn_batch_filtered ?(semantics = 0) ?(fill = 0) (f : sharded_filter) (batch : Lacaml.S.mat) ~ef ~k :
  int array array * float array array * int array =
  let s = f.sf_index in
  let nq = A2.dim2 batch in
  let ids = CArray.make int64_t (max 1 (nq * k)) and dist = CArray.make float (max 1 (nq * k)) in
  let stage = CArray.make uint32_t (max 1 nq) in
  let p = make search_params in
  setf p p_ef (Int32.of_int ef); setf p p_k (Int32.of_int k); setf p p_fill (Int32.of_int fill);
  setf p p_semantics (Int32.of_int semantics);
  check (hnsw_sharded_search_batch_filtered s.s_handle f.sf_handle (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int s.s_dim) (addr p) (CArray.start ids) (CArray.start dist) (from_voidp uint32_t null)
           (from_voidp uint32_t null) (CArray.start stage));
  let rows, dists = sharded_rows nq k ids dist in
  (rows, dists, Array.init nq (fun q -> stage_of (CArray.get stage q)))

(* a sharded range result fetched whole and freed: per query its (global id, distance) pairs, ascending under (distance, global
   id), and its stage (the maximum over the shards, -1 = an exact scan) *)
let fetch_sharded_range (r : sharded_range_handle) : (int * float) array array * int array =
  Fun.protect ~finally:(fun () -> ignore (hnsw_sharded_range_result_destroy r)) (fun () ->
      let nq = allocate int64_t 0L and total = allocate int64_t 0L in
      check (hnsw_sharded_range_result_size r nq total);
      let nq = Int64.to_int !@nq and total = Int64.to_int !@total in
      let lims = CArray.make int64_t (nq + 1) in
      let ids = CArray.make int64_t (max 1 total) and dist = CArray.make float (max 1 total) in
      let stage = CArray.make uint32_t (max 1 nq) in
      check (hnsw_sharded_range_result_fetch r (CArray.start lims) (CArray.start ids) (CArray.start dist) (from_voidp uint32_t null)
               (from_voidp uint32_t null) (CArray.start stage));
      (Array.init nq (fun q ->
           let a = Int64.to_int (CArray.get lims q) and b = Int64.to_int (CArray.get lims (q + 1)) in
           Array.init (b - a) (fun j -> (Int64.to_int (CArray.get ids (a + j)), CArray.get dist (a + j)))),
       Array.init nq (fun q -> stage_of (CArray.get stage q))))

let sharded_filter_arg = function None -> null | Some (f : sharded_filter) -> f.sf_handle

(* hnsw_sharded_range_search_batch: per query the union of the shards' own [range_search] segments; ?filter: under the shards'
   parts of a sharded filter *)
let sharded_range_search ?(semantics = 0) ?(filter : sharded_filter option) (s : sharded) (batch : Lacaml.S.mat) ~radius ~ef
  : (int * float) array array * int array =
  let nq = A2.dim2 batch in
  let p = make range_params in
  setf p r_radius radius; setf p r_ef (Int32.of_int ef); setf p r_semantics (Int32.of_int semantics);
  let out = allocate sharded_range_handle null in
  check (hnsw_sharded_range_search_batch s.s_handle (sharded_filter_arg filter) (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int s.s_dim) (addr p) out);
  ignore (Sys.opaque_identity filter);      (* (alive until the call has returned) *)
  fetch_sharded_range !@out

(* hnsw_sharded_range_brute_force_batch: the exact form, the set [brute_force_range] gives over one index of all rows *)
let sharded_brute_force_range ?(filter : sharded_filter option) (s : sharded) (batch : Lacaml.S.mat) ~radius
  : (int * float) array array * int array =
  let nq = A2.dim2 batch in
  let out = allocate sharded_range_handle null in
  check (hnsw_sharded_range_brute_force_batch s.s_handle (sharded_filter_arg filter) (bigarray_start array2 batch) (Int64.of_int nq)
           (Int64.of_int s.s_dim) radius out);
  ignore (Sys.opaque_identity filter);
  fetch_sharded_range !@out

(* hnsw_merge_segments: lists.(g).(q) = list g's whole segment for query q as (id, distance) pairs, ascending under (distance,
   id); first_row.(g) = the global row of list g's local node 0 (non-decreasing).  -> per query the union of its segments under
   (distance, first_row.(g) + id); the same global id in two lists: the lower list first. *)
let merge_segments ?(device = 0) ?(id_base = 0) ~(first_row : int array) (lists : (int * float) array array array)
  : (int * float) array array =
  let n_lists = Array.length lists in
  if n_lists <> Array.length first_row then invalid_arg "merge_segments: one first_row per list";
  let nq = if n_lists = 0 then 0 else Array.length lists.(0) in
  let per_list = Array.map (fun per_query ->
      if Array.length per_query <> nq then invalid_arg "merge_segments: every list answers the same queries";
      let total = Array.fold_left (fun a row -> a + Array.length row) 0 per_query in
      let lims = CArray.make int64_t ~initial:0L (nq + 1) in
      let ids = CArray.make int32_t (max 1 total) and dist = CArray.make float (max 1 total) in
      let at = ref 0 in
      Array.iteri (fun q row ->
          Array.iter (fun (v, d) -> CArray.set ids !at (Int32.of_int v); CArray.set dist !at d; incr at) row;
          CArray.set lims (q + 1) (Int64.of_int !at)) per_query;
      (lims, ids, dist)) lists in
  let pl = CArray.make (ptr int64_t) (max 1 n_lists) and pi = CArray.make (ptr int32_t) (max 1 n_lists)
  and pd = CArray.make (ptr float) (max 1 n_lists) in
  Array.iteri (fun g (l, i, d) -> CArray.set pl g (CArray.start l); CArray.set pi g (CArray.start i); CArray.set pd g (CArray.start d))
    per_list;
  let first = CArray.of_list int64_t (List.map Int64.of_int (Array.to_list first_row)) in
  let out = allocate sharded_range_handle null in
  check (hnsw_merge_segments (Int32.of_int device) (Int32.of_int n_lists) (Int64.of_int nq) (CArray.start pl) (CArray.start pi)
           (CArray.start pd) (CArray.start first) (Int32.of_int id_base) out);
  ignore (Sys.opaque_identity per_list);    (* (alive until the call has returned) *)
  fst (fetch_sharded_range !@out)
