/*
 * hnsw_mi355x.h -- C ABI of libhnsw_mi355x.so: the MI355X (gfx950) HNSW search path.
 *
 * Drop-in boundary for ONE path of lehy/ocaml-hnsw: batched k-NN search = greedy upper-layer
 * descent + ef-bounded best-first expansion on layer 0.  The reference has no FFI of its own
 * (it is 100 % OCaml); each entry point below names the OCaml function whose BODY it replaces
 * while the OCaml signature stays (see INTEGRATION.md for the ctypes binding):
 *
 *   hnsw_index_create        flatten + upload of Ohnsw.Hgraph.t (lib/ohnsw.ml:307-312, iterated
 *                            with Graph.iter_neighbours :176-180) or Hnsw.Ba.Hgraph.t
 *                            (lib/hnsw.ml:342-351, fold_layers) plus the vectors (value:
 *                            lib/ohnsw.ml:842, lib/hnsw.ml:313)
 *   hnsw_search_batch        Ohnsw.knn_batch_bigarray (lib/ohnsw.ml:877-897)
 *                            Hnsw.Ba.knn_batch / MakeBatch.knn_batch (lib/hnsw.ml:769-777)
 *   hnsw_knn                 Ohnsw.knn (lib/ohnsw.ml:859-875), Hnsw.Ba.knn (lib/hnsw.ml:763-767),
 *                            Hnsw_algo.Knn.knn (lib/hnsw_algo.ml:990-1011)
 *   hnsw_search_layer_batch  Ohnsw.search_k (lib/ohnsw.ml:543-588), Hnsw_algo.Search.search
 *                            (lib/hnsw_algo.ml:350-391): one layer, explicit start nodes
 *   hnsw_search_one_batch    Ohnsw.search_one (lib/ohnsw.ml:492-512), Search.search_one
 *                            (lib/hnsw_algo.ml:393-437)
 *   hnsw_search_batch_h2d    the same call with host queries in and DEVICE results out (per-rank step of a
 *                            one-process-per-GPU deployment: results are exchanged between devices first)
 *   hnsw_search_submit/_wait the same batch call in two halves (several batches in flight)
 *   hnsw_multi_*             the batch entry point over several GPUs from one host process (RCCL all-gather)
 *   hnsw_sharded_*           (nothing in the reference) the ROWS partitioned over several GPUs, one graph per slice, every query
 *                            on all slices, the answers merged on the device (hnsw_merge_lists): capacity where hnsw_multi is rate;
 *                            also under a filter over the global rows and as range search (hnsw_merge_segments)
 *   hnsw_distance_batch      Ohnsw.distance_l2 / EuclideanBa.distance (lib/ohnsw.ml:899,
 *                            lib/hnsw.ml:809-815) as timed by bench_dist/bench_dist.ml:22-33
 *   hnsw_index_layer_stats / hnsw_index_layer_isolated   Hgraph.Stats.compute (lib/hnsw.ml:353-375)
 *   hnsw_select_neighbours_batch  Ohnsw.select_neighbours (lib/ohnsw.ml:647-663),
 *                            Hnsw_algo.SelectNeighbours.select_neighbours (lib/hnsw_algo.ml:572-609)
 *   hnsw_build               Ohnsw.build_batch_bigarray (lib/ohnsw.ml:840-857), batched on the device
 *   hnsw_index_insert        Ohnsw.insert (lib/ohnsw.ml:766-837) of m vectors into an index the library holds
 *   hnsw_index_remove        hard deletion (new: the reference never forgets a vector): nodes out, graph repaired on the device
 *   hnsw_brute_force_batch   brute_force_knn_l2 (benchmark/dataset.ml:15-30): the exact scan recall is measured against
 *   hnsw_rerank_batch        (nothing in the reference) the k nearest of caller-given candidates over the float32 vectors:
 *                            the refine step of the half-row searches (option "refine")
 *   hnsw_search_batch_filtered  (nothing in the reference) the k nearest AMONG the nodes an allow-mask names (hnsw_filter_create):
 *                            several tenants, categories or time windows in one index; a mask of live nodes = soft deletes
 *   hnsw_search_batch_filtered_each  ... with one filter per query: a mixed batch of many tenants in one call
 *                            (hnsw_filter_create_by_label: the tenants' filters from one label per node)
 *   hnsw_range_search_batch  (nothing in the reference) EVERY node within a radius of the query, a result of variable length;
 *                            hnsw_range_brute_force_batch is its exact form; the _filtered forms of both answer under an allow-mask
 *   hnsw_index_mark_deleted  (nothing in the reference) soft deletion owned by the index: mark a node now, every search goes
 *                            around it; hnsw_index_compact pays for the repair (hnsw_index_remove of the marked nodes) later
 *   hnsw_host_alloc / hnsw_host_register   (nothing in the reference) page-locked query / result matrices,
 *                            which the entry points above read and write from the device in place
 *
 * Plain pointers and sizes only.  All host buffers stay owned by the caller and are not
 * retained after a call returns (OCaml Bigarrays are not moved by the GC, so they can be passed
 * for the duration of a call).  One thread at a time per handle.
 *
 * Search semantics (identical to the reference's imperative path, with its heap tie order --
 * which the reference leaves to an un-vendored library -- fixed to the total order
 * (distance, node id)):
 *   - descent on layers max_layer..1: Ohnsw.search_one_simple (lib/ohnsw.ml:492-508);
 *   - layer 0: Ohnsw.search_k (lib/ohnsw.ml:543-588) with W bounded by ef: a neighbour is
 *     accepted iff |W| < ef or d < max(W).d (strict, :574); neighbours of an expanded node are
 *     tested in adjacency-row order (:570); the search stops when the nearest unexpanded
 *     candidate is farther than max(W) (:568);
 *   - the result is W[0..k), ascending.  (Hnsw.Nearest.nearest_k, lib/hnsw.ml:522-525, returns
 *     the k FARTHEST of W when ef > k; that defect is not reproduced.)  k > ef is rejected.
 */
#ifndef HNSW_MI355X_H
#define HNSW_MI355X_H

#include <math.h>   /* INFINITY: HNSW_CURSOR_START */
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point, a structure or a documented behaviour changes; the Python and OCaml loaders refuse a library
 * that answers another number (hnsw_abi_version).
 *   2  (round 5) hnsw_index_locality_codes and the option "visited_blocks"; hnsw_host_unregister / hnsw_host_free wait for
 *      asynchronous readers and refuse pointers that are not theirs (HNSW_ERR_BAD_ARG); and, since version 1 was first cut:
 *      hnsw_search_batch_h2d, hnsw_host_alloc / hnsw_host_free, hnsw_index_layer_isolated, hnsw_multi_debug_counters,
 *      hnsw_index_info.row_format (was `reserved`), hnsw_index_layer_stats' values for a layer without nodes
 *      (min 1000000, max -1, mean nan: the reference's fold), Hgraph.stats()['isolated'] a list of ids
 *   3  (round 6) hnsw_index_desc.expected_ef / expected_semantics and hnsw_build_params.expected_ef / expected_semantics (the
 *      structures GROW: a caller compiled against version 2 passes too short a structure), hnsw_index_prepare; the index file
 *      (hnsw_index_save, format 2) also carries the locality codes and the prepared shapes' decisions, hnsw_index_load applies
 *      them (format 1 files still load); W in three and six key registers (ef 129..192, 257..384: no interface change);
 *      hnsw_multi_search_batch* abort their communicators when an exchange is refused part-way */
#define HNSW_ABI_VERSION 3

typedef struct hnsw_index hnsw_index;

/* Error convention: 0 = ok, negative = error; the message is in hnsw_last_error().
 * The OCaml shim maps BAD_ARG / EMPTY_INDEX / DEGREE_OVERFLOW to Invalid_argument (as
 * "knn: empty hgraph", lib/ohnsw.ml:862) and the rest to Failure. */
enum {
    HNSW_OK = 0,
    HNSW_ERR_BAD_ARG = -1,
    HNSW_ERR_EMPTY_INDEX = -2,     /* Invalid_argument "knn: empty hgraph" */
    HNSW_ERR_DEGREE_OVERFLOW = -3, /* a neighbour list longer than its row: never truncated */
    HNSW_ERR_NO_DEVICE = -4,
    HNSW_ERR_HIP = -5,
    HNSW_ERR_OOM = -6,
    HNSW_ERR_UNSUPPORTED = -7
};

enum { HNSW_METRIC_L2 = 0,  /* sqrt(sum (a_i-b_i)^2)                                     */
       HNSW_METRIC_IP = 1,  /* 1 - <a,b>  (new: the reference has Euclidean only,
                               benchmark/dataset.ml:6-13; extension point = DISTANCE sig) */
       HNSW_METRIC_COSINE = 2 };/* 1 - <a,b> / (|a| |b|): the index normalises what it is handed (below) */

/* ---- cosine distance as a metric the index owns ---------------------------------------------------------------------------------
 * THE NORMALISER N.  N(x) is a float32 row that is a function of the row's d values only -- not of its row number, stride,
 * alignment, batch size or of where the matrix lies (device memory, a page-locked host matrix read in place):
 *   s = <x,x> summed in float32 on the distance kernels' own lane grid: with NCH = the smallest of 1, 2, 4, 8, 16 that is
 *       >= ceil(ceil(d / 4) / 16), lane l (0..15) starts from 0 and adds, for i = 0 .. NCH - 1 in this order, the four values of
 *       chunk c = 16 i + l (dimensions 4c .. 4c + 3, in this order; dimensions >= d count as 0), each as one fused multiply-add
 *       acc = fma(v, v, acc); the 16 partial sums p are then added as p[j] += p[j + 8 mod 16]; p[j] += p[j + 4 mod 16];
 *       p[j] += p[j + 2 mod 16]; p[j] += p[j + 1 mod 16] (the order of every distance of this library);
 *   norm = sqrt(s), correctly rounded;  N(x)_i = x_i / norm, one correctly rounded division each.
 *   A row whose sum of squares is 0 becomes all zeros, its norm reads 0, and its cosine distance to everything is 1.
 *   A row whose sum of squares is NaN or infinite becomes all NaN (its norm reads as s).
 * hnsw_normalise_batch is N as an operator of its own (it needs no index): host arrays in ([n][in_stride], in_stride >= d) and out
 *   ([n][out_stride], out_stride >= d; only the d values of a row are written), out_norms [n] or NULL.  out may be in with the
 *   same stride (in == out with different strides: HNSW_ERR_BAD_ARG); otherwise the two arrays must not overlap.  n == 0 is
 *   HNSW_OK; d in 1..1024, d > 1024: HNSW_ERR_UNSUPPORTED; a null in / out, n < 0, d < 1 or a stride < d: HNSW_ERR_BAD_ARG.
 *
 * THE TWIN CONTRACT.  A COSINE index over X answers every call on queries Q with exactly the bits (ids, distances, counters,
 * stages, graph links) of an IP index over N(X) called with N(Q).  What follows from it:
 *   * the index stores N(X) as its float32 rows; the rows as handed over are not kept on the device.  hnsw_index_get_rows returns
 *     what a handle holds;
 *   * hnsw_index_create, hnsw_build and hnsw_index_insert normalise the data they are handed and refuse the whole call, all or
 *     nothing, with HNSW_ERR_BAD_ARG when a data row's sum of squares is not finite (the message names the first such row);
 *     zero rows are accepted.  hnsw_index_insert takes params->metric = HNSW_METRIC_COSINE, as the index's;
 *   * every call that takes queries or targets (the knn searches in all their forms, hnsw_distance_batch, the exact scans,
 *     hnsw_rerank_batch, the filtered and the range calls, the layer operators, hnsw_select_neighbours_batch, the sharded calls)
 *     normalises them exactly once, on the device, on the call's stream, into scratch of the handle: the caller's matrix is
 *     not written.  A host call reads a page-locked matrix in place for that and then runs on the device-resident copy: it takes
 *     no head split (option "head_queries" has no effect).  The device forms keep one scratch matrix of the batch's size per
 *     caller stream they have been called on, for the life of the handle (as the ordering pre-pass keeps its block): a caller
 *     that makes a stream per request grows the handle with every new stream -- reuse a few streams.  A batch larger than any
 *     before on its stream allocates (hipMalloc) inside the call, so a COSINE device form cannot be recorded by a stream capture
 *     unless a call of that size on that stream came before it;
 *   * hnsw_index_save writes the stored rows with metric 2 (the file format stays 2); on hnsw_index_load the rows are not
 *     normalised again: N(N(x)) is not N(x) bit for bit;
 *   * hnsw_index_info.metric and hnsw_sharded_get_info report 2; the shards of an hnsw_sharded agree on it as on any metric;
 *   * options "split_rows", "half_rows", "sq8_rows", "refine", "visited_blocks", "filter_collect" behave as for the IP twin
 *     (byte rows only where N(X) happens to be byte-valued, as for the twin);
 *   * NOT BUILT: hnsw_multi.  hnsw_multi_create refuses a COSINE desc with HNSW_ERR_UNSUPPORTED, "cosine: not built for hnsw_multi".
 *
 * hnsw_index_get_rows: the stored float32 rows of the m nodes ids[0..m) (id_base-based; ids NULL: all n rows in order, m must be n)
 *   into the host array out ([m][out_stride], out_stride >= d; d values per row written).  For every metric and row format (the
 *   float32 table is always there); for COSINE it is N(X).  An id out of range, m < 0, a null out (m > 0) or out_stride < d:
 *   HNSW_ERR_BAD_ARG and nothing is written.  m == 0 is HNSW_OK. */
int32_t hnsw_normalise_batch(int32_t device, const float *in, int64_t n, int32_t d, int64_t in_stride, float *out, int64_t out_stride,
                             float *out_norms /* may be NULL */);
int32_t hnsw_index_get_rows(const hnsw_index *idx, const int64_t *ids /* NULL: all n rows in order, m must be n */, int64_t m,
                            float *out, int64_t out_stride);

enum { HNSW_FILL_OHNSW = 0, /* missing results: id -1, distance NaN  (lib/ohnsw.ml:880-881) */
       HNSW_FILL_BA = 1 };  /* missing results: id -1, distance +inf (lib/hnsw.ml:771)      */

/* One upper layer (l >= 1) as a sparse list of the nodes present in it. */
typedef struct hnsw_layer_desc {
    int64_t n_nodes;
    const int64_t *nodes; /* [n_nodes] node ids (id_base-based), any order                  */
    const int32_t *deg;   /* [n_nodes]                                                      */
    const int32_t *nbr;   /* [n_nodes][max_degree] ids (id_base-based) in the reference's
                             iteration order (Neighbours.iter / fold); entries >= deg ignored */
} hnsw_layer_desc;

typedef struct hnsw_index_desc {
    const float *vectors; /* [n][row_stride] fp32: a Lacaml.S.mat (dim x n, Fortran layout)  */
    int64_t n;
    int32_t d;
    int64_t row_stride;   /* floats between consecutive vectors (>= d)                       */
    int32_t metric;       /* HNSW_METRIC_*                                                   */
    int32_t id_base;      /* 0 for Ohnsw (lib/ohnsw.ml:159), 1 for Hnsw.Ba (lib/hnsw.ml:325) */
    int32_t max_degree0;  /* row width of nbr0 = Mmax0 = 2M (lib/hnsw.ml:719, ohnsw.ml:818)  */
    int32_t max_degree;   /* row width of upper rows = Mmax = M                              */
    int32_t max_layer;    /* number of upper layers                                          */
    int64_t entry_point;  /* id_base-based; id_base-1 (or any value < id_base) = empty index */
    const int32_t *deg0;  /* [n]                                                             */
    const int32_t *nbr0;  /* [n][max_degree0], reference iteration order                     */
    const hnsw_layer_desc *upper; /* [max_layer]; upper[l-1] describes layer l               */
    /* Optional (0 = not known): the ef (~num_neighbours_search; Ohnsw: k) and accept rule (HNSW_SEM_*) the index will be searched
     * with.  When given, hnsw_index_create does NOW, once, what the first search with these parameters would otherwise do inside
     * the call (hnsw_index_prepare below): construction is where the reference's benchmark pays one-time costs too
     * (benchmark/benchmark.ml:66-80 before :89-96).  A value the library cannot serve (ef > 1024) is ignored here and
     * reported by the search. */
    int32_t expected_ef;
    int32_t expected_semantics;
} hnsw_index_desc;

/* Which accept rule W uses (they differ only when a neighbour is exactly as far as max(W)):
 * OHNSW   = accept iff |W| < ef or d < max(W).d (Ohnsw.search_k, lib/ohnsw.ml:574): a tied neighbour
 *           is dropped.
 * FUNCTOR = Nearest.insert_distance (lib/hnsw.ml:494-506) with the in-tree heap's merge
 *           (lib/hnsw_algo.ml:25-31): d < max(W).d replaces the maximum; d == max(W).d is answered
 *           Inserted -- the neighbour enters VisitMe and IS expanded later (lib/hnsw_algo.ml:360-364) --
 *           but W keeps the incumbent; d > max(W).d is Too_far.  Use it for Hnsw.Ba / Hnsw_algo.Knn.knn.
 * What neither mode takes from the reference is the ORDER a heap yields equal keys in (Core_kernel.Heap
 * on the imperative path: un-vendored; the in-tree pairing heap on the functor path: shape dependent):
 * equal distances are popped / evicted in node-id order.  Against the pairing-heap restatement the
 * functor mode's full ef-sized distance profile (and the ids up to the farthest class) agree on 2699 of
 * the 2700 query runs of the tie-heavy suites of tests/test_gpu_functor_ties.py; the residual (suite
 * "levels8", ef 16, query 82) is such an order effect (profiles/r02_functor_tie_agreement.txt). */
enum { HNSW_SEM_OHNSW = 0, HNSW_SEM_FUNCTOR = 1,
       /* FUNCTOR, and the result is what Hnsw.Nearest.nearest_k (lib/hnsw.ml:522-525) returns: when
        * ef > k that is the k FARTHEST members of W, nearest of those first -- the reference's
        * actual behaviour of Hnsw.Ba.knn / knn_batch with ~num_neighbours_search > ~num_neighbours,
        * a defect its author's notes acknowledge.  For callers that want that output reproduced;
        * knn entry points only. */
       HNSW_SEM_FUNCTOR_NEAREST_K = 2 };

typedef struct hnsw_search_params {
    int32_t ef;   /* ~num_neighbours_search (lib/hnsw.ml:763); Ohnsw: ef == k (ohnsw.ml:859) */
    int32_t k;    /* ~num_neighbours / ~k                                                    */
    int32_t fill; /* HNSW_FILL_*                                                             */
    int32_t semantics; /* HNSW_SEM_*                                                         */
} hnsw_search_params;

enum { HNSW_ROWS_F32 = 0,   /* the float32 rows as handed over                                              */
       HNSW_ROWS_BYTES = 2, /* lossless byte copy (every value an integer in 0..255)                         */
       HNSW_ROWS_SPLIT = 3, /* float32 rows whose last 16 / 32 bytes past a 128-byte line are stored beside the
                               neighbour in the layer-0 adjacency (option "split_rows")                      */
       HNSW_ROWS_HALF = 4,  /* the values rounded to fp16 (option "half_rows"): NOT the search over the float32
                               vectors but the exact search over X rounded to fp16                          */
       HNSW_ROWS_SQ8 = 5,   /* 8-bit codes under one affine map (option "sq8_rows"): the walk is the exact search
                               over the codes, the answer its candidates re-ranked over the float32 vectors  */
       HNSW_ROWS_SQ8_DIM = 6, /* 8-bit codes under one affine map PER DIMENSION (option "sq8_dim_rows"): the walk is
                               the exact search over Z = codes * s, the answer re-ranked over the float32 vectors */
       HNSW_ROWS_BITS = 7 }; /* one bit per dimension (option "bit_rows"): the walk runs under Hamming distance over the
                               bits x_i > t_i, the answer is its candidates re-ranked over the float32 vectors */

typedef struct hnsw_index_info {
    int64_t n;
    int32_t d, metric, id_base, max_degree0, max_degree, max_layer;
    int64_t entry_point;
    int64_t device_bytes;      /* HBM held by the index                                       */
    int64_t row_stride_bytes;  /* padded vector row on the device                             */
    int32_t device;
    int32_t row_format;        /* HNSW_ROWS_*: what the knn searches read right now (options "byte_rows", "split_rows",
                                  "half_rows", "sq8_rows", "sq8_dim_rows") */
} hnsw_index_info;

int32_t hnsw_abi_version(void);
const char *hnsw_last_error(void);
int32_t hnsw_device_count(int32_t *count);

/* Copies vectors and graph to `device` (HBM); validates ids and degrees (never truncates).
 * An empty graph (no entry point) creates a valid handle whose searches fail with
 * HNSW_ERR_EMPTY_INDEX, like the reference. */
int32_t hnsw_index_create(const hnsw_index_desc *desc, int32_t device, hnsw_index **out);
int32_t hnsw_index_destroy(hnsw_index *idx);
int32_t hnsw_index_get_info(const hnsw_index *idx, hnsw_index_info *info);
/* Knobs that never change results:
 *   "vt_bits"       log2 entries of the per-query LDS visited cache (0 = automatic);
 *   "order_queries" a batch of more than half the queries the device holds at once is searched longest
 *                   walk first (a descent pre-pass + a sort decide the order; per-query results are
 *                   unchanged, the long walks start first and the launch's drain phase gets shorter):
 *                   -1 = automatic (default), 0 = never, 1 = always;
 *   "head_queries"  hnsw_search_batch on a page-locked query matrix, where the batch would be ordered and is a plain
 *                   knn walk (no "refine", no "sq8_rows"): the first H rows of the batch are searched unordered by a
 *                   launch of their own on a second stream, whose waves fetch their queries over the link themselves,
 *                   while the pre-pass of the other rows waits for the link; the two parts join at the end of the
 *                   call.  -1 = automatic (default: batches of at least 1.2 times the queries the device holds at once
 *                   give 0.3 to 0.5 of their rows to the head), 0 = never, > 0 = H (at most nq - 1).  Ignored by every
 *                   other call;
 *   "time_kernels"  1 = bracket the launches of every hnsw_search_batch_device call with HIP events
 *                   on the caller's stream (read back with hnsw_index_kernel_times).  A hnsw_search_batch call that
 *                   splits off a head ("head_queries") times its other rows: the pre-pass and the search figure
 *                   are theirs, the head's launch runs beside both on its own stream -- bytes of ALL nq queries
 *                   over that search figure read high by about nq / (nq - H);
 *   "lds_pad"       LDS bytes a search workgroup asks for beyond its own (how many queries a CU holds
 *                   at once in a batch larger than the device holds): -1 = automatic (default);
 *   "scan_slabs"    into how many row slabs hnsw_brute_force_batch cuts the table (1..1024; 0 = automatic, the default);
 *   "byte_rows"     when every value of the vectors is an integer in 0..255 (SIFT descriptors stored as
 *                   float32) the index keeps a second, lossless copy of the rows as bytes and the knn
 *                   searches read that one: each byte is converted back to the float it came from and
 *                   the arithmetic is unchanged, so distances are bit-identical for a quarter of the
 *                   bytes gathered.  1 = use the copy where it exists (default), 0 = read the float32
 *                   rows.
 *   "split_rows"    a float32 row that ends 1..32 bytes past a 128-byte line (4d mod 128 in 1..32, e.g. d = 100: 400
 *                   bytes) costs one more 128-byte request per evaluation for those last bytes.  For such shapes
 *                   (when there are no byte rows) the index keeps the whole lines of every row in a table of its own
 *                   and the 16 / 32 remaining bytes of node nbr0[c][j] beside slot (c, j) of the layer-0 adjacency,
 *                   where one hop finds all its candidates' tails in a few contiguous lines; the knn searches read
 *                   those on layer 0 (same lanes, operands and order of arithmetic: bit-identical results).
 *                   1 = use the copy where it exists (default), 0 = read the plain rows, -1 = read the plain rows and FREE
 *                   the copy (it cannot come back).  The copy is not small: n * (128-byte lines of a row) + n * max_degree0 *
 *                   (16 or 32) bytes -- for a GloVe-shaped index (1.18 M x 100, M 32) 0.45 + 1.2 GB beside 0.47 GB of
 *                   vectors; hnsw_index_info.device_bytes counts it.
 *   "visited_blocks" how the knn kernels with W in four or more registers (ef > 128) remember visited nodes
 *                   (Visited, lib/ohnsw.ml:256-268): 0 = an LDS cache of node tags (all that rounds 1-4 had); 1 = an LDS
 *                   cache of BITMAP BLOCKS over "locality codes" -- a second numbering of the nodes, derived from the
 *                   index's own upper layers, under which graph-close nodes are consecutive, so that the nodes a walk
 *                   visits share blocks and cost one bit each (ocaml-hnsw_amd/csrc/hnsw_locality.hip); -1 (default) = the
 *                   handle decides per kernel shape by searching 256 probe queries (midpoints between a stored vector and
 *                   its first neighbour) both ways and counting evaluations, inside the first search call that needs the answer --
 *                   or ahead of it: hnsw_index_prepare, expected_ef -- (which then also builds the codes: one
 *                   small layer search per node, n * (1 + max_degree0) * 4 bytes of tables, a device synchronisation --
 *                   1.2 s for 10 M nodes; indices below 200 000 nodes are not measured).  MEMORY: the n * max_degree0 * 4 bytes of
 *                   per-slot codes (2.56 GB for 10 M nodes at M 32; counted in hnsw_index_info.device_bytes while they exist) are kept
 *                   only while some kernel shape of the handle uses the blocks: a measurement that chooses the tag cache frees
 *                   them again, the n * 4 bytes of per-node codes stay (a later measurement re-makes the table in milliseconds).
 *                   Clustered / embedding-like data:
 *                   the blocks end the repeated evaluations of forgotten nodes (DEEP10M shape, ef 512: 40 % -> 5 % of all
 *                   evaluations); structureless data: the tags win and are kept.  Results are the same bits either way.
 * and one that buys exactness for the device-pointer entry point:
 *   "device_fallback_slab_bytes"  the library allocates a slab of this many bytes (0 frees it); hnsw_search_batch_device
 *                   then lists the queries its launch flagged (d_status bit 0: tie list outgrew its LDS slots) ON THE
 *                   DEVICE and searches them again with the slab on the caller's stream -- no host round trip, two small
 *                   extra launches per call.  One flagged query needs 4 n bytes (a slot per node), so a slab repairs
 *                   bytes / (4 n) queries per call; those it could not take keep their flag.  Needs d_status.  The list and
 *                   the slab belong to the handle: with this option ONE hnsw_search_batch_device / hnsw_search_batch_h2d call
 *                   in flight per handle (calls on one stream are ordered and therefore fine; calls on different streams
 *                   must not overlap).
 * and one that CHANGES results (off by default):
 *   "half_rows"     the knn searches read a copy of the vectors rounded to fp16 (round to nearest even; subnormals and
 *                   -0 kept: numpy's astype(float16)), 8 bytes per 4 dimensions in rows of 128-byte lines -- half the
 *                   bytes gathered per evaluation of float32 rows.  Each half is converted back to float exactly and the
 *                   arithmetic is that of the float32 rows, so the results are BIT FOR BIT those of the same search over
 *                   Xh = X.astype(float16).astype(float32): exact over Xh, approximate over X.  The query stays float32.
 *                   1 = make the copy if it does not exist and read it (it takes the place of the split rows and of the
 *                   float32 rows), 0 = read the float32 / split rows again (the copy is kept), -1 = ... and FREE the copy
 *                   (after a device synchronisation).  The copy costs n * 128 * NCH bytes, NCH = ceil(d / 64) rounded up
 *                   to 1, 2, 4, 8 or 16 (the kernel's lane grid, zero padded), counted in hnsw_index_info.device_bytes.  Refused, the index unchanged: HNSW_ERR_BAD_ARG while byte rows are in
 *                   use (they are exact and half the size: set "byte_rows" 0 first; "byte_rows" 1 later puts them
 *                   first again), HNSW_ERR_UNSUPPORTED when a value is NaN or rounds to an fp16 infinity (|x| >= 65520).
 *                   The builder, hnsw_index_insert's searches, the layer operators and hnsw_distance_batch keep reading
 *                   the float32 rows.  hnsw_index_insert makes the copy again for the grown index (new vectors out of
 *                   range: the whole insert is refused).  Not saved: a loaded index starts without half rows.
 *                   (Hand-scheduled loops exist for the other row formats only: half rows run the C++ hop loop.)
 *                   HNSW_ERR_BAD_ARG while option "sq8_rows" is on.
 *   "sq8_rows"      the knn searches WALK a copy of the vectors quantised to 8 bits under one affine map for the whole table and
 *                   answer from the float32 rows: the byte-row kernels (a quarter of the bytes of float32 rows per evaluation,
 *                   the hand-scheduled loops for 65..256 dimensions) for float data that is not byte-valued.
 *                   1 = make the copy if it is missing and search it, 0 = read the previous rows again (the copy is kept),
 *                   -1 = ... and FREE the copy (after a device synchronisation).
 *                   QUANTISER (float32, round to nearest even, no contraction: numpy reproduces the bits): lo = min, hi = max
 *                   over the n * d stored values; s = (hi - lo) / 255, s = 1 when hi == lo (a bound of -0 counts as +0);
 *                   code(x) = min(255, max(0, rint((x - lo) / s))), ties to even.  Rows lie in the byte kernels' lane grid:
 *                   64 * NCH bytes per row, zero padded.  A NaN or infinity in X, hi - lo overflowing, or a range so narrow
 *                   (subnormal) that (hi - lo) / 255 rounds to 0, is HNSW_ERR_UNSUPPORTED and leaves the index unchanged.
 *                   QUERY: L2: q' = (q - lo) / s, the same operations on the d real values (zero beyond d, matching the rows'
 *                   padding); inner product: q' = q.  q' is NOT checked: a finite query value so large that (q - lo) / s
 *                   overflows float32 walks with infinite or NaN distances in code space (the re-rank still returns exact
 *                   distances for whatever the walk found); a NaN in a query behaves as it does on every other row format.
 *                   With ONE map x^ = lo + s * code(x), |x^ - q|^2 = s^2 |code(x) - q'|^2 and
 *                   <x^, q> = lo * sum(q) + s * <code(x), q>: the search over X^ orders exactly as the search over the codes.
 *                   A SEARCH of (ef, k) while sq8 rows are read
 *                     1. walks the codes B with q': the unchanged byte-row kernels, descent included -- bit for bit the search
 *                        over B.astype(float32) with q' (the integer path runs when q' is byte-valued),
 *                     2. takes the first c = min(ef, max(k, R)) members of W, R = option "refine" (0 gives c = k, -1 gives c = ef),
 *                     3. re-ranks those c over the FLOAT32 rows with hnsw_rerank_batch's kernel and
 *                     4. returns the first k under (distance, node id).
 *                   The walk's distances live in code space and mean nothing to a caller, so the re-rank is unconditional: the
 *                   returned distances are always the bits of hnsw_distance_batch over X.  out_nhops is the walk's count,
 *                   out_ndist the walk's count plus c.  HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG, as with refine active.
 *                   Applies to every knn form: hnsw_search_batch, _device, _h2d, hnsw_search_submit / _wait, hnsw_knn, and
 *                   hnsw_multi_search_batch* through a replica's handle (hnsw_multi_replica).  Does NOT apply to the builder,
 *                   hnsw_index_insert's searches, the layer operators, hnsw_distance_batch, hnsw_brute_force_batch and
 *                   hnsw_rerank_batch, which keep reading the float32 rows.
 *                   EXCLUSIONS: HNSW_ERR_BAD_ARG while byte rows are in use (they are exact and the same size: "byte_rows" 0
 *                   first) and while "half_rows" is on; the split rows step aside as they do for half rows.
 *                   hnsw_index_info.row_format reports HNSW_ROWS_SQ8, hnsw_index_row_bytes gives d, and the copy's
 *                   n * 64 * NCH bytes count in device_bytes.  Not saved: a loaded index starts without it.  hnsw_index_insert
 *                   quantises the WHOLE grown table again (the range may widen); a new vector that is not finite refuses the
 *                   whole insert and leaves the index, the copy and its parameters as before.
 *                   SCRATCH: q' ([nq][d padded to 16] floats) lives beside the refine scratch -- owned by the handle, by the
 *                   request for submit / wait, sized on demand, not counted in device_bytes --: the same ONE
 *                   hnsw_search_batch_device / hnsw_search_batch_h2d call in flight per handle as with refine active.
 *                   hnsw_index_sq8_params / hnsw_index_sq8_codes give lo, s and the codes.  A scale per dimension is option
 *                   "sq8_dim_rows" below (a weighted L2 walk in a kernel family of its own).  HNSW_ERR_BAD_ARG while that
 *                   option is on.  Rate and recall: not measured yet (tools/sq8_rate.py prints the table for profiles/sq8_rows.txt).
 *   "sq8_dim_rows"  as "sq8_rows", with one affine map PER DIMENSION: where the columns of X do not share a range (a few outliers in
 *                   one column are enough) one map for the whole table spends its 256 codes on the widest column and is blind in
 *                   the others.  1 = make the copy if it is missing and search it, 0 = read the previous rows again (the copy is
 *                   kept), -1 = ... and FREE the copy (after a device synchronisation); any other value is HNSW_ERR_BAD_ARG.
 *                   QUANTISER (float32, round to nearest even, no contraction: numpy reproduces the bits): for each dimension i,
 *                   lo_i = min, hi_i = max over the n stored values of column i (a bound of -0 counts as +0);
 *                   s_i = (hi_i - lo_i) / 255, s_i = 1 when hi_i == lo_i; code = min(255, max(0, rint((x - lo_i) / s_i))), ties to
 *                   even.  Rows lie in the byte kernels' lane grid: 64 * NCH bytes per row, zero padded.  A NaN or infinity in X,
 *                   a column whose hi - lo overflows, or one so narrow that (hi - lo) / 255 rounds to 0, is HNSW_ERR_UNSUPPORTED
 *                   (the message names the first such column) and leaves the index unchanged.
 *                   WALK, with x^_i = lo_i + s_i * code_i.  Inner product (and HNSW_METRIC_COSINE through its inner-product twin):
 *                   <x^, q> = sum(lo_i q_i) + <code, s o q>, the first term constant per query, so the walk is the UNCHANGED
 *                   byte-row search over the codes C with q'_i = fl(s_i * q_i): bit for bit the inner-product search over
 *                   C.astype(float32) with q'.  L2: |x^ - q|^2 = sum((s_i code_i - (q_i - lo_i))^2) is a weighted distance: a row
 *                   format of the knn kernel of its own (the loads of the byte rows; per dimension z = fl((float)code * s_i),
 *                   dx = fl(z - q''_i), acc = fma(dx, dx, acc) with q''_i = fl(q_i - lo_i), 0 beyond d; lanes, chunk order and
 *                   16-lane tree of every distance of the library; the C++ hop loop: no hand-scheduled loop).  TWIN: ids, walk
 *                   distances, hops and W of this walk are bit for bit those of a float32-row L2 index with the same graph over
 *                   Z = C.astype(float32) * s (numpy float32), searched with Q'' = Q - lo.  q' and q'' are NOT checked for
 *                   overflow, as with "sq8_rows".
 *                   Everything after the walk is "sq8_rows" unchanged: c = min(ef, max(k, R)) members of W (R = option "refine")
 *                   re-ranked over the FLOAT32 rows, unconditionally; the first k under (distance, node id) come back with the
 *                   bits of hnsw_distance_batch; out_nhops is the walk's count, out_ndist the walk's count plus c;
 *                   HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG; the same scratch and the same ONE call in flight per handle;
 *                   every knn form, the filtered and range ladders (all of W re-ranked), marked indexes, multi replicas
 *                   (hnsw_multi_replica) and sharded indexes (hnsw_sharded_set_option: one set of maps per shard).  The builder,
 *                   hnsw_index_insert's searches, the layer operators, hnsw_distance_batch, the exact scans and hnsw_rerank_batch
 *                   keep reading the float32 rows.  Option "visited_blocks" treats these rows as it treats sq8 rows.
 *                   EXCLUSIONS: HNSW_ERR_BAD_ARG, the index unchanged, when it is set to 1 while byte rows are in use
 *                   ("byte_rows" 0 first) or while option half_rows, sq8_rows or filter_collect is on, and when one of those
 *                   three is set to 1 while this option is on; the split rows step aside.
 *                   hnsw_index_info.row_format reports HNSW_ROWS_SQ8_DIM, hnsw_index_row_bytes gives d, and the copy's
 *                   n * 64 * NCH bytes plus its two per-dimension tables (lo and s in the lane grid: 2 * 4 * 64 * NCH bytes) count
 *                   in device_bytes.  Not saved: a loaded index starts without it.  hnsw_index_insert and hnsw_index_remove
 *                   quantise the WHOLE remaining table again; a new vector that is not finite refuses the whole insert and leaves
 *                   the index, the copy and its parameters as before.  hnsw_index_sq8_dim_params / hnsw_index_sq8_dim_codes
 *                   give lo[d], s[d] and the codes.  Not built: hand-scheduled loops for this format, a saved copy.
 *                   RATE AND RECALL (one MI355X, 1 M x 128, L2, ef 128, k 10, 10 k queries; tools/sq8_dim_rate.py,
 *                   profiles/sq8_dim_rows.txt): the walk costs 1.01 to 1.03 times the launches of the "sq8_rows" walk on the same
 *                   handle (the same bytes gathered; one more multiply per dimension, the C++ hop loop).  SIFT-like data: 16.6 M
 *                   queries/s device-resident against 16.8 over sq8 rows and 13.4 over float32 rows, recall@10 0.989 for both kinds
 *                   of codes at refine 0 and 1.000 at refine 64.  Standard normal data with 8 rows multiplied by 400 in dimension
 *                   0: recall@10 0.285 against 0.093 over sq8 rows (0.167 at refine 64) and 0.293 over the float32 rows, at 2.3
 *                   times the float32 rows' rate.
 *   "filter_collect" 0 = off (default: every result, counter and code path is exactly as without the option); 1 = the filtered
 *                   searches answer from EVERY node the layer-0 walk evaluates, not from the final W only: a walk at ef 128
 *                   evaluates about 950 to 2400 nodes and keeps 128, and each evaluated node has an exact distance.  The
 *                   definition is the paragraph WITH OPTION filter_collect of the filtered search below.  Any other value is
 *                   HNSW_ERR_BAD_ARG.  It changes answers only for queries the ladder would otherwise walk again (and, at stage 0,
 *                   a tie at the k-th place): there it trades recall for not re-walking, which is why it is opt-in.
 *                   k <= 128 only: for k > 128 the option has no effect and the ladder over W answers.
 *                   EXCLUSIONS: exact-row formats only (float32, byte and split rows).  HNSW_ERR_BAD_ARG, the index unchanged,
 *                   when it is set to 1 while option "half_rows" or "sq8_rows" is on, and when "half_rows" or "sq8_rows" is
 *                   set to 1 while it is 1 (option "sq8_dim_rows": likewise, both ways).  Not saved: a loaded index starts with it off.  hnsw_index_insert and
 *                   hnsw_index_remove keep the setting.  Range search is not affected.  RATE AND RECALL (one MI355X, 1 M x 128 byte
 *                   rows, ef 128, k 10, 10 k queries; tools/filter_rate.py --collect, profiles/filter_collect.txt), on against off:
 *                   selectivity 0.01: 8.2 ms per batch against 45.9, recall@10 0.787 against 0.998; 0.1: 8.2 against 8.9, recall
 *                   0.920 against 0.935; 1 and 0.5: 2-8 % slower with the same rows (the collect kernel runs the C++ hop loop);
 *                   0.001: 5 % slower (the exact scan answers either way); a marked index: 2-8 % slower, the same rows.
 * and one that gives the half-row searches float32 answers again (off by default):
 *   "refine"        0 = off (default: behaviour is exactly as without the option); R in 1..1024 = a candidate count; -1 = all
 *                   of W; anything else is HNSW_ERR_BAD_ARG.  While the knn searches read the half rows, a search of (ef, k)
 *                     1. runs the half-row search unchanged,
 *                     2. takes the first c = min(ef, max(k, R)) members of W (c = ef for -1) -- W holds ef candidates where the
 *                        caller asked for k --,
 *                     3. re-ranks those c over the FLOAT32 rows (hnsw_rerank_batch's kernel: the summation order every
 *                        distance-returning entry point shares) and
 *                     4. returns the first k under (distance, node id).
 *                   So: the candidate set is the half-row search's (the search over Xh with k := c), the returned distances
 *                   are the bits of hnsw_distance_batch for their own vectors, equal distances come lowest id first, and no
 *                   query's id-set recall over X is below that of its unrefined half-row answer (with -1 it is
 *                   |truth and W| / k).  out_nhops is unchanged; out_ndist is the walk's count PLUS the number of
 *                   candidates re-evaluated.  The re-rank runs behind the tie-overflow repair (host forms) or the device
 *                   fallback slab.  It applies to hnsw_search_batch, _device, _h2d, hnsw_search_submit / _wait, hnsw_knn and,
 *                   through a replica's handle (hnsw_multi_replica: where "half_rows" is set too), to hnsw_multi_search_batch.
 *                   The walk's [nq][c] results live in scratch the handle owns (per request for submit / wait), sized on
 *                   demand and not counted in device_bytes: with refine active ONE hnsw_search_batch_device /
 *                   hnsw_search_batch_h2d call in flight per handle (calls on one stream are ordered and therefore fine).
 *                   While the searches read any other rows (bytes, split, float32) the option is accepted and does nothing
 *                   -- except over sq8 rows (options "sq8_rows", "sq8_dim_rows"), whose searches are always re-ranked and take c from it --:
 *                   those distances are exact over X already, results and out_ndist are bit-identical to refine 0; set
 *                   before "half_rows" it takes effect when half rows are turned on.  HNSW_SEM_FUNCTOR_NEAREST_K with refine
 *                   active is HNSW_ERR_BAD_ARG ("the k farthest of W" has no refined meaning).  hnsw_index_insert keeps the
 *                   setting; it is not saved (neither is "half_rows").  COST: c float32 rows per query on top of the walk's
 *                   roughly 950 to 2400 half-row evaluations (the benchmark's float shapes); the rate has not been measured
 *                   yet (tools/refine_rate.py prints the table that belongs beside profiles/half_rows.txt).
 * and one more row format that CHANGES results, for wide rows (off by default):
 *   "bit_rows"      binary quantisation: the knn searches walk ONE BIT per dimension under Hamming distance and answer from the
 *                   float32 rows.  A 1024-dimensional row is one 128-byte line (float32: 32 lines, sq8: 8), a 512-dimensional one
 *                   half a line.  0 = off (default; the copy is FREED, after a device synchronisation, and the previous rows are
 *                   read again); 1 = on, the thresholds t at the column means; 2 = on, the thresholds at zero (sign bits: the
 *                   usual choice for cosine / inner-product embeddings); any other value is HNSW_ERR_BAD_ARG.  Setting 1 or 2
 *                   makes the copy (again, when the mode changes).
 *                   THRESHOLDS t[d].  Mode 2: t_i = +0.  Mode 1: t_i = the float32 rounding of the mean of column i of the rows
 *                   the handle holds (hnsw_index_get_rows; for a HNSW_METRIC_COSINE index these are N(X)), the mean accumulated in
 *                   float64 by a two-stage reduction whose grid is fixed by (n, d) alone: the same table gives the same bits on
 *                   every call.  The sums and the finite check come from one pass over the rows; a NaN or infinity, under either
 *                   mode, is HNSW_ERR_UNSUPPORTED (the message names the first such column) and leaves the index unchanged.
 *                   CODES.  Bit i of a row is x_i > t_i: equality gives 0, and -0 counts as +0.  Bits are packed little-endian into
 *                   uint32 words: dimension i is bit i % 32 of word i / 32.  With NW = ceil(d / 512) (1 or 2) a stored row is
 *                   16 * NW words (64 * NW bytes), zero beyond d; lane l16 of a 16-lane group reads word 16 * j + l16 in step j, so
 *                   for d > 512 a group's step pair is one whole 128-byte line.
 *                   QUERIES get the same rule against the same t, on the device, once per call (for a HNSW_METRIC_COSINE index
 *                   after the index's own normalisation); a page-locked host matrix is read in place, each value once.
 *                   WALK.  H = sum over the words of popcount(row_word ^ query_word), an integer; the walk's key is that of the
 *                   squared L2 distance 4 * H -- (float)(4 * H) -- on every layer, WHATEVER the index's metric: Hamming order is the
 *                   order of L2, of -IP and of cosine between +-1 vectors.  TWIN: ids, members of W, hops and evaluations of this
 *                   walk are bit for bit those of a float32-row L2 index with the same graph over S = where(X > t, 1, -1)
 *                   (float32), searched with where(Q > t, 1, -1): every term of that float sum is 0 or 4 and every partial sum an
 *                   integer <= 4096, so the float32 arithmetic never rounds and the order of summation does not show.
 *                   Everything after the walk is "sq8_rows" unchanged: c = min(ef, max(k, R)) members of W (R = option "refine")
 *                   re-ranked over the FLOAT32 rows under the index's real metric, unconditionally; the first k under (distance,
 *                   node id) come back with the bits of hnsw_distance_batch; out_nhops is the walk's count, out_ndist the walk's
 *                   count plus c; HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG; the same scratch and the same ONE call in flight
 *                   per handle; every knn form, the filtered, range and grouped ladders (all of W re-ranked), marked indexes,
 *                   multi replicas (hnsw_multi_replica) and sharded indexes (hnsw_sharded_set_option: thresholds per shard).  With
 *                   R = 0 ONLY THE FIRST k BY HAMMING DISTANCE are re-scored -- one bit per dimension orders neighbours coarsely --:
 *                   "refine" -1 (all ef) is the setting this format is meant for; the default of "refine" is not changed.
 *                   The builder, hnsw_index_insert's searches, the layer operators, hnsw_distance_batch, the exact scans and
 *                   hnsw_rerank_batch keep reading the float32 rows.  Option "visited_blocks" treats these rows as sq8 rows.
 *                   EXCLUSIONS: HNSW_ERR_BAD_ARG, the index unchanged, when it is set to 1 or 2 while byte rows are in use
 *                   ("byte_rows" 0 first) or while option half_rows, sq8_rows, sq8_dim_rows or filter_collect is on, and when one
 *                   of those four is set to 1 while this option is on; the split rows step aside.
 *                   hnsw_index_info.row_format reports HNSW_ROWS_BITS, hnsw_index_row_bytes gives (d + 7) / 8, and the copy's
 *                   n * 64 * NW bytes plus its threshold table (4 * 512 * NW bytes) count in device_bytes; at 0 device_bytes is
 *                   what it was.  Not saved: a loaded index starts without the copy.  hnsw_index_insert and hnsw_index_remove
 *                   quantise the WHOLE remaining table again (mode 1: the means move); a new vector that is not finite refuses the
 *                   whole insert.  hnsw_index_bit_params / hnsw_index_bit_codes give t and the codes.
 *                   Not built: hand-scheduled hop loops for this format, an asymmetric distance (float query against bits), more
 *                   than one bit per dimension, a saved copy, "filter_collect" with bit rows, a changed default for "refine".
 *                   RATE AND RECALL (one MI355X; 200 000 clustered unit vectors, inner product, M 16, k 10, 10 k queries; medians of
 *                   15 device-resident calls, the formats alternated on one handle; tools/bit_rows_rate.py, profiles/bit_rows.txt).
 *                   d = 1024, ef 128: the walk's launches take 1.31 ms per batch over the bits against 2.18 ms over the
 *                   "sq8_dim_rows" codes and 6.82 ms over the float32 rows -- and find little: recall@10 0.18 at refine 0, 0.72 at
 *                   refine -1 (1.95 ms), where the sq8_dim codes reach 0.998 at refine 40 in 2.36 ms.  The bits need a wide W:
 *                   refine -1 gives 0.89 at ef 256 (3.43 ms) and 0.986 at ef 512 (7.67 ms; float32 rows: 1.000 in 11.5 ms, sq8_dim
 *                   1.000 in 6.74 ms).  d = 512: the walk over the bits (1.28 to 1.35 ms at ef 128) is no faster than the one over
 *                   the sq8_dim codes (1.23 ms): both are bound by a hop's latency, not by bytes.  On this data the sq8_dim codes
 *                   are the better trade at every setting measured; the two threshold modes do not differ.
 *   "bit_query_bits" supersedes the "asymmetric distance" item of the Not built list above: 0 = off (default: every result, counter
 *                   and code path of "bit_rows" is exactly as without the option); 4 = while the searches walk the bit rows, the QUERY
 *                   keeps 4 bits per dimension; any other value is HNSW_ERR_BAD_ARG.  The rows are the same copy, the same bytes and
 *                   the same device_bytes, and row_format stays HNSW_ROWS_BITS.  It may be set before or after "bit_rows" and takes
 *                   effect while the bit rows are walked, as "refine" does for half rows; while other rows are walked it is accepted
 *                   and does nothing.
 *                   QUERY CODES, made on the device once per call, where the query's bits are made when the option is off (for a
 *                   HNSW_METRIC_COSINE index after the index's own normalisation; a page-locked host matrix is read in place, each
 *                   value once).  With the index's thresholds t (hnsw_index_bit_params): y_i = fl(q_i - t_i) in float32 for i < d;
 *                   a = max |y_i|; r = fl(7.0f / a), an IEEE-rounded division, not a reciprocal estimate; v_i = (int)rint(fl(y_i *
 *                   r)), ONE rounded product, round-half-even, in -7..7 by construction.  DEGENERATE QUERIES: if a = 0, or any y_i is
 *                   NaN or infinite, or r is infinite (a subnormal a), every code of that query is 0; every node then ties and the
 *                   walk orders by node id.  PLANES: a code is stored as the four bit planes of its two's-complement nibble, v = p0 +
 *                   2 * p1 + 4 * p2 - 8 * p3; each plane is packed exactly as a row's bits are (dimension i in bit i % 32 of word
 *                   i / 32, 16 * NW words a plane, zero beyond d), so a query row is 64 * NW words.  hnsw_index_bit_query_codes
 *                   returns the v_i.
 *                   WALK.  The loads are those of "bit_rows".  Per row word, c_p = popcount(row_word & plane_p word) and the term is
 *                   c0 + 2 * c1 + 4 * c2 - 8 * c3; their sum over the row's words is A = the sum of v_i over the row's set bits, an
 *                   integer.  With SV = the sum of all v_i (made once per walk), acc = 2 * A - SV is <v, s> for the +-1 vector s the
 *                   row's bits stand for, and the key is the inner product's -- that of the distance 1 - (float)acc -- on every
 *                   layer, WHATEVER the index's metric: for a fixed query, -<y, s> orders the rows as |y - c * s| does, so the
 *                   argument of "bit_rows" carries over.  TWIN: ids, members of W, hops and evaluations of this walk are bit for bit
 *                   those of a float32-row HNSW_METRIC_IP index with the same graph over S = where(X > t, 1, -1) (float32),
 *                   searched with V (the codes as float32): every term of that float sum is an integer of magnitude <= 7 and every
 *                   partial sum an integer of magnitude <= 7168, so the float32 arithmetic never rounds and the order of summation
 *                   does not show.  Shapes, batches in flight, the visited set and everything after the walk (the re-rank over the
 *                   float32 rows under the real metric, "refine", out_ndist = the walk's count plus c, ladders, marks, shards,
 *                   hnsw_search_submit / _wait, HNSW_SEM_FUNCTOR_NEAREST_K refused) are those of "bit_rows".
 *                   Not saved.  hnsw_index_insert and hnsw_index_remove keep it; hnsw_sharded_set_option forwards it; a replica of a
 *                   multi index takes it through hnsw_multi_replica.
 *                   RATE AND RECALL (one MI355X; the data, the method and the handle of the figures above; tools/bit_rows_rate.py --query-bits,
 *                   profiles/bit_query_bits.txt; option on against off, same handle, same session, refine -1).  d = 1024: the search
 *                   launches take 1.90 ms per 10 k batch against 1.95 ms at ef 128, 3.50 against 3.39 at ef 256, 7.62 against 7.69 at ef
 *                   512 -- the 4-bit query costs nothing measurable -- and recall@10 goes from 0.72 to 0.88, from 0.89 to 0.97, from
 *                   0.986 to 0.9986; d = 512: 1.50 against 1.68 ms, 2.68 against 2.62, 5.92 against 6.00, recall 0.72 to 0.89, 0.89 to
 *                   0.97, 0.988 to 0.9992.  With refine 40: 0.42 to 0.62.  The query transform takes 19 to 39 us per 10 k queries
 *                   (the 1-bit one: 15 to 28 us), the pre-pass 0.085 ms against 0.068.  The extra registers (5 to 7 VGPRs for d <=
 *                   512, 12 above) cross an occupancy step for 16 of the 40 kernel instances; no rate above follows the steps.  It
 *                   still does not beat the "sq8_dim_rows" codes at equal recall (0.998 at ef 128 with 40 re-ranked in 2.32 ms at d =
 *                   1024, 1.32 ms at d = 512); only the cheapest points at d = 1024 (0.62 in 1.42 ms, 0.88 in 1.90 ms) lie below the
 *                   fastest sq8_dim setting measured. */
int32_t hnsw_index_set_option(hnsw_index *idx, const char *name, int64_t value);
/* Bytes of one vector as the knn searches read it: d for byte and sq8 rows (either kind), 2 * d for half rows, 4 * d for float32 rows,
 * (d + 7) / 8 for bit rows. */
int32_t hnsw_index_row_bytes(const hnsw_index *idx, int64_t *row_bytes);
/* The sq8 copy (option "sq8_rows"), for callers who want X^ = lo + scale * codes: its two parameters, and its codes as
 * [n][d] bytes (the rows' padding is not exported).  HNSW_ERR_BAD_ARG when no copy exists (never made, or freed by -1). */
int32_t hnsw_index_sq8_params(const hnsw_index *idx, float *lo, float *scale);
int32_t hnsw_index_sq8_codes(const hnsw_index *idx, uint8_t *out);
/* The per-dimension sq8 copy (option "sq8_dim_rows"), x^_i = lo[i] + scale[i] * code: its parameters (lo and scale: [d] floats
 * each), and its codes as [n][d] bytes (the rows' padding is not exported).  HNSW_ERR_BAD_ARG for a null argument and when no copy
 * exists (never made, or freed by -1). */
int32_t hnsw_index_sq8_dim_params(const hnsw_index *idx, float *lo, float *scale);
int32_t hnsw_index_sq8_dim_codes(const hnsw_index *idx, uint8_t *out);
/* The 1-bit copy (option "bit_rows"): its thresholds t ([d] floats; mode 2: all +0), and its codes as [n][ceil(d / 32)] uint32
 * words, dimension i in bit i % 32 of word i / 32 (the rows' padding words are not exported).  HNSW_ERR_BAD_ARG for a null argument
 * and while the option is off. */
int32_t hnsw_index_bit_params(const hnsw_index *idx, float *t /* [d] */);
int32_t hnsw_index_bit_codes(const hnsw_index *idx, uint32_t *out /* [n][ceil(d/32)], padding words not exported */);
/* The 4-bit query codes of option "bit_query_bits" (the rule stands there): the v_i in -7..7 the walk would use for these queries
 * ([nq][q_stride] floats on the host; a HNSW_METRIC_COSINE index normalises them first), as [nq][d] int8.  It does not require
 * "bit_query_bits" to be on.  HNSW_ERR_BAD_ARG for a null argument, nq < 0, q_stride < d, and while option "bit_rows" is off. */
int32_t hnsw_index_bit_query_codes(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int8_t *out /* [nq][d] */);
/* Mean durations (ms) over the device-entry calls recorded since the last call of this function
 * (option "time_kernels"): the search kernel itself, and the ordering pre-pass (descent kernel +
 * sort; 0 when the batch was searched in the given order).  Waits for the recorded calls. */
int32_t hnsw_index_kernel_times(hnsw_index *idx, double *search_ms, double *prepass_ms, int32_t *calls);

/* Batched search, host buffers.  queries: [nq][q_stride] fp32 (a Lacaml.S.mat d x nq).
 * out_ids [nq][k] int32 (id_base-based), out_dist [nq][k] fp32, ascending.
 * out_ndist / out_nhops (optional, [nq]): distance evaluations and expanded candidates on
 * layer 0 per query -- the unit the reference counts in lib/hnsw.ml:730-751. */
int32_t hnsw_search_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                          const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                          uint32_t *out_ndist, uint32_t *out_nhops);

/* Optional: page-locked query / result matrices.  The host-buffer entry points (hnsw_search_batch, hnsw_search_batch_h2d,
 * hnsw_search_submit / hnsw_search_wait, hnsw_multi_search_batch) then do not copy such a matrix at all where they can: the
 * device reads the queries straight out of it (each query once, by the wave that searches it: the transfer runs under the
 * ordering pre-pass) and writes every query's results straight into the caller's result matrices as the query finishes.
 * Everything is complete when the call returns.  Two ways to get such memory:
 *   hnsw_host_alloc / hnsw_host_free        the library allocates page-locked memory (hipHostMalloc); the OCaml side wraps it
 *                                           as a Bigarray (Ctypes.bigarray_of_ptr; Hnsw_mi355x.alloc_mat).
 *   hnsw_host_register / hnsw_host_unregister  page-lock an array the caller already has (hipHostRegister).  The CALLER owns
 *                                           the lifetime: the array stays allocated (a Bigarray: reachable) until
 *                                           hnsw_host_unregister; the library never registers anything behind the caller's
 *                                           back.  Registering an array twice is not an error; an array of which only a
 *                                           part is registered already is refused (HNSW_ERR_BAD_ARG); an array somebody else
 *                                           has page-locked is accepted, left to its owner and never accessed in place.
 * Only ranges obtained through these four calls are accessed directly; any other pointer is staged through copies.
 * LIFETIME.  A range may be unregistered / freed at any time after the call that used it has RETURNED: hnsw_host_unregister and
 * hnsw_host_free wait for the asynchronous work that still reads it (hnsw_search_batch_h2d's kernels read a registered query
 * matrix in place after the call has returned; hnsw_search_submit's upload is a DMA out of it) -- the library keeps an event
 * behind the last such reader per range and stream.  What the library cannot defend against is the memory itself going away
 * while registered (munmap / free of an array that was never unregistered): unregister first.  Both calls answer
 * HNSW_ERR_BAD_ARG for a pointer that is not the start of a range THEY handed out (hnsw_host_unregister: registered through
 * hnsw_host_register; hnsw_host_free: allocated by hnsw_host_alloc). */
int32_t hnsw_host_register(void *p, int64_t bytes);
int32_t hnsw_host_unregister(void *p);
int32_t hnsw_host_alloc(void **out, int64_t bytes);
int32_t hnsw_host_free(void *p);

/* Same, device buffers, asynchronous on `stream` (a hipStream_t; NULL = default stream).
 * d_status (optional, [nq] uint32): bit 0 set if the query's list of tied, still expandable
 * candidates outgrew its 64 LDS slots.  WITHOUT THE OPTION "device_fallback_slab_bytes" THIS ENTRY POINT HAS NO EXACTNESS
 * FALLBACK: entries that did not fit were not expanded, so a flagged query's result may MISS neighbours the reference would return
 * (tests/test_gpu_parity.py::test_tie_overflow_beyond_lds_stack builds such a case), not merely order
 * ties differently.  A caller that needs the reference's result passes d_status and re-runs the flagged
 * queries through hnsw_search_batch (host buffers; it searches them again with a global slab), as
 * bench.py counts them (checks.tie_overflow_flagged).  Needs exact ties on a massive scale (e.g. > 64
 * nodes at exactly max(W).d): 0 of the 10 000 queries of the SIFT-shaped benchmark sets. */
int32_t hnsw_search_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq,
                                 int64_t q_stride, const hnsw_search_params *params,
                                 int32_t *d_ids, float *d_dist, uint32_t *d_ndist,
                                 uint32_t *d_nhops, uint32_t *d_status, void *stream);

/* The batch call with its two ends apart: the queries come from HOST memory ([nq][q_stride], as hnsw_search_batch takes
 * them: read by the device directly when the caller registered the matrix with hnsw_host_register, staged through the
 * handle's scratch otherwise), the results are left in DEVICE buffers, everything asynchronous on `stream` -- for a caller
 * that exchanges per-shard results between devices (one process per GPU and an RCCL all-gather: bench.py --gpus N,
 * ocaml-hnsw_amd/sharding.py) before anything goes back to the host.  The query matrix must stay ALLOCATED until the stream has
 * passed the call (unregistering it earlier is safe: hnsw_host_unregister waits, see LIFETIME above); one such call in flight
 * per handle (it uses the handle's query scratch).  As hnsw_search_batch_device:
 * flags only (d_status), unless the option "device_fallback_slab_bytes" is set. */
int32_t hnsw_search_batch_h2d(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                              const hnsw_search_params *params, int32_t *d_ids, float *d_dist,
                              uint32_t *d_ndist, uint32_t *d_nhops, uint32_t *d_status, void *stream);

/* The same batch call in two halves, for callers that keep batches coming: a single batch ends with
 * a drain phase (its last queries run on a nearly empty chip at their serial latency, DESIGN.md
 * section 4), which the next batch can fill.  hnsw_search_submit copies the queries in and starts the
 * search on one of the handle's streams, then returns; hnsw_search_wait blocks until that request is
 * done, copies its results out (same arrays and meaning as hnsw_search_batch) and releases it.
 * Requests may be waited for in any order; every submitted request must be waited for (or the index
 * destroyed).  Still one host thread at a time per handle.
 *     submit(b1); submit(b2); wait(b1); submit(b3); wait(b2); ...                                  */
typedef struct hnsw_request hnsw_request;
int32_t hnsw_search_submit(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                           const hnsw_search_params *params, hnsw_request **out);
int32_t hnsw_search_wait(hnsw_request *req, int32_t *out_ids, float *out_dist,
                         uint32_t *out_ndist, uint32_t *out_nhops);

/* Single query (Ohnsw.knn / Hnsw.Ba.knn).  *out_count = number of results (<= k). */
int32_t hnsw_knn(hnsw_index *idx, const float *query, const hnsw_search_params *params,
                 int32_t *out_ids, float *out_dist, int32_t *out_count);

/* Gathered distances: out[q][j] = distance(query q, vector ids[q][j]); ids id_base-based.
 * Counterpart of bench_dist/bench_dist.ml (one distance call per pair). */
int32_t hnsw_distance_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                            const int32_t *ids, int32_t m, float *out);
int32_t hnsw_distance_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq,
                                   int64_t q_stride, const int32_t *d_ids, int32_t m,
                                   float *d_out, void *stream);

/* brute_force_knn_l2 (benchmark/dataset.ml:15-30) over the vectors the index holds, with the index's metric: the exact ("flat")
 * search, what recall is measured against (Dataset.random, benchmark/dataset.ml:47-58; Recall.compute, :105-127).
 *   - Result: for each query the k smallest of ALL n stored vectors under the total order (distance, node id), ascending, in
 *     out_ids [nq][k] (id_base-based) and out_dist [nq][k].  Among equal distances the lowest ids win and come first.  The
 *     distances are the bits hnsw_distance_batch and the knn searches give for the same pair (same lanes, fmaf order and tree).
 *   - Rows: always the float32 vectors, whatever hnsw_index_info.row_format says: the scan is the ground truth for X, so the
 *     options "half_rows", "byte_rows" and "split_rows" do not change it.
 *   - Graph: none is needed.  An index whose nodes have no edges (deg0 all zero) is scanned like any other; n = 0 gives HNSW_OK
 *     with every entry filled (not HNSW_ERR_EMPTY_INDEX: nothing is walked); k > n: the first n entries are real, the rest filled.
 *     fill: HNSW_FILL_OHNSW = id -1 and distance NaN, HNSW_FILL_BA = id -1 and +inf.
 *   - Limits: k in 1..1024; k < 1 and an unknown fill are HNSW_ERR_BAD_ARG, k > 1024 is HNSW_ERR_UNSUPPORTED.  nq, q_stride and
 *     null pointers as hnsw_search_batch (nq == 0 is a no-op).  NaN in the data or in a query: no promise.
 *   - Determinism: the result does not depend on the batch size, on which queries share a call, or on how the table is cut
 *     into slabs (option "scan_slabs"): no candidate is ever dropped, a full survivor buffer is merged and the scan goes on.
 *   - Host form: as hnsw_search_batch, matrices of hnsw_host_alloc / hnsw_host_register are read and written in place, others are
 *     copied; complete on return.  Device form: asynchronous on `stream`; ONE such call in flight per handle (calls on one
 *     stream are ordered and therefore fine).
 *   - Scratch: the per-slab candidate lists (at most 256 MiB; larger batches are scanned in pieces) belong to the handle, are sized
 *     on demand and reused, and -- like the other scratch of the host-buffer calls -- are NOT counted in device_bytes.
 *   - After hnsw_index_insert the scan covers the grown table.  A replica borrowed from an hnsw_multi may be scanned. */
int32_t hnsw_brute_force_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                               int32_t k, int32_t fill, int32_t *out_ids, float *out_dist);
int32_t hnsw_brute_force_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride,
                                      int32_t k, int32_t fill, int32_t *d_ids, float *d_dist, void *stream);

/* Exact re-ranking of caller-given candidates (the refine step of option "refine" as an operator of its own): for query q the
 * candidates cand[q][0 .. cand_stride) (id_base-based) are evaluated against the FLOAT32 vectors -- whatever
 * hnsw_index_info.row_format says -- and the k smallest under the total order (distance, node id) come back ascending in
 * out_ids [nq][k] (id_base-based) and out_dist [nq][k]: the order of hnsw_brute_force_batch restricted to the candidates, the
 * distance bits of hnsw_distance_batch for the same pair (same lanes, fmaf order and tree).
 *   - Candidates: entries < id_base are padding and skipped (lists may be ragged), as hnsw_search_layer_batch treats start
 *     nodes; the ids of a row must be distinct.  With fewer than k real candidates the first entries are real and the rest
 *     filled: HNSW_FILL_OHNSW = id -1 and distance NaN, HNSW_FILL_BA = id -1 and +inf.
 *   - Limits: cand_stride in 1..1024 (> 1024: HNSW_ERR_UNSUPPORTED), k in 1..cand_stride; k < 1, k > cand_stride and an unknown
 *     fill are HNSW_ERR_BAD_ARG.  nq, q_stride and null pointers as hnsw_search_batch (nq == 0 is a no-op).
 *   - Host form: an id >= id_base + n is HNSW_ERR_BAD_ARG, checked before any launch; matrices of hnsw_host_alloc /
 *     hnsw_host_register are read and written in place, others are copied; complete on return.  Device form: asynchronous on
 *     `stream`, uses no scratch of the handle; an id >= id_base + n is skipped like padding.
 *   - Graph: none is needed (a flat index can be re-ranked); after hnsw_index_insert the new nodes are candidates like any other.
 *   - Determinism: a query's result depends on its own candidates only, not on the batch it is in. */
int32_t hnsw_rerank_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                          const int32_t *cand, int32_t cand_stride, int32_t k, int32_t fill,
                          int32_t *out_ids, float *out_dist);
int32_t hnsw_rerank_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride,
                                 const int32_t *d_cand, int32_t cand_stride, int32_t k, int32_t fill,
                                 int32_t *d_ids, float *d_dist, void *stream);

/* ---- filtered search: the k nearest among the nodes an allow-mask names -------------------------------------------------------
 * THE FILTER.  hnsw_filter_create uploads `bits`, a host array of ceil(n_bits / 32) words (not retained): bit (v & 31) of word
 * (v >> 5) set = the 0-based node v is allowed, whatever id_base is (the node the searches report as v + id_base).  n_bits must be
 * the index's current n (HNSW_ERR_BAD_ARG otherwise); bits at positions >= n in the last word are ignored (the device copy has
 * them clear).  The filter is uploaded once and belongs to the index and the device it was made for; hnsw_filter_count gives the
 * number of allowed nodes (counted on the device at creation).  A filter is refused by the search (HNSW_ERR_BAD_ARG) when it was
 * made for another handle, or when hnsw_index_insert has grown the index since it was made: make a new one.  Destroying the index
 * before its filters is the caller's error, as with requests (hnsw_filter_destroy itself stays valid: it only frees the mask).
 * The mask's bytes are NOT counted in hnsw_index_info.device_bytes.  A filter is not saved with the index.  Any number of
 * filters per index; a filter is never modified by a search.  A mask of the live nodes gives soft deletes without touching a
 * graph table (hnsw_index_remove is the hard deletion; it, like every hnsw_index_insert, makes the filters made before it stale;
 * hnsw_index_mark_deleted is the soft deletion the index keeps itself, across inserts and removals).
 *
 * THE RESULT of hnsw_search_batch_filtered, in terms of public calls only.  Let W_e(q) be the ids hnsw_search_batch returns for
 * (ef = e, k = e) with the caller's semantics (HNSW_SEM_OHNSW / HNSW_SEM_FUNCTOR) -- the host form: exact, tie-overflow repair
 * included; under half or sq8 rows that is the walk over those rows --, and A_e(q) the allowed members of W_e(q), in order.
 *   1. LADDER.  e_0 = ef, e_{j+1} = min(1024, 2 * e_j).  A query is served at the first stage j with |A_{e_j}(q)| >= k.  Only the
 *      queries still short are searched again at the next stage, as one compacted batch.  The walk itself is never filtered: it
 *      is the walk every other entry point runs, over all nodes.
 *   2. EXACT STAGE.  A query still short at e = 1024, and EVERY query when fewer than k nodes are allowed (n_allowed < k: no walk
 *      is made), is answered by the exact scan restricted to the allowed nodes: the k smallest allowed nodes under the total order
 *      (distance, node id), as hnsw_brute_force_batch defines its order and its bits; with fewer than k allowed nodes the first
 *      entries are real and the rest filled per params->fill (HNSW_FILL_OHNSW: id -1, NaN; HNSW_FILL_BA: id -1, +inf).
 *   3. DISTANCES ARE ALWAYS OVER THE FLOAT32 ROWS: the bits of hnsw_distance_batch for the returned ids, whatever
 *      hnsw_index_info.row_format says.
 *        - byte, split and float32 rows: the walk's distances are those bits already: the answer is the first k of A_e(q).
 *        - HNSW_ROWS_HALF and HNSW_ROWS_SQ8: ALL members of A_e(q) are re-ranked over the float32 rows by hnsw_rerank_batch's
 *          kernel and the first k under (distance, node id) are returned; option "refine" does not shorten the list here.  (The
 *          disallowed members of W are handed to that kernel as padding, id_base - 1.)  The stage test is unchanged: at least k
 *          allowed members in W.
 *   4. OUTPUTS.  out_ids [nq][k] (id_base-based), out_dist [nq][k], ascending.  out_stage (optional, [nq]): j for a query served
 *      at ladder stage j, 0xFFFFFFFF for the exact stage.  out_nhops (optional): the sum of the hops of the walks the query took
 *      (0 without a walk).  out_ndist (optional): the sum of those walks' evaluations plus the candidates re-ranked (half / sq8
 *      rows: |A_e(q)| at the stage that served it); for the exact stage that sum plus n_allowed.
 *   5. ERRORS.  k > ef: HNSW_ERR_BAD_ARG; ef > 1024: HNSW_ERR_UNSUPPORTED; HNSW_SEM_FUNCTOR_NEAREST_K: HNSW_ERR_BAD_ARG; an empty
 *      index: HNSW_ERR_EMPTY_INDEX; a null, foreign or outgrown filter: HNSW_ERR_BAD_ARG; nq == 0 is a no-op; null pointers,
 *      q_stride and nq as hnsw_search_batch.  An error leaves the outputs untouched.  Matrices of hnsw_host_alloc /
 *      hnsw_host_register are read and written in place, others are copied, as by the other host forms; complete on return.
 *   6. DETERMINISM.  A query's answer depends on its own vector, the mask and (ef, k, semantics) only: not on the batch it is in,
 *      and not on which stage other queries reached.
 * WITH OPTION filter_collect (hnsw_index_set_option(idx, "filter_collect", 1); k <= 128, float32 / byte / split rows).  For the walk
 * of (ef = e, the caller's semantics) for query q let X_e(q) be the nodes the layer-0 loop expands, and
 *      E_e(q) = {the layer-0 entry node} united with adj0(c) for every c in X_e(q):
 * THE EVALUATED SET, every node whose distance the layer-0 search evaluates.  It is a set: it does not depend on what the visited
 * cache forgets, nor on option "visited_blocks".  Upper-layer evaluations are not collected.  R_e(q) is the first min(k, .) allowed
 * members of E_e(q) under the order of hnsw_brute_force_batch: the ordered distance key (pre-square-root for L2), then the node
 * id; distances are the bits of hnsw_distance_batch.  The ladder is unchanged (e_0 = ef, e_{j+1} = min(1024, 2 * e_j), the short
 * queries compacted and walked as one batch per stage); only THE STAGE TEST changes: a query is served at the first stage where
 * |R_e(q)| >= k, and its answer is R_e(q).  A query still short at 1024 goes to the unchanged exact stage, and a query whose filter
 * allows fewer than k nodes takes no walk and goes there at once.  out_stage, out_nhops and out_ndist mean what they mean above
 * (the sum over the walks taken, plus n_allowed for the exact stage); nothing is re-ranked; the walk itself is the unchanged walk:
 * for a query served at stage j its hop count at that stage is hnsw_search_batch's for (e_j, e_j).  CONSEQUENCES: a query that
 * point 1 serves at stage 0 gets the same row with the option, because every evaluated node outside the final W is at least as
 * far as max(W) -- except where such a node is tied with max(W) at the k-th place, where (key, id) decides --; point 6
 * (DETERMINISM) holds unchanged.  SCOPE: hnsw_search_batch_filtered and hnsw_search_batch_filtered_each; the plain calls that run
 * under marks (hnsw_search_batch and hnsw_knn while n_deleted > 0 remain bit for bit the filtered call under LIVE, now with the
 * same option); through hnsw_sharded_set_option the sharded filtered call, whose definition in terms of the shard handles' own
 * rows is unchanged.  Range search is not affected.  For k > 128 the option has no effect (R lives in two key registers) and
 * points 1 - 6 answer.  Exact-row formats only and not saved with the index: see the option list of hnsw_index_set_option.
 * Scratch (a stage's W, the short list, the gathered queries) belongs to the handle, is sized on demand and not counted in
 * device_bytes: ONE filtered call in flight per handle, and no range call beside it (the short list and the gathered queries are
 * shared between the filtered and the range calls).  There is no device-pointer form: the ladder needs the number of short
 * queries on the host.  Cost: a mask that allows a fraction s of the nodes leaves about s * e members of W; below s ~ k / 1024 most
 * queries end in the exact stage after walking the whole ladder (no threshold skips it: tools/filter_rate.py prints the rates). */
typedef struct hnsw_filter hnsw_filter;
int32_t hnsw_filter_create(hnsw_index *idx, const uint32_t *bits, int64_t n_bits, hnsw_filter **out);
int32_t hnsw_filter_destroy(hnsw_filter *f);
int32_t hnsw_filter_count(const hnsw_filter *f, int64_t *n_allowed);
int32_t hnsw_search_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                   const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                                   uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);

/* ---- one filter per query: a mixed batch of many tenants, categories or time windows in one call ------------------------------
 * THE RESULT of hnsw_search_batch_filtered_each.  Query q is answered under filters[query_filter[q]] (query_filter: a host array
 * of nq values in 0 .. n_filters - 1).  Row q of all five outputs is bit for bit the row a hnsw_search_batch_filtered call with
 * filters[query_filter[q]] and the same params gives that query -- by point 6 (DETERMINISM) of that definition such a row depends on
 * the query's own vector, its mask and (ef, k, semantics) only, so the result is fully defined by public calls.  Everything in
 * points 1 - 6 holds per query, with "the filter" read as "the query's filter":
 *   - A query whose filter allows fewer than k nodes (n_allowed < k) takes no walk and goes to the exact stage: out_stage
 *     0xFFFFFFFF, out_nhops 0, out_ndist = that filter's n_allowed.  The other queries of the batch are not affected by it.
 *   - LADDER.  At each stage, all queries still short, whatever their filters, are walked as ONE compacted batch in ascending
 *     query order, by the same ladder: one launch over all of them per stage, not one per filter.
 *   - EXACT STAGE.  out_ndist adds the n_allowed of the query's own filter.  One masked scan serves all filters: the queries left
 *     are ordered by (filter index, query) and each filter's group is padded to whole tiles of the scan.
 *   - ERRORS (outputs untouched, nothing walked, all checked on the host before any launch).  n_filters < 1, null `filters`, or
 *     null `query_filter` with nq > 0: HNSW_ERR_BAD_ARG.  ANY entry of `filters` null, made for another handle, or outgrown by
 *     hnsw_index_insert: HNSW_ERR_BAD_ARG, whether or not a query names it.  A query_filter value outside 0 .. n_filters - 1:
 *     HNSW_ERR_BAD_ARG.  Everything else as hnsw_search_batch_filtered: k > ef, ef > 1024 (HNSW_ERR_UNSUPPORTED),
 *     HNSW_SEM_FUNCTOR_NEAREST_K, an empty index (HNSW_ERR_EMPTY_INDEX), nq == 0 is a no-op (then query_filter may be null),
 *     strides, null buffers.
 *   - A handle may appear twice in `filters`.  There is no upper limit on n_filters beyond memory.
 * Scratch and the rule "ONE filtered call in flight per handle, no range call beside it" are unchanged.  hnsw_search_batch_filtered
 * is the case "table of one filter, no query_filter" of the same driver.
 *
 * FILTERS FROM LABELS.  hnsw_filter_create_by_label makes n_labels filters from one label per node (labels: a host array of n
 * values, not retained): out[l] allows node v (0-based, whatever id_base is) iff labels[v] == l.  n must be the index's current n,
 * n_labels >= 1, each label in -1 .. n_labels - 1, where -1 means the node is in no filter; any other value is HNSW_ERR_BAD_ARG,
 * found on the host before anything is allocated.  All or nothing: on any error out[0 .. n_labels) are all NULL and nothing stays
 * allocated.  On success every out[l] is an ordinary hnsw_filter: its own object, destroyed on its own with hnsw_filter_destroy,
 * counted (hnsw_filter_count), accepted by both filtered entry points, bound to the handle and its n like any other.  A label no
 * node carries gives a filter of count 0.  The labels are uploaded once and one pass over them on the device builds all masks and
 * counts.  Cost: n_labels * ceil(n / 32) * 4 bytes on the device, NOT counted in hnsw_index_info.device_bytes.
 *
 * hnsw_filter_bits copies the mask of a filter made either way back to the host: ceil(n / 32) words in hnsw_filter_create's layout,
 * the bits past n clear (for tests and for callers that persist masks).  Null arguments: HNSW_ERR_BAD_ARG. */
int32_t hnsw_search_batch_filtered_each(hnsw_index *idx, const hnsw_filter *const *filters, int32_t n_filters,
                                        const int32_t *query_filter, const float *queries, int64_t nq, int64_t q_stride,
                                        const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                                        uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);
int32_t hnsw_filter_create_by_label(hnsw_index *idx, const int32_t *labels, int64_t n, int32_t n_labels, hnsw_filter **out);
int32_t hnsw_filter_bits(const hnsw_filter *f, uint32_t *out);

/* ---- range search: every stored vector within a radius of the query -----------------------------------------------------------
 * The other standard question of a vector index: not "the k nearest" but ALL nodes within distance `radius` (de-duplication,
 * similarity thresholds, density queries, range recall).  The result has no fixed k -- 0 to n ids per query -- and is an object
 * that owns its device buffers (hnsw_range_result): lims [nq + 1] (lims[0] = 0, lims[nq] = total), ids and distances [total];
 * query q's SEGMENT is ids / dist [lims[q], lims[q + 1]).
 *
 * THE RESULT of the range calls, in terms of public calls only.
 *   1. IN RANGE.  Node v is in range of q iff the float distance the library returns for the pair is <= radius: the bits of
 *      hnsw_distance_batch (L2 after the square root, inner product as 1 - <a,b>), for both entry points.  Keys are monotone in
 *      distance, so under the scan's order the in-range nodes are a prefix.  A NaN radius is HNSW_ERR_BAD_ARG; a radius below every
 *      distance gives empty segments (lims[q + 1] == lims[q]); +inf gives everything.
 *   2. ORDER.  Every segment is ascending in the order hnsw_brute_force_batch returns: ordered distance key, then node id --
 *      (distance, node id).  Ids are id_base-based.  DISTANCES ARE ALWAYS OVER THE FLOAT32 ROWS, whatever
 *      hnsw_index_info.row_format says.
 *   3. hnsw_range_brute_force_batch.  The segment of q is exactly the in-range prefix of the full order over all n rows (what
 *      hnsw_brute_force_batch would return for k = n).  No graph is needed; n = 0 gives HNSW_OK with all segments empty; row formats
 *      and options never change it (option "scan_slabs" cuts the table, results do not depend on it).  out_stage is 0xFFFFFFFF,
 *      out_ndist is n, out_nhops is 0.
 *   4. hnsw_range_search_batch.  Let W_e(q) be what hnsw_search_batch returns for (ef = e, k = e) under the caller's rule
 *      (HNSW_SEM_OHNSW / HNSW_SEM_FUNCTOR) -- the host form: exact, tie-overflow repair included.  Under HNSW_ROWS_HALF and
 *      HNSW_ROWS_SQ8 W_e is the walk over those rows, and then ALL its members are re-ranked over the float32 rows by
 *      hnsw_rerank_batch's kernel with k := e; option "refine" does not shorten the list.
 *        LADDER.  e_0 = ef, e_{j+1} = min(1024, 2 * e_j).  A query is SERVED at the first stage j where W_{e_j}(q) is not saturated:
 *      |W| < e_j (the walk ran out of graph), or its last member's distance is > radius.  The segment of a served query is the
 *      in-range prefix of that W.  Only the queries still saturated are walked again, as one compacted batch in ascending query
 *      order.  The walk is never modified: it is the walk every other entry point runs.
 *        EXACT STAGE.  A query saturated at e = 1024 gets the exact segment of hnsw_range_brute_force_batch; its stage is 0xFFFFFFFF.
 *   5. COUNTERS (hnsw_range_result_fetch, each optional, [nq]).  out_stage: j for a query served at ladder stage j, 0xFFFFFFFF for
 *      the exact stage.  out_nhops: the sum of the hops of the walks taken.  out_ndist: the sum of those walks' evaluations, plus
 *      |W_e| for every stage that re-ranked (half and sq8 rows), plus n for the exact stage.
 *   6. ERRORS.  An error leaves *out NULL and nothing allocated.  ef < 1: HNSW_ERR_BAD_ARG; ef > 1024: HNSW_ERR_UNSUPPORTED;
 *      HNSW_SEM_FUNCTOR_NEAREST_K: HNSW_ERR_BAD_ARG; an empty graph: HNSW_ERR_EMPTY_INDEX (the search only, not the brute-force form);
 *      nq == 0: HNSW_OK with a valid empty result; null pointers, q_stride and nq as hnsw_search_batch.  A call whose total exceeds
 *      2^31 - 1 results: HNSW_ERR_UNSUPPORTED, found after counting and before any result buffer is allocated.  Allocation failure:
 *      HNSW_ERR_OOM.
 *   7. DETERMINISM.  A query's answer depends on its own vector and (radius, ef, semantics) only: not on the batch it is in, and not
 *      on which stage other queries reached.
 * Buffers.  Query matrices of hnsw_host_alloc / hnsw_host_register are read in place, others are staged; complete on return.  Scratch
 * (every stage's W, the saturated list, the gathered queries, the scan's counts, offsets and unsorted hits: 16 bytes per hit of the
 * exact stage) belongs to the handle, is sized on demand and not counted in device_bytes: ONE range call in flight per handle, and no
 * filtered call beside it (the list and the gathered queries are shared between the range and the filtered calls).  The
 * result's own buffers belong to the result: any number of results may be alive, and a result outlives later calls (destroy it before
 * or after the index, as convenient: it holds no reference to the handle).  There is no device-pointer form: the ladder needs the
 * number of saturated queries, and the result its total, on the host.  A replica of an hnsw_multi may be searched through its handle
 * (hnsw_multi_replica).  After hnsw_index_insert the new nodes are found like any other.
 * Cost: the exact stage reads the table twice (count, then fill) and sorts only its hits; a batch so large that its per-(query,
 * slab) counts exceed the scan's 256 MiB of scratch is scanned in pieces, and then counts each piece once more before filling it
 * (tools/range_rate.py prints the rates). */
typedef struct hnsw_range_params {
    float radius;      /* in range: distance <= radius                                              */
    int32_t ef;        /* the ladder's first stage, 1..1024                                         */
    int32_t semantics; /* HNSW_SEM_OHNSW or HNSW_SEM_FUNCTOR                                        */
} hnsw_range_params;
typedef struct hnsw_range_result hnsw_range_result;   /* owns its device buffers; any number may be alive */
int32_t hnsw_range_search_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                                const hnsw_range_params *params, hnsw_range_result **out);
/* exact; no graph needed */
int32_t hnsw_range_brute_force_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                                     float radius, hnsw_range_result **out);
int32_t hnsw_range_result_size(const hnsw_range_result *r, int64_t *nq, int64_t *total);
/* lims [nq + 1] (lims[0] = 0, lims[nq] = total), ids / dist [total], counters [nq]; every pointer may be NULL */
int32_t hnsw_range_result_fetch(hnsw_range_result *r, int64_t *lims, int32_t *ids, float *dist,
                                uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);
/* borrowed device pointers, valid until destroy (for callers that go on working on the device); each may be NULL */
int32_t hnsw_range_result_device(hnsw_range_result *r, const int64_t **d_lims, const int32_t **d_ids, const float **d_dist);
int32_t hnsw_range_result_destroy(hnsw_range_result *r);   /* NULL is HNSW_OK */

/* ---- range search under an allow-mask -------------------------------------------------------------------------------------------
 * THE RESULT of the filtered range calls, in terms of public calls only.  f is a filter of hnsw_filter_create /
 * hnsw_filter_create_by_label; "the unfiltered call" is hnsw_range_search_batch for hnsw_range_search_batch_filtered and
 * hnsw_range_brute_force_batch for hnsw_range_brute_force_batch_filtered, with the same other arguments.
 *   1. SEGMENT.  Query q's segment is the segment the unfiltered call gives q, with the nodes f does not allow left out and the
 *      order kept: ids and distance bits of the allowed members are those of the unfiltered call.
 *   2. STAGE AND HOPS.  The ladder's stage test is the unfiltered one: W_e(q) is saturated iff all e entries are real and in range,
 *      whatever the mask says.  So out_stage and out_nhops equal the unfiltered call's.  Under HNSW_ROWS_HALF and HNSW_ROWS_SQ8 all
 *      of W is re-ranked first, as in the unfiltered call; the mask is applied after.
 *   3. EVALUATIONS.  out_ndist equals the unfiltered call's, except that the exact stage adds the filter's n_allowed instead of n
 *      (the brute-force form: out_ndist is n_allowed).
 *   4. NO WALK.  A filter that allows no node takes no walk: every segment is empty, out_stage is 0xFFFFFFFF, and both counters are 0.
 *   5. ERRORS as the unfiltered call (NaN radius, ef, semantics, HNSW_ERR_EMPTY_INDEX for the search form, nq == 0, the 2^31 - 1
 *      cap), plus the filtered search's filter checks: a null, foreign or stale filter (made for another handle, or before the
 *      index last changed) is HNSW_ERR_BAD_ARG.  An error leaves *out NULL.
 *   6. SINGLE FILTER ONLY: per-query filters and per-query radii are not built.
 * This is done on the device, not as a host post-filter: a disallowed hit is never counted, stored, sorted or held against the
 * 2^31 - 1 cap, and the exact stage steps over a mask word without a set bit without loading its 32 rows, as the masked k-scan
 * does.  Scratch, "ONE range call in flight per handle" and the result object are those of the unfiltered calls, which are the case
 * "no mask" of the same driver. */
int32_t hnsw_range_search_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                         const hnsw_range_params *params, hnsw_range_result **out);
int32_t hnsw_range_brute_force_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq,
                                              int64_t q_stride, float radius, hnsw_range_result **out);

/* ---- the layer-level functions of the path, as batched operators -------------------------------
 * hnsw_search_layer_batch = Ohnsw.search_k (lib/ohnsw.ml:543-588; params->semantics = OHNSW) or
 * Hnsw_algo.Search.search (lib/hnsw_algo.ml:350-391; FUNCTOR) on ONE layer from explicit start
 * nodes -- what Ohnsw.knn calls on layer 0 (:872-874) and what the builder calls on every layer
 * (lib/ohnsw.ml:811, lib/hnsw_algo.ml:663).  For target q: W is seeded with start_nodes[q][*]
 * (id_base-based; entries < id_base are skipped, so lists may be ragged; distinct ids;
 * 1 <= n_start <= ef, the only shape the reference produces), the layer is searched with W
 * bounded by params->ef, and W[0..k) comes back ascending in out_ids/out_dist [nq][k] with
 * out_cnt[q] = min(|W|, k) (optional).  A start node that does not exist on `layer` has no
 * neighbours there (MapGraph.adjacent of a missing node is empty, lib/hnsw.ml:146-149). */
int32_t hnsw_search_layer_batch(hnsw_index *idx, int32_t layer, const float *targets, int64_t nq,
                                int64_t t_stride, const int64_t *start_nodes, int32_t n_start,
                                const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                                int32_t *out_cnt, uint32_t *out_ndist, uint32_t *out_nhops);

/* hnsw_search_one_batch = Ohnsw.search_one (= search_one_simple, lib/ohnsw.ml:492-512); also the
 * result of Hnsw_algo.Search.search_one (lib/hnsw_algo.ml:393-437), which reaches the same node by
 * an ef = 1 search.  Greedy walk on `layer` from start[q]: scan all neighbours of the current
 * node, move to the nearest one if it is strictly closer (:502), until no change.
 * out_node [nq] id_base-based; out_dist [nq] (optional) its distance (the value_distance the
 * functor version carries down, lib/hnsw_algo.ml:1005). */
int32_t hnsw_search_one_batch(hnsw_index *idx, int32_t layer, const float *targets, int64_t nq,
                              int64_t t_stride, const int64_t *start, int64_t *out_node,
                              float *out_dist);

/* ---- one host process, several GPUs ------------------------------------------------
 * An OCaml program is ONE process: this is the form of BASELINE.json's "replicated index, query batch
 * sharded across the GPUs of one node, RCCL all-gather of per-shard results over xGMI" it can reach.
 * The index is REPLICATED on every listed device; a query batch is split into n_devices contiguous
 * shards [g*nq/G, (g+1)*nq/G), shard g is uploaded to and searched on device g (all devices
 * concurrently, one HIP stream each), and ONE exchange -- ncclAllGather on communicators from
 * ncclCommInitAll (in-place; unequal shards: one ncclBroadcast per shard inside the same group) --
 * leaves the full [nq][k] ids and distances resident on EVERY device.  Results are bit-identical to
 * hnsw_search_batch on one device (each query is an independent traversal, lib/ohnsw.ml:883-895), the
 * exactness fallback for tie-list overflow runs per shard before the exchange.
 * RCCL is bound at first use (dlopen librccl.so.1).  A device may be listed more than once (several
 * replicas on one GPU: a test arrangement); RCCL refuses that, the exchange is then device-to-device
 * copies.  The library pins nothing of the caller's: the shard uploads run at PCIe speed when the caller registered its
 * query matrix with hnsw_host_register (its lifetime, not the library's) and are staged by the runtime otherwise.
 * ERRORS.  A search that fails before the exchange leaves nothing enqueued.  If the exchange itself is refused part-way (one
 * device's collective not accepted inside the group) the library ABORTS the handle's communicators (ncclCommAbort) before it
 * returns HNSW_ERR_HIP, so no device is left waiting for a peer that never joins; the result tables of that call are undefined
 * and the next search on the handle creates new communicators.
 * (One process PER GPU, each with its own RCCL rank, is the other deployment:
 * ocaml-hnsw_amd/sharding.py and bench.py.) */
typedef struct hnsw_multi hnsw_multi;
int32_t hnsw_multi_create(const hnsw_index_desc *desc, const int32_t *devices, int32_t n_devices,
                          hnsw_multi **out);
int32_t hnsw_multi_destroy(hnsw_multi *m);
int32_t hnsw_multi_num_replicas(const hnsw_multi *m, int32_t *n_devices);
/* replica g (borrowed: destroyed with the hnsw_multi) */
int32_t hnsw_multi_replica(hnsw_multi *m, int32_t g, hnsw_index **out);
/* Ohnsw.knn_batch_bigarray / Hnsw.Ba.knn_batch over all replicas, host arrays in and out: the host
 * receives the table from one device after the exchange. */
int32_t hnsw_multi_search_batch(hnsw_multi *m, const float *queries, int64_t nq, int64_t q_stride,
                                const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                                uint32_t *out_ndist, uint32_t *out_nhops);
/* The same with the results left on the devices: on return (synchronised) d_ids[g] / d_dist[g],
 * g < n_devices, point to device g's copy of the full [nq][k] table (library-owned, valid until the
 * next search on this handle).  d_ids / d_dist are caller arrays of n_devices pointers (either may be
 * NULL). */
int32_t hnsw_multi_search_batch_device(hnsw_multi *m, const float *queries, int64_t nq, int64_t q_stride,
                                       const hnsw_search_params *params, int32_t **d_ids, float **d_dist);
/* What the exchanges of this handle were made of so far (tests, debugging): out4 = { ncclAllGather calls, ncclBroadcast
 * calls (unequal shards, and the re-send of a repaired shard), device-to-device copies (replicas sharing a device),
 * shards searched again by the exactness fallback }, each summed over the devices. */
int32_t hnsw_multi_debug_counters(const hnsw_multi *m, int64_t *out4);
/* device g's copy of the last device-resident result, copied to host arrays [nq][k] (tests, debugging) */
int32_t hnsw_multi_copy_result(hnsw_multi *m, int32_t g, int32_t *out_ids, float *out_dist);

/* ---- graph construction on the device (next-row scope: the reference's builder stays OCaml;
 * this entry point exists so an index can also be produced where no OCaml build is at hand,
 * e.g. by bench.py).  Batched restatement of Ohnsw.build_batch_bigarray (lib/ohnsw.ml:840-857):
 * same level law, same per-node steps (search_one descent, search_k with efConstruction,
 * select_neighbours with M / 2M, symmetric links, shrink), nodes inserted in batches against
 * the graph as of batch start.  Deterministic for a given seed. */
typedef struct hnsw_build_params {
    int32_t num_connections;               /* M   (~num_connections, lib/ohnsw.ml:841)          */
    int32_t num_nodes_search_construction; /* efConstruction                                   */
    int32_t metric;
    int32_t id_base;
    uint64_t seed;                         /* level draws (own RNG)                            */
    int32_t max_batch;                     /* 0 = default (8192)                               */
    int32_t batch_div;                     /* batch <= nodes already inserted / batch_div; 0 = 16 */
    int32_t expected_ef;                   /* as hnsw_index_desc.expected_ef: 0 = not known      */
    int32_t expected_semantics;
} hnsw_build_params;

int32_t hnsw_build(const float *vectors, int64_t n, int32_t d, int64_t row_stride,
                   const hnsw_build_params *params, int32_t device, hnsw_index **out);

/* Ohnsw.insert (lib/ohnsw.ml:766-837) for m vectors, on the device, into an index this library holds (made by
 * hnsw_index_create, hnsw_build or hnsw_index_load); the fold of build_batch_bigarray (:840-857) continued.
 *   - Ids: the new nodes get ids n_old .. n_old+m-1 (plus id_base), in row order.  m == 0 is a no-op (HNSW_OK).
 *   - Each new node goes through hnsw_build's per-node steps (level draw, search_one descent, search_k with efConstruction,
 *     select_neighbours with M / 2M on layer 0, symmetric links, shrink), batched exactly as hnsw_build batches (max_batch,
 *     batch_div, a node that raises max_layer ends its batch), continuing from position n_old: the same code runs both.
 *   - Levels: node i's level is the draw hnsw_build with the same seed gives node i (splitmix64 of the state
 *     seed + i * 0x9E3779B97F4A7C15; node 0 draws nothing).  So build(X[:a]) then inserts of X[a:b], X[b:] with max_batch 1
 *     equal hnsw_build(X) with max_batch 1 link for link, however the inserts are split; with default batching they do when a
 *     is a batch boundary of hnsw_build(X)'s schedule.  Inserting into an empty index equals hnsw_build of the same vectors.
 *   - params: metric and id_base must be the index's (HNSW_ERR_BAD_ARG); num_connections 2..32 and
 *     num_nodes_search_construction 1..512 as for hnsw_build; the vectors have the index's d, row_stride >= d.
 *   - Row widths: rows narrower than the insert needs (max_degree0 < 2M, max_degree < M: e.g. a graph flattened from OCaml,
 *     whose widths are its longest lists) are widened to 2M / M first, order kept; wider rows (max_degree0 > 2M, or
 *     max_degree > M with an upper layer) are refused (HNSW_ERR_BAD_ARG).
 *   - expected_ef / expected_semantics: as for hnsw_build.  Shapes prepared before (hnsw_index_prepare) are prepared again.
 *   - Refused (HNSW_ERR_BAD_ARG): a handle with submitted requests not yet waited for; a replica owned by an hnsw_multi (the
 *     other replicas would not follow); a device fallback slab (option device_fallback_slab_bytes) that holds no query of the
 *     grown index.  Work on caller streams (hnsw_search_batch_device) is waited for before any table is freed.
 *   - What the handle derived from its graph follows it: byte rows (kept only if old and new vectors are all byte-valued),
 *     split rows (rebuilt; not after option split_rows -1), locality codes (new node v gets code v), the options' effects.
 *     The device fallback slab keeps its bytes and so holds fewer queries (bytes / (4 n)).
 *   - All or nothing: on ANY error (including HNSW_ERR_OOM) the index is exactly as before.  The grown tables are built beside
 *     the old ones and swapped in at the end, so at its peak the call holds two copies of the index on the device. */
int32_t hnsw_index_insert(hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride,
                          const hnsw_build_params *params);

/* ---- hard deletion: hnsw_index_remove takes nodes out of the index and repairs the graph on the device --------------------------
 * A mask of the live nodes (hnsw_filter_create) is the soft half of deletion: the dead rows stay in device memory and every walk
 * still pays for them.  hnsw_index_remove is the hard half: the m stored nodes `ids` (id_base-based, distinct; m == 0 is a no-op
 * that only fills out_new_id with the identity) leave the index, which afterwards holds n = n_old - m nodes, the graph repaired as
 * defined below -- in terms of hnsw_select_neighbours_batch and hnsw_distance_batch, so the result can be checked link for link.
 * out_new_id (optional, [n_old]): the new id_base-based id of old node v; for a removed node id_base - 1.
 *
 *   NUMBERING.  D is the removed set, L the rest.  Live nodes keep their order: new(v) = v - |{d in D : d < v}|.  Vectors,
 *     levels and every row move accordingly.
 *   REPAIR, per layer l (layer 0 with cap = max_degree0, layers >= 1 with cap = max_degree).  It reads the OLD tables only, so
 *     the result depends on no processing order (and on no atomic arrival order).  A live node u on layer l is TOUCHED when its
 *     row on l lists a removed node.  An untouched live row is copied, renumbered, order kept.  For a touched u:
 *       live(u) = the live entries of u's row, in row order.
 *       C(u)    = u's removed neighbours walked in row order, each one's row on l in row order: every live w that is not u, not
 *                 in live(u) and not already taken (the first occurrence counts).  The walk stops once |live(u)| + |C(u)| = 1024.
 *                 Removed neighbours of removed neighbours are not followed.
 *     1. PROPOSE.  S(u) = what hnsw_select_neighbours_batch returns after the forced entries for: target = u's vector,
 *        candidates = live(u) then C(u), num_neighbours = cap, keep_all_if_few = 0, cand_degree = 0 for live(u) (forced, kept in
 *        order) and 2 for C(u).  (The heuristic with live(u) already kept: C(u) is taken in (distance, id) order, the test is
 *        strict and is made against the forced entries too.)
 *     2. OFFER.  U(u) = S(u) united with { touched w on l : u in S(w), w not in live(u) }, ordered by
 *        (hnsw_distance_batch(u's vector, w), id); T(u) = its first cap - |live(u)| entries.
 *     3. AGREE.  new(u) = the w in T(u) with u in T(w), in T's order.  (An untouched w has no T: it takes no new link.  In a
 *        symmetric graph every member of C(u) is touched.)
 *     The new row of u is live(u) followed by new(u), renumbered.  Consequences: no live link is ever dropped; degrees stay within
 *     the caps; a symmetric graph stays symmetric (Graph.Test.invariant, which hnsw_index_insert relies on); a node whose
 *     neighbours all die, and whose dead neighbours had no other live neighbour, is left with degree 0 and shows up in
 *     hnsw_index_layer_isolated.
 *   LEVELS, TOP, ENTRY.  Live nodes keep their levels.  max_layer becomes the highest live level.  The entry point is the old one
 *     if it is live, else the lowest-id live node of the highest live level.  The upper tables are laid out again for the live
 *     nodes.  Removing every node gives the empty index: searches answer HNSW_ERR_EMPTY_INDEX, and an insert into it equals
 *     hnsw_build of the same vectors.  Later inserts draw levels for positions n.. as documented there: numbering continues from
 *     the shrunk n.
 *   REFUSALS, each checked before anything is built, the index untouched: HNSW_ERR_BAD_ARG for null ids with m > 0, m < 0, an id
 *     out of range or a duplicate id; for a handle with submitted requests not yet waited for; for a replica of an hnsw_multi;
 *     for a graph whose upper rows list a node that is not on that layer or whose entry point is not on the top layer (the check
 *     hnsw_index_insert makes).  A null handle: HNSW_ERR_BAD_ARG, out_new_id untouched.
 *   ALL OR NOTHING, as hnsw_index_insert: the new tables are built beside the old ones, then hipDeviceSynchronize, then swapped.
 *     On any error (HNSW_ERR_OOM included) the index is exactly as before; at its peak the call holds two copies of the index and
 *     the repair's scratch (per touched node of a layer: two rows of 64 ids and 2 * cap proposal keys of 8 bytes).
 *   WHAT FOLLOWS THE GRAPH, as after an insert: byte rows (they may now APPEAR, if only byte-valued vectors are left), split rows,
 *     half rows and sq8 rows while their option is on (sq8 quantises the whole remaining table again: lo and scale may change);
 *     the locality codes are dropped and rebuilt on demand; prepared shapes are prepared again; the device fallback slab holds
 *     bytes / (4 n) queries of the smaller n; device_bytes follows the new tables.
 *   FILTERS.  The handle has a graph epoch that every successful hnsw_index_insert and hnsw_index_remove moves on; a filter
 *     records the epoch it was made in and is refused (HNSW_ERR_BAD_ARG) once it differs -- also after "remove 5, insert 5", where
 *     n alone would let a stale mask through.  Make a new one.  Range results (hnsw_range_result) alive across a remove keep the
 *     OLD ids; out_new_id translates them. */
int32_t hnsw_index_remove(hnsw_index *idx, const int64_t *ids, int64_t m, int32_t *out_new_id);

/* ---- soft deletion owned by the index: mark, search around, compact -------------------------------------------------------------
 * hnsw_index_remove is a rebuild-sized call; nobody makes it per deleted item.  hnsw_index_mark_deleted deletes cheaply now --
 * a few bits on the device -- and hnsw_index_compact pays for the repair later.  Unlike a caller-made mask of the live nodes, the
 * marks survive hnsw_index_insert and hnsw_index_remove, and the plain entry points honour them without being told.
 *
 *   THE MARKS.  The handle owns a device mask of the LIVE (not marked) nodes and an internal filter over it, both allocated on the
 *     first mark and NOT counted in hnsw_index_info.device_bytes, as no filter is.  hnsw_index_mark_deleted marks the m stored
 *     nodes `ids` (id_base-based); hnsw_index_unmark_deleted makes them live again.  Marking a marked node or unmarking a live one is
 *     allowed and does nothing; m == 0 is a no-op.  Refused with HNSW_ERR_BAD_ARG, the index untouched, everything checked on the host
 *     first: an id out of range, a duplicate within the call, null ids with m > 0, m < 0; a handle with submitted requests not yet
 *     waited for; a replica of an hnsw_multi (as hnsw_index_insert refuses them).  hnsw_index_deleted_count gives the number of
 *     marked nodes; hnsw_index_deleted_bits copies the marks to the host: ceil(n / 32) words, bit (v & 31) of word (v >> 5) set =
 *     the 0-based node v is marked, the bits past n clear.
 *   EPOCH.  A successful call that changes at least one bit moves the handle's graph epoch on: filters made before it are refused
 *     (HNSW_ERR_BAD_ARG) like filters made before an insert -- their masks may allow a node that is marked now.
 *   GRAPH.  Marked nodes stay in the graph.  Every walk still goes through them, so no region is cut off; they are only never
 *     returned.
 *   WHAT HONOURS THE MARKS, only while n_deleted > 0.  Let LIVE be the filter of the unmarked nodes.
 *     - hnsw_search_batch, hnsw_knn: rows (ids, distances, out_ndist, out_nhops) are bit for bit those of
 *       hnsw_search_batch_filtered under LIVE with the same params: ladder, exact stage, fill, half / sq8 rule and all.
 *       HNSW_SEM_FUNCTOR_NEAREST_K: HNSW_ERR_BAD_ARG.  hnsw_knn's *out_count = the real entries.
 *     - hnsw_brute_force_batch, hnsw_brute_force_batch_device: the k smallest LIVE nodes under (distance, node id), the rest filled.
 *     - hnsw_range_search_batch, hnsw_range_brute_force_batch: their _filtered forms under LIVE.
 *     - hnsw_filter_create, hnsw_filter_create_by_label: the mask is ANDed with the live mask at creation, on the device (a marked
 *       node's label counts as -1); hnsw_filter_count and hnsw_filter_bits report the ANDed mask.  So a current filter already
 *       excludes the marked nodes, and hnsw_search_batch_filtered, hnsw_search_batch_filtered_each and the filtered range calls run
 *       unchanged code.
 *     - hnsw_index_insert: accepted.  Marks keep their positions, the new nodes are live, and the live mask grows inside the
 *       all-or-nothing swap.
 *     - hnsw_index_remove: accepted.  The marks move with their nodes under out_new_id's numbering, a removed marked node is gone,
 *       and the new mask is built before the swap.
 *     - hnsw_search_batch_device, hnsw_search_batch_h2d, hnsw_search_submit: HNSW_ERR_UNSUPPORTED ("compact or unmark first"):
 *       these forms cannot run the ladder.
 *     - hnsw_index_save: HNSW_ERR_BAD_ARG ("marked nodes are not saved: compact or unmark first").  A file that resurrects deleted
 *       vectors is the one outcome to rule out, and the format does not change.
 *   NOT AFFECTED: the calls that take explicit ids (hnsw_distance_batch, hnsw_rerank_batch, hnsw_select_neighbours_batch), the
 *     layer operators (hnsw_search_layer_batch, hnsw_search_one_batch), the exports, hnsw_index_get_info (n stays the stored
 *     count), the layer stats and the locality codes; hnsw_multi searches (a replica cannot be marked).
 *   EVERY NODE MARKED: the searches fill every row and the range segments are empty; this is not HNSW_ERR_EMPTY_INDEX.
 *   COUNT BACK AT 0 (unmark, or compact): the handle takes the plain paths again, results are bit for bit those of a handle never
 *     marked, and the device forms and hnsw_index_save are accepted again.
 *   hnsw_index_compact is hnsw_index_remove(idx, the marked ids ascending, n_deleted, out_new_id): same repair, same refusals, all
 *     or nothing.  Afterwards nothing is marked.  With nothing marked it fills out_new_id (optional, [n]) with the identity.
 *   NOT BUILT: device forms under marks, saved marks, filters that survive a mark.
 * Cost: a marked index is searched by the filtered ladder, several times slower than the plain call until compacted
 * (tools/soft_delete_rate.py prints the rates). */
int32_t hnsw_index_mark_deleted(hnsw_index *idx, const int64_t *ids, int64_t m);
int32_t hnsw_index_unmark_deleted(hnsw_index *idx, const int64_t *ids, int64_t m);
int32_t hnsw_index_deleted_count(const hnsw_index *idx, int64_t *n_deleted);
int32_t hnsw_index_deleted_bits(const hnsw_index *idx, uint32_t *out);   /* ceil(n/32) words, bit v = node v is marked */
int32_t hnsw_index_compact(hnsw_index *idx, int32_t *out_new_id);        /* hnsw_index_remove of the marked nodes */

/* select_neighbours as a batched operator (Ohnsw.select_neighbours lib/ohnsw.ml:647-663;
 * keep_all_if_few = 1 adds the functor path's "#candidates <= M returns them all" shortcut,
 * lib/hnsw_algo.ml:596-599).  For each of nb target vectors: the candidates (ids, id_base-based)
 * are ordered by (distance to the target, id) and kept iff strictly closer to the target than
 * to every neighbour kept so far; at most num_neighbours are kept.  out [nb][num_neighbours] in
 * selection order (nearest first), -1 padded. */
int32_t hnsw_select_neighbours_batch(hnsw_index *idx, const float *targets, int64_t nb, int64_t t_stride,
                                     const int32_t *cand, const int32_t *cand_cnt, int32_t cand_stride,
                                     int32_t num_neighbours, int32_t keep_all_if_few,
                                     const int32_t *cand_degree /* NULL, or [nb][cand_stride]: ~do_not_isolate:true,
                                        candidates whose degree is <= 1 are kept unconditionally, hnsw_algo.ml:591-592 */,
                                     int32_t *out, int32_t *out_cnt);

/* Export of the flattened graph held by an index (inverse of hnsw_index_create): ids
 * id_base-based, rows compacted, -1 padded. */
int32_t hnsw_index_export_layer0(const hnsw_index *idx, int32_t *deg0, int32_t *nbr0);
int32_t hnsw_index_export_upper_count(const hnsw_index *idx, int32_t layer, int64_t *n_nodes);
int32_t hnsw_index_export_upper(const hnsw_index *idx, int32_t layer, int64_t *nodes, int32_t *deg,
                                int32_t *nbr);

/* The locality codes behind the option "visited_blocks" (built on first use or by this call): out[v] = position of node v
 * (0-based, whatever id_base is) in an order that keeps graph-close nodes together -- a permutation of 0 .. n-1 derived
 * from the index's own upper layers (ocaml-hnsw_amd/csrc/hnsw_locality.hip).  Introspection and tests; the search never
 * hands codes out.  HNSW_ERR_UNSUPPORTED when the index has no upper layer to derive an order from. */
int32_t hnsw_index_locality_codes(hnsw_index *idx, int32_t *out);
/* Which visited structure the knn kernel of this handle uses for searches with this ef and accept rule (params->semantics):
 * *log2_slots = 0: the tag cache; else the bitmap-block directory has 2^*log2_slots slots (256 codes each).  With the option
 * "visited_blocks" at -1 the first call for a kernel shape makes the measurement described there (as the first search would):
 * a program that must not meet a device synchronisation inside its first search (a latency-critical path, a stream capture)
 * calls this once per ef at set-up. */
int32_t hnsw_index_visited_blocks(hnsw_index *idx, const hnsw_search_params *params, int32_t *log2_slots);

/* Everything a handle does ONCE for searches with these parameters, done now instead of inside the first such search call:
 * the visited-structure decision of option "visited_blocks" at -1 (building the locality codes and the measurement: 0.1-1.3 s
 * and a device synchronisation for an eligible shape), the kernel variant's residency query, and loading the code object of
 * the variant's translation unit (one query searched and discarded: ~1.4 ms).  hnsw_index_create / hnsw_build call it for
 * desc->expected_ef / params->expected_ef; hnsw_index_load for every shape the saved handle had prepared.  Any number of
 * parameter sets may be prepared; preparing is never needed for correctness.  The measurement draws its 256 probe queries from
 * midpoints between a stored vector and its first layer-0 neighbour (in-distribution, not themselves stored); an index whose
 * real queries come from elsewhere can still be steered with option "visited_blocks" 0 / 1.  Results never depend on any of it. */
int32_t hnsw_index_prepare(hnsw_index *idx, const hnsw_search_params *params);

/* Per-layer degree statistics: Hgraph.Stats.compute (lib/hnsw.ml:353-375; printed by
 * benchmark/benchmark.ml:70-71): layer size (layer_sizes) and the layer's mima record -- min / max / mean of the
 * neighbour-list lengths, the nodes without a neighbour.  Computed on the device from the resident tables.  The keys of
 * layer l >= 1 are the nodes inserted at level >= l.  A layer without nodes yields what the reference's fold yields:
 * min 1000000, max -1, mean nan. */
typedef struct hnsw_layer_stats {
    int64_t num_nodes;     /* layer_sizes */
    int32_t min_degree, max_degree;
    double mean_degree;
    int64_t num_isolated;  /* length of mima.isolated */
} hnsw_layer_stats;
int32_t hnsw_index_layer_stats(const hnsw_index *idx, int32_t layer, hnsw_layer_stats *out);
/* mima.isolated of that layer: the node ids (id_base-based) in the reference's list order -- min_max_connectivity
 * conses a key onto the list as the ascending Map.fold meets it (lib/hnsw.ml:364-366), so the list is DESCENDING.
 * *count = length of the list; the first min(cap, *count) ids are written (cap = 0, ids = NULL: count only). */
int32_t hnsw_index_layer_isolated(const hnsw_index *idx, int32_t layer, int64_t *ids, int64_t cap, int64_t *count);

/* Flattened-index file (new: the reference has no persistence; its types derive sexp but values
 * are sexp_opaque and nothing reads one back, lib/hnsw.ml:348, lib/ohnsw.ml:312).  Little-endian
 * header + vectors + layer 0 + upper layers; hnsw_index_load re-validates everything through
 * hnsw_index_create.  Format 2 (this version writes it; format 1 files still load) appends what the handle had learnt:
 * the locality codes, if built (n int32), and for every prepared / measured kernel shape whether it took the bitmap blocks --
 * hnsw_index_load adopts the codes (a permutation check: a corrupt table is dropped and rebuilt on demand) and the decisions
 * instead of building and measuring again, and prepares the saved shapes, so the first search after a load runs at the
 * steady-state rate.  Option "half_rows" is not saved (the format is unchanged): a loaded index starts without half rows. */
int32_t hnsw_index_save(const hnsw_index *idx, const char *path);
int32_t hnsw_index_load(const char *path, int32_t device, hnsw_index **out);

/* ---- sharded index: one data set PARTITIONED over several GPUs ------------------------------------------------------------------
 * hnsw_multi replicates the index and splits the query batch: throughput, at G times the memory.  An hnsw_sharded splits the ROWS:
 * each listed device holds a slice of the table with a graph of its own, every query visits all slices, and the per-slice answers
 * are merged.  That is capacity: 100 M x 768 float32 vectors do not fit one device and do fit eight.
 *
 * THE PARTITION.  n_shards = G is in 1..64 (one lane of the merge kernel's wave per shard); outside that range every constructor
 *   returns HNSW_ERR_BAD_ARG, and so does hnsw_sharded_build for n < n_shards.  A device may be listed more than once (the test
 *   arrangement, and legitimate on one large GPU).  Shard g of G holds the rows [lo_g, lo_{g+1}), for hnsw_sharded_build with
 *   lo_g = floor(n * g / G).  A local node v of shard g (0-based) has the GLOBAL id lo_g + v + id_base.  Global ids are int64: a
 *   sharded table may hold more than 2^31 rows even though no single shard may.  hnsw_sharded_shard gives shard g's handle and
 *   first_row = lo_g; hnsw_sharded_get_info gives n = lo_G, the shards' common d, metric and id_base, and the sum of their
 *   device_bytes (each pointer may be NULL).
 * hnsw_sharded_build.  Shard g is exactly hnsw_build(vectors + lo_g * row_stride, lo_{g+1} - lo_g, d, row_stride, params', devices[g])
 *   where params' is *params with seed = params->seed + g: a shard's graph can be checked link for link against that public call.
 *   The shards are built one after another, on the calling thread.  On any error every shard built so far is destroyed and *out is NULL.
 * hnsw_sharded_create adopts G graphs built elsewhere (one OCaml build per slice): descs[g] describes shard g with LOCAL ids, as
 *   hnsw_index_create takes it.  All shards must agree on d, metric and id_base (HNSW_ERR_BAD_ARG otherwise); lo_g is the running sum
 *   of the shards' n, so here the shards need not be equal in size; hnsw_sharded_get_info and hnsw_sharded_shard report the real
 *   bounds.
 * SAVING AND LOADING.  hnsw_sharded_load runs hnsw_index_load(paths[g], devices[g]) per shard and applies the same agreement rules.
 *   Saving needs no call of its own: hnsw_index_save on each borrowed shard handle writes the files hnsw_sharded_load reads.
 * SHARD HANDLES.  A shard handle is an ordinary hnsw_index, borrowed (destroyed with the hnsw_sharded).  The read-only calls work on
 *   it: searches, filters, range calls, stats, exports, hnsw_index_save.  It is marked as owned, as a replica of an hnsw_multi is:
 *   hnsw_index_insert, hnsw_index_remove and hnsw_index_mark_deleted refuse it (HNSW_ERR_BAD_ARG) -- a shard that grows or shrinks
 *   would move every later shard's first_row.  Sharded insert, remove and marks are NOT BUILT; filters and range calls: see below.
 * hnsw_sharded_set_option applies hnsw_index_set_option(name, value) to every shard, in order.  If shard j refuses, shards 0 .. j-1
 *   are set back to the value they had before and shard j's error is returned.  (What "half_rows" / "sq8_rows" -1 freed is not made
 *   again by that.)
 *
 * THE RESULT of hnsw_sharded_search_batch, in terms of public calls only.  Let R_g(q) be the row hnsw_search_batch returns for q on
 *   shard g's handle with the same params -- the host form: exact, tie-overflow repair included, under half or sq8 rows with the
 *   refine rules of that handle.  The real entries of the R_g (id >= id_base) get their global ids, and the answer is the first k of
 *   their union under the total order (distance, global id), where the distance is the returned float32 value compared as IEEE <.
 *   (No entry point returns -0 or, on data without NaN, a NaN for a real id.)  out_ids [nq][k] are int64; rows past the real entries
 *   are filled per params->fill: id -1, and NaN (HNSW_FILL_OHNSW) or +inf (HNSW_FILL_BA).  out_ndist / out_nhops (optional, [nq]) are
 *   the sums over the shards.  k > ef, ef > 1024, null pointers, strides and nq == 0 behave as in hnsw_search_batch.
 *   HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG: "the k farthest of W" has no merged meaning.  A shard whose graph is empty is
 *   HNSW_ERR_EMPTY_INDEX.  DETERMINISM: a query's row depends on its own vector and the params only.
 * hnsw_sharded_brute_force_batch is the same merge over hnsw_brute_force_batch(shard g, k): the exact k nearest of ALL rows.  Each
 *   pair's distance is computed by the same lanes in the same order wherever the row lives, so the returned distances are bit for bit
 *   those of hnsw_brute_force_batch over one index holding all rows.  The ids are bit for bit the same too, with one
 *   ROUNDING EXCEPTION: the unsharded scan orders by its pre-square-root key, two different keys can round to one float distance,
 *   and among such entries the merge orders by id where the unsharded scan orders by key.  It cannot occur on data whose squared
 *   sums are integers below 2^16.  k in 1..1024 (k < 1, unknown fill: HNSW_ERR_BAD_ARG; k > 1024: HNSW_ERR_UNSUPPORTED); k larger than a
 *   shard fills inside that shard's list only.
 * DATA MOVEMENT.  Every device searches the full batch on a stream of its own, concurrently; each shard's [nq][k] ids, distances and
 *   counters go to devices[0] by peer copies ordered behind the shard's search; after one host round trip (a shard whose launch
 *   flagged a tie overflow is repaired and sent again) the merge kernel runs on devices[0] and the merged rows are downloaded once.
 *   One code path whether or not the devices are distinct.  Scratch belongs to the hnsw_sharded, is sized on demand and not counted
 *   in device_bytes: ONE call in flight per handle.
 *
 * hnsw_merge_lists is the merge as an operator of its own (in the spirit of hnsw_rerank_batch; it needs no index): host arrays
 *   ids and dist, each [n_lists][nq][k_in]; each list ascending under (distance, id) with its padding (id < id_base) at the end;
 *   first_row [n_lists], non-decreasing.  out_ids [nq][k_out] (int64) = first_row[list] + id of the first k_out real entries of the
 *   union under (distance, global id); out_dist their distances, the bits given.  Fewer real entries than k_out: the rest is filled
 *   (id -1, NaN or +inf).  n_lists in 1..64, k_in in 1..1024, k_out in 1..1024; a value outside these ranges, an unknown fill or a
 *   decreasing first_row is HNSW_ERR_BAD_ARG; nq == 0 is a no-op.  It runs on `device`.  Both sharded calls above go through its kernel. */
typedef struct hnsw_sharded hnsw_sharded;
int32_t hnsw_sharded_build(const float *vectors, int64_t n, int32_t d, int64_t row_stride, const hnsw_build_params *params,
                           const int32_t *devices, int32_t n_shards, hnsw_sharded **out);
int32_t hnsw_sharded_create(const hnsw_index_desc *const *descs, const int32_t *devices, int32_t n_shards, hnsw_sharded **out);
int32_t hnsw_sharded_load(const char *const *paths, const int32_t *devices, int32_t n_shards, hnsw_sharded **out);
int32_t hnsw_sharded_destroy(hnsw_sharded *s);   /* NULL is HNSW_OK */
int32_t hnsw_sharded_num_shards(const hnsw_sharded *s, int32_t *n_shards);
/* shard g (borrowed: destroyed with the hnsw_sharded) and the global row its local node 0 is; first_row may be NULL */
int32_t hnsw_sharded_shard(hnsw_sharded *s, int32_t g, hnsw_index **out, int64_t *first_row);
int32_t hnsw_sharded_get_info(const hnsw_sharded *s, int64_t *n, int32_t *d, int32_t *metric, int32_t *id_base, int64_t *device_bytes);
int32_t hnsw_sharded_set_option(hnsw_sharded *s, const char *name, int64_t value);
int32_t hnsw_sharded_search_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                                  int64_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops);
int32_t hnsw_sharded_brute_force_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                       int64_t *out_ids, float *out_dist);
int32_t hnsw_merge_lists(int32_t device, const int32_t *ids, const float *dist, const int64_t *first_row, int32_t n_lists,
                         int64_t nq, int32_t k_in, int32_t k_out, int32_t id_base, int32_t fill, int64_t *out_ids, float *out_dist);

/* ---- sharded index: a filter over the global rows, filtered search, range search ---------------------------------------------------
 * The query calls a single index has under an allow-mask or a radius, for an hnsw_sharded.  Every definition is in terms of the
 * public single-index calls on the borrowed shard handles.  Still NOT BUILT for a sharded index: insert, remove and marks (they
 * change the partition), and -- NOT part of this section -- filters from labels (hnsw_filter_create_by_label) and one filter per
 * query (hnsw_search_batch_filtered_each); those two work on a shard handle, one shard at a time.
 *
 * hnsw_sharded_filter_create.  bits is laid out as for hnsw_filter_create, over GLOBAL rows: bit v & 31 of word v >> 5 allows global
 *   row v (0-based, whatever id_base is); n_bits must be the sharded index's n = lo_G (else HNSW_ERR_BAD_ARG).  Shard g's part is
 *   hnsw_filter_create(shard g, B_g, n_g), where B_g is the bits [lo_g, lo_{g+1}) moved down so that global row lo_g is bit 0 (sliced
 *   on the host, n / 8 bytes, once; the tail of B_g's last word is clear).  The object owns G ordinary filters;
 *   hnsw_sharded_filter_part lends part g (for hnsw_filter_bits / hnsw_filter_count; destroyed with the sharded filter);
 *   hnsw_sharded_filter_count is the sum of the parts' counts.  All or nothing: on any error *out is NULL and nothing stays
 *   allocated.  Shard handles cannot grow, shrink or be marked, so a sharded filter never goes stale; destroy it before its
 *   hnsw_sharded.  The calls below refuse a filter made for another hnsw_sharded (HNSW_ERR_BAD_ARG).
 *
 * hnsw_sharded_search_batch_filtered.  Let R_g(q) be the row hnsw_search_batch_filtered(shard g, f's part g, ... the same params ...)
 *   returns for q.  The answer is the first k real entries of the union of the R_g under (distance, global id), then the fill:
 *   exactly what hnsw_sharded_search_batch says about the unfiltered rows.  out_ndist / out_nhops (optional) are the sums over the
 *   shards; out_stage[q] (optional) is the maximum over the shards as unsigned 32-bit numbers, so it is 0xFFFFFFFF as soon as one
 *   shard answered q from its exact stage.  A shard whose part allows fewer than k nodes, or none, behaves as the single-index
 *   definition says (exact stage, the fill inside its list); the merge then fills only what all shards together could not supply.
 *   Errors (the outputs stay untouched): those of hnsw_sharded_search_batch; a null or foreign filter is HNSW_ERR_BAD_ARG;
 *   HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG; an empty shard graph is HNSW_ERR_EMPTY_INDEX.
 *
 * hnsw_sharded_range_search_batch / hnsw_sharded_range_brute_force_batch.  Let S_g(q) be the segment q gets on shard g from
 *   hnsw_range_search_batch (f NULL) or hnsw_range_search_batch_filtered with f's part g; for the exact form from
 *   hnsw_range_brute_force_batch or hnsw_range_brute_force_batch_filtered.  Query q's merged segment is the union of the S_g(q) with
 *   global ids (first_row[g] + id: int64), ascending under (distance, global id), the distance being the returned float compared
 *   as IEEE <.  (A single-index segment is ordered by the scan's pre-rounding key: where two keys round to one float distance, two
 *   entries of ONE shard can stand with the higher id first.  The merged segment is in (distance, global id) order there too: the
 *   merge puts such entries right, so even with one shard it can differ from the shard's own segment in the order of such pairs.)
 *   lims[q] = the sum over g of lims_g[q] (each shard's lims is a prefix sum, so the sum is one).  Counters: ndist and
 *   nhops are summed, stage is the unsigned maximum over the shards.  For the exact form the in-range test is on distance bits that do
 *   not depend on where a row lives: the merged SET is exactly that of hnsw_range_brute_force_batch over one index holding all
 *   rows, and the order too, with the ROUNDING EXCEPTION of hnsw_sharded_brute_force_batch.  Errors: as the single-index calls (a
 *   NaN radius, ef, semantics; HNSW_ERR_EMPTY_INDEX for the graph form only; nq == 0 gives a valid empty result), reported for the
 *   lowest-numbered failing shard; a foreign filter is HNSW_ERR_BAD_ARG; a merged total above 2^31 - 1 is HNSW_ERR_UNSUPPORTED,
 *   found from the shards' totals before the merged buffers are allocated.  An error leaves *out NULL and the shard results
 *   destroyed.  An hnsw_sharded_range_result owns its buffers on devices[0] and holds no reference to the hnsw_sharded: it
 *   outlives it; any number may be alive; _size, _fetch (every pointer optional), _device and _destroy (NULL is HNSW_OK) are those
 *   of hnsw_range_result with int64 ids.
 *
 * DATA MOVEMENT.  The single-index filtered and range calls are host-driven ladders, complete on return, so they are not queued on
 *   G streams: the G shard calls run on one host thread per shard (each sets its shard's device; at most 16 at a time; all joined
 *   before anything else happens; the error message of the lowest-numbered failing shard is carried to the caller's thread).
 *   Filtered k-NN: the shards' rows and counters are staged into the [G][nq][k] and [G][nq] tables on devices[0], then the merge
 *   kernel of hnsw_merge_lists, then one download.  Range: every shard result stays on its device; its lims, ids, distances and
 *   counters go to devices[0] by peer copies, one concatenated table per kind; then the segment merge and the counter reduce; the
 *   shard results are destroyed before return.  ONE call in flight per hnsw_sharded, as for the calls above.
 *
 * hnsw_merge_segments is the segment merge as an operator of its own (it needs no index): host arrays lims[g] ([nq + 1], starting
 *   at 0, non-decreasing), ids[g] and dist[g] ([lims[g][nq]]) for n_lists in 1..64 lists; each segment ascending under (distance,
 *   id) with no padding entries (id_base is accepted for symmetry with hnsw_merge_lists and has no effect); first_row [n_lists],
 *   non-decreasing.  The result is the merge defined above; the same global id in two lists: the lower list comes first; its
 *   counters read as 0.  n_lists outside 1..64, a decreasing first_row, a lims that does not start at 0 or decreases, a null
 *   array: HNSW_ERR_BAD_ARG, found on the host before a device is touched; more than 2^31 - 1 entries: HNSW_ERR_UNSUPPORTED.  That the
 *   segments are sorted is not checked: entries of equal distance may stand in any id order (they are put right), distances out of
 *   order give some permutation of each query's entries.  It runs on `device`. */
typedef struct hnsw_sharded_filter hnsw_sharded_filter;
typedef struct hnsw_sharded_range_result hnsw_sharded_range_result;   /* owns its buffers on devices[0]; int64 global ids */
int32_t hnsw_sharded_filter_create(hnsw_sharded *s, const uint32_t *bits, int64_t n_bits, hnsw_sharded_filter **out);
int32_t hnsw_sharded_filter_destroy(hnsw_sharded_filter *f);          /* NULL is HNSW_OK */
int32_t hnsw_sharded_filter_count(const hnsw_sharded_filter *f, int64_t *n_allowed);
int32_t hnsw_sharded_filter_part(const hnsw_sharded_filter *f, int32_t g, const hnsw_filter **out);   /* borrowed */
int32_t hnsw_sharded_search_batch_filtered(hnsw_sharded *s, const hnsw_sharded_filter *f, const float *queries, int64_t nq,
                                           int64_t q_stride, const hnsw_search_params *params, int64_t *out_ids, float *out_dist,
                                           uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);
int32_t hnsw_sharded_range_search_batch(hnsw_sharded *s, const hnsw_sharded_filter *f /* may be NULL */, const float *queries,
                                        int64_t nq, int64_t q_stride, const hnsw_range_params *params, hnsw_sharded_range_result **out);
int32_t hnsw_sharded_range_brute_force_batch(hnsw_sharded *s, const hnsw_sharded_filter *f /* may be NULL */, const float *queries,
                                             int64_t nq, int64_t q_stride, float radius, hnsw_sharded_range_result **out);
int32_t hnsw_sharded_range_result_size(const hnsw_sharded_range_result *r, int64_t *nq, int64_t *total);
int32_t hnsw_sharded_range_result_fetch(hnsw_sharded_range_result *r, int64_t *lims, int64_t *ids, float *dist, uint32_t *out_ndist,
                                        uint32_t *out_nhops, uint32_t *out_stage);
int32_t hnsw_sharded_range_result_device(hnsw_sharded_range_result *r, const int64_t **d_lims, const int64_t **d_ids, const float **d_dist);
int32_t hnsw_sharded_range_result_destroy(hnsw_sharded_range_result *r);
int32_t hnsw_merge_segments(int32_t device, int32_t n_lists, int64_t nq, const int64_t *const *lims, const int32_t *const *ids,
                            const float *const *dist, const int64_t *first_row, int32_t id_base, hnsw_sharded_range_result **out);

/* ---- grouped search: the k nearest GROUPS, one node per label ("group by", "collapse": chunked documents, tenants, products) ----
 * THE LABELS.  hnsw_labels_create uploads one label per node (labels: a host array of n values, not retained).  n must be the
 * index's current n, n_labels >= 1, each label in -1 .. n_labels - 1, where -1 means the node is in no group; any other value is
 * HNSW_ERR_BAD_ARG, found on the host before anything is allocated, and *out is NULL.  A node marked deleted
 * (hnsw_index_mark_deleted) gets -1 in the device copy; hnsw_labels_get copies the n labels as the device holds them back to the
 * host.  The object belongs to the handle and its graph epoch: after hnsw_index_insert, hnsw_index_remove,
 * hnsw_index_mark_deleted or hnsw_index_unmark_deleted it is stale and every call that takes it answers HNSW_ERR_BAD_ARG, as for a
 * filter.  hnsw_labels_info reports n_labels, n_labelled (the nodes with a label >= 0) and n_groups (the labels at least one node
 * carries), both counted on the device at creation; each pointer may be NULL.  Cost: 4 * n bytes on the device, NOT counted in
 * hnsw_index_info.device_bytes.  Not saved with the index.  Any number of label objects per index; hnsw_labels_destroy(NULL) is HNSW_OK.
 *
 * THE RESULT of hnsw_search_batch_grouped, in terms of public calls only.  A node is ELIGIBLE when its label is >= 0 and, with a
 * filter (f may be NULL), it is allowed.  For an ordered list S of node ids let G(S) be the subsequence that keeps the first
 * eligible member of each label.  W_e(q) is as the filtered section defines it: the ids hnsw_search_batch returns for (ef = e,
 * k = e) with the caller's semantics, the host form.
 *   1. LADDER.  e_0 = ef, e_{j+1} = min(1024, 2 * e_j).  A query is served at the first stage j with |G(W_{e_j}(q))| >= k; its
 *      answer is the first k members of G(W_{e_j}(q)).  Only the queries still short are searched again at the next stage, as one
 *      compacted batch.  The walk itself is never filtered or grouped: it is the walk every other entry point runs.
 *   2. EXACT STAGE.  A query still short at e = 1024, and EVERY query, with no walk made, when n_groups < k or f->n_allowed < k,
 *      gets what hnsw_brute_force_batch_grouped returns: for each label the eligible node smallest under the scan's order -- the
 *      ordered pre-square-root key, then the node id, over the float32 rows -- and of those the k smallest, ascending.  With fewer
 *      than k groups the first entries are real and the rest filled per params->fill: id -1, label -1, distance NaN
 *      (HNSW_FILL_OHNSW) or +inf (HNSW_FILL_BA).
 *   3. DISTANCES ARE ALWAYS OVER THE FLOAT32 ROWS: the bits of hnsw_distance_batch for the returned ids.
 *        - byte, split and float32 rows: the walk's distances are those bits already.
 *        - HNSW_ROWS_HALF, HNSW_ROWS_SQ8 and HNSW_ROWS_SQ8_DIM: ALL eligible members of W_e(q) are first re-ranked over the float32
 *          rows by hnsw_rerank_batch's kernel (the ineligible members as padding, k := e), at every stage the query walks, and G is
 *          taken over that re-ranked list.  The stage test is unchanged: it does not depend on the order.
 *   4. OUTPUTS.  out_ids [nq][k] (id_base-based), out_dist [nq][k], ascending, out_labels [nq][k].  out_stage (optional, [nq]): j
 *      for a query served at ladder stage j, 0xFFFFFFFF for the exact stage.  out_nhops (optional): the sum of the hops of the walks
 *      taken (0 without a walk).  out_ndist (optional): the walks' evaluations, plus the members re-ranked (half / sq8 rows: the
 *      eligible members of W at each stage walked), plus n_labelled for the exact stage -- with a filter that last term is
 *      f->n_allowed.
 *   5. ERRORS are those of hnsw_search_batch_filtered.  k > ef: HNSW_ERR_BAD_ARG; ef > 1024: HNSW_ERR_UNSUPPORTED;
 *      HNSW_SEM_FUNCTOR_NEAREST_K: HNSW_ERR_BAD_ARG; an empty index: HNSW_ERR_EMPTY_INDEX; null, foreign or stale labels, a
 *      foreign or stale filter: HNSW_ERR_BAD_ARG; null pointers, q_stride and nq as hnsw_search_batch; nq == 0 is a no-op.  An error
 *      leaves the outputs untouched.  Matrices of hnsw_host_alloc / hnsw_host_register are read and written in place, others are
 *      copied; complete on return.
 *   6. DETERMINISM.  A row depends on the query's own vector, the labels, the mask and (ef, k, semantics) only: not on the batch
 *      it is in, and not on which stage other queries reached.
 * ONE filtered, range or grouped call in flight per handle: they share the ladder's and the filtered search's scratch.  There is
 * no device-pointer form.
 *
 * hnsw_brute_force_batch_grouped is the exact form: the rows point 2 describes, for every query.  k in 1..1024: k < 1 or a bad
 * fill is HNSW_ERR_BAD_ARG, k > 1024 HNSW_ERR_UNSUPPORTED.  It needs no graph, always scans the float32 rows, and its result does
 * not depend on option "scan_slabs" or on the batch.  Scratch: one 64-bit cell per (query, label), 8 * n_labels bytes per query of
 * a piece of the batch (pieces of at most 256 MiB, never below one tile of the scan); it belongs to the handle and is not counted
 * in device_bytes; if it cannot be allocated the call answers HNSW_ERR_OOM with the outputs untouched.
 *
 * NOT BUILT: more than one member per group (group_size > 1); one label object per query; hnsw_sharded_* grouped forms (a borrowed
 * shard or replica handle is served like any handle); option "filter_collect" for this call (the option is ignored here).
 * Rates (tools/group_rate.py, profiles/grouped.txt; one run), MI355X, 1 M x 128 byte rows, ef 128, k 10, 10 k queries: all-distinct
 * labels 1.81 ms per batch, random groups of 10 nodes 1.79 ms, against 0.86 ms for hnsw_search_batch and 6.3 - 6.6 ms for
 * hnsw_search_batch_filtered under an all-ones mask on the same handle; 256 far-apart clusters as labels: 336 ms, every query ends
 * in the exact stage; the exact stage alone: 0.028 / 0.042 / 0.068 ms per query for 10^3 / 10^5 / 10^6 labels (64 queries). */
typedef struct hnsw_labels hnsw_labels;
int32_t hnsw_labels_create(hnsw_index *idx, const int32_t *labels, int64_t n, int32_t n_labels, hnsw_labels **out);
int32_t hnsw_labels_destroy(hnsw_labels *l);                       /* NULL is HNSW_OK */
int32_t hnsw_labels_info(const hnsw_labels *l, int32_t *n_labels, int64_t *n_labelled, int64_t *n_groups);  /* each may be NULL */
int32_t hnsw_labels_get(const hnsw_labels *l, int32_t *out);       /* the n labels as the device holds them */
int32_t hnsw_search_batch_grouped(hnsw_index *idx, const hnsw_labels *labels, const hnsw_filter *f /* may be NULL */,
                                  const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                                  int32_t *out_ids, float *out_dist, int32_t *out_labels,
                                  uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);
int32_t hnsw_brute_force_batch_grouped(hnsw_index *idx, const hnsw_labels *labels, const hnsw_filter *f /* may be NULL */,
                                       const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                       int32_t *out_ids, float *out_dist, int32_t *out_labels);

/* ---- keys: stable 64-bit names the index owns -- search, find and mutate by key ----
 * hnsw_index_remove and hnsw_index_compact renumber every surviving node, so a row number is no name to keep.  An index may own one
 * KEY per stored node: a caller-chosen int64_t, every value legal (INT64_MIN, -1, 0 and INT64_MAX included), pairwise distinct
 * within the index.  The index keeps the keys on the device in row order (key_of, 8 n bytes) beside a lookup table of the n pairs
 * (key, node) ordered by key as SIGNED 64-bit numbers (12 n bytes), rebuilt from key_of whenever that changes, and moves the keys
 * with their nodes through insert, remove and compact.  Everything here is opt-in: a handle never given keys behaves bit for bit as
 * before, and no other entry point changes its result on such a handle.  The tables belong to the handle as the live mask does:
 * NOT counted in hnsw_index_info.device_bytes; hnsw_index_keys_info reports has_keys (0 / 1) and their bytes (each pointer may be
 * NULL).  Every call below but set / clear / info / insert_keyed answers HNSW_ERR_BAD_ARG on a handle without keys.
 *
 * hnsw_index_set_keys(idx, keys, n): n must be the index's n; NULL keys with n > 0 are refused.  The keys must be pairwise distinct,
 *   otherwise HNSW_ERR_BAD_ARG and the message names the smallest duplicated key (a min-reduction on the device, not the first to
 *   arrive).  All or nothing: on any error, HNSW_ERR_OOM included, the handle keeps the keys it had, or none.  A second call
 *   replaces all keys.  It does not move the graph epoch: filters and labels stay valid.  A replica of an hnsw_multi or a shard of
 *   an hnsw_sharded is refused, as hnsw_index_insert refuses them.
 * hnsw_index_clear_keys: afterwards the handle is one that never had keys.
 * hnsw_index_keys_of(idx, ids, m, missing_key, out): out[i] = the key of node ids[i] (id_base-based); any id outside
 *   [id_base, id_base + n) gives missing_key -- that includes the searches' fill id -1.  A node marked deleted still has its key:
 *   the ids are explicit.  ids == NULL: all n rows in order, m must be n.  This is the operator that makes every other search form
 *   usable with keys: range results, grouped rows, the per-query-filter call, the layer operators.  hnsw_index_keys_of_device is
 *   the same over device arrays, queued on `stream` (d_ids and d_out must not be NULL when m > 0).
 * hnsw_index_find_keys(idx, keys, m, out_ids): out_ids[i] = the id_base-based id of the node whose key is keys[i], or id_base - 1
 *   if there is none (a binary search per key on the device).  Repeated keys in the call are fine; m == 0 is a no-op.
 * hnsw_search_batch_keyed: with f NULL the rows are those of hnsw_search_batch (marks honoured as there), otherwise those of
 *   hnsw_search_batch_filtered(f); both passed through hnsw_index_keys_of with missing_key: out_keys [nq][k].  Distances and
 *   counters are bit-identical to those calls', errors are theirs.  out_stage is optional: as the filtered call writes it, and zero
 *   for the plain path of an unmarked handle.  It costs one translate launch over the device-resident ids and the download of
 *   8-byte instead of 4-byte rows, not a second pass over host memory.
 * hnsw_index_insert_keyed(idx, vectors, m, row_stride, keys, params): hnsw_index_insert of the vectors -- the graph is link for
 *   link what the plain call builds on a twin without keys -- with the m keys appended to key_of.  Refused before anything is
 *   built, the index and its keys untouched: a key equal to a stored key, or two equal keys in the call (HNSW_ERR_BAD_ARG, the key
 *   named); an index without keys that has n > 0 (hnsw_index_set_keys first).  An EMPTY index without keys starts its keys with this
 *   call.  Plain hnsw_index_insert on a handle with keys is refused (HNSW_ERR_BAD_ARG, pointing at the keyed call): an index with
 *   keys must never hold a node without one.
 * hnsw_index_remove, hnsw_index_compact on a handle with keys: the keys move with their nodes under out_new_id's numbering
 *   (new_key_of[new_id[v]] = key_of[v], on the device), inside the all-or-nothing swap.  Removing every node leaves an empty index
 *   that still has keys (none).
 * hnsw_index_remove_keys(idx, keys, m, out_new_id) is hnsw_index_remove(find(keys)); hnsw_index_mark_deleted_keys and
 *   hnsw_index_unmark_deleted_keys are hnsw_index_mark_deleted(find(keys)) and hnsw_index_unmark_deleted(find(keys)).  An absent
 *   key is HNSW_ERR_BAD_ARG with the key named (the first by position), and nothing is changed.  Duplicates: remove's and mark's rule.
 * hnsw_filter_create_by_keys(idx, keys, m, out): an ordinary filter that allows exactly the named nodes, ANDed with the live mask
 *   as hnsw_filter_create's is.  An absent key is refused, naming the first by position; a repeated key is fine; on error *out is NULL.
 * hnsw_index_save stays accepted and the format does not change: keys are NOT saved.  hnsw_index_keys_of(NULL ids) before the
 *   save and hnsw_index_set_keys on the loaded handle is the round trip.
 *
 * NOT BUILT: keys for hnsw_sharded and hnsw_multi; saved keys; keyed forms of the range,
 * grouped and per-query-filter calls -- compose those with hnsw_index_keys_of.  (upsert, replacing the vector under a key: built,
 * see hnsw_index_upsert_keyed in the header's last section.)
 * Rates (tools/keys_rate.py, profiles/keys.txt; one run), MI355X, 1 M x 128 byte rows, ef 128, k 10, 10 k queries, the two calls
 * alternating on one handle: hnsw_search_batch_keyed 0.894 ms per batch against 0.849 ms for hnsw_search_batch (+0.045 ms: the
 * launch and 800 KB of keys downloaded where the plain call downloads 400 KB of ids); hnsw_index_set_keys of 1 M keys 1.75 ms;
 * hnsw_index_find_keys 0.05 ms for 10 k keys and 0.99 ms for 1 M; hnsw_index_remove_keys of 1000 keys 53 ms against 75 ms for
 * hnsw_index_remove of the same nodes on a twin (one run each). */
int32_t hnsw_index_set_keys(hnsw_index *idx, const int64_t *keys, int64_t n);
int32_t hnsw_index_clear_keys(hnsw_index *idx);
int32_t hnsw_index_keys_info(const hnsw_index *idx, int32_t *has_keys, int64_t *bytes);
int32_t hnsw_index_keys_of(const hnsw_index *idx, const int32_t *ids, int64_t m, int64_t missing_key, int64_t *out);
int32_t hnsw_index_keys_of_device(hnsw_index *idx, const int32_t *d_ids, int64_t m, int64_t missing_key, int64_t *d_out, void *stream);
int32_t hnsw_index_find_keys(const hnsw_index *idx, const int64_t *keys, int64_t m, int64_t *out_ids);
int32_t hnsw_search_batch_keyed(hnsw_index *idx, const hnsw_filter *f /* may be NULL */, const float *queries, int64_t nq,
                                int64_t q_stride, const hnsw_search_params *params, int64_t missing_key, int64_t *out_keys,
                                float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage);
int32_t hnsw_index_insert_keyed(hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const int64_t *keys,
                                const hnsw_build_params *params);
int32_t hnsw_index_remove_keys(hnsw_index *idx, const int64_t *keys, int64_t m, int32_t *out_new_id);
int32_t hnsw_index_mark_deleted_keys(hnsw_index *idx, const int64_t *keys, int64_t m);
int32_t hnsw_index_unmark_deleted_keys(hnsw_index *idx, const int64_t *keys, int64_t m);
int32_t hnsw_filter_create_by_keys(hnsw_index *idx, const int64_t *keys, int64_t m, hnsw_filter **out);

/* ---- search by stored item: neighbours of nodes named by id or by key, the k-NN graph of the whole index ----
 * "What is near THIS stored item": the queries of a call are rows the index already holds, so only their ids cross the link -- the
 * rows are gathered on the device out of the float32 table, which is resident whatever row_format is.
 *
 * THE DEFINITION is one equivalence.  Let Q = hnsw_index_get_rows(ids): the stored float32 rows (for HNSW_METRIC_COSINE that is N(X)).
 *   exclude_self = 0: the call answers bit for bit what hnsw_search_batch(idx, Q, params) answers on the same handle in the same
 *     state: ids, distances and both counters.
 *   exclude_self = 1: let P = {ef' = max(ef, k + 1), k' = k + 1, fill, semantics} and R = hnsw_search_batch(idx, Q, P).  For query q
 *     let p be the smallest j in [0, k] with R.ids[q][j] == ids[q], or k if there is none.  The output row is R's row with
 *     position p deleted: k entries.  If self is absent from the first k + 1, the row is the first k of them.  Trailing fill
 *     entries stay fill: removal shifts them left unchanged.  The counters are R's.
 * Everything the host call does is therefore inherited, not restated: the row formats (byte, split, half, sq8, sq8_dim, bits,
 * bit_query_bits) with their query transforms and re-rank; option "refine"; COSINE's normalisation of the call's queries (so
 * N(N(x)), as for any caller); the live mask of a marked handle with the filtered ladder and the exact stage -- a node marked
 * deleted is a legal QUERY, its row is there, and it can never be in its own row --; the ordering pre-pass, the tie-overflow repair
 * and option "visited_blocks".  A query's row depends on its own id only, not on the batch it is in.
 *
 * hnsw_index_get_rows_device(idx, d_ids, m, d_out, out_stride, stream): the bits of hnsw_index_get_rows over device arrays, queued on
 *   `stream`: d_ids [m] int32, id_base-based; row j of d_out (out_stride floats apart, d written) is the row of node d_ids[j].  An id
 *   outside the index gives a row of d zeros: the device cannot refuse.  m == 0 is a no-op; NULL arrays with m > 0, or
 *   out_stride < d, are HNSW_ERR_BAD_ARG.  It uses no scratch of the handle.  With it and hnsw_search_batch_device a
 *   device-resident caller composes its own search by id.
 * hnsw_search_batch_by_id(idx, ids, nq, params, exclude_self, out_ids, out_dist, out_ndist, out_nhops): the definition above.  ids
 *   [nq] are int32 and id_base-based, so the output of a search can be fed straight back; repeated ids are fine.  An id out of range
 *   is HNSW_ERR_BAD_ARG naming the first by position, and nothing is written.  exclude_self other than 0 / 1 is HNSW_ERR_BAD_ARG;
 *   exclude_self = 1 with HNSW_SEM_FUNCTOR_NEAREST_K is HNSW_ERR_BAD_ARG (the k farthest of a W one wider have no meaning);
 *   k + 1 > 1024 is HNSW_ERR_UNSUPPORTED.  Every other check and error is hnsw_search_batch's, on P.  nq == 0 is a no-op.
 *   out_ids / out_dist [nq][k]; matrices of hnsw_host_alloc / hnsw_host_register are written in place, others downloaded;
 *   out_ndist / out_nhops are optional.  Complete on return.
 * hnsw_search_batch_by_key(idx, keys, nq, params, exclude_self, missing_key, out_keys, ...): by_id(find_keys(keys)) with the rows
 *   returned as keys (hnsw_index_keys_of's rule with missing_key, applied in the same pass that removes self).  An absent key is
 *   HNSW_ERR_BAD_ARG naming the first by position, and nothing is written: hnsw_index_remove_keys' rule.  A handle without keys is
 *   HNSW_ERR_BAD_ARG.  Distances and counters are bit for bit those of the by-id call.
 * hnsw_brute_force_batch_by_id(idx, ids, nq, k, fill, exclude_self, out_ids, out_dist): the same two definitions over
 *   hnsw_brute_force_batch: k + 1 <= 1024, marks honoured as there.  Under L2 it is the exact answer without self: the nodes ahead
 *   of self under (distance, id) are its lower-numbered duplicates; if more than k of them exist, self is past position k and the
 *   first k are right.
 * hnsw_knn_graph(idx, params, exact, out_ids, out_dist): the k-NN graph of the whole index.  Row v of out_ids / out_dist ([n][k];
 *   out_dist may be NULL) is the row of hnsw_search_batch_by_id for ids[v] = id_base + v with exclude_self = 1 -- with exact = 1
 *   the row of hnsw_brute_force_batch_by_id instead --, bit for bit that one call.  It is computed inside the library in chunks of
 *   option "graph_chunk_rows" nodes (hnsw_index_set_option; default 65536, values < 1 refused), so the handle's scratch stays a
 *   chunk's whatever n is; the option changes no result.  n == 0 is HNSW_OK.
 * A replica of an hnsw_multi (hnsw_multi_replica) is accepted read-only, as the scan accepts it.  After hnsw_index_insert,
 * hnsw_index_remove or hnsw_index_compact the calls see the table as it then is.  One such call in flight per handle: they share
 * the host calls' scratch.
 *
 * NOT BUILT: a device-pointer form of the search by id (compose hnsw_index_get_rows_device and hnsw_search_batch_device);
 * hnsw_sharded_* forms; range search by id; starting the layer-0 walk at the node itself instead of descending (the knn kernels
 * take a pre-computed entry already, but the ladder, the repair path and the re-rank would all have to carry it along: a follow-up
 * with a definition of its own, through hnsw_search_layer_batch); overlap of one chunk's download with the next chunk's search in
 * hnsw_knn_graph.
 * Rates (tools/by_id_rate.py, profiles/by_id.txt; one run), MI355X, 1 M x 128 byte rows, ef 128, k 10, 10 k stored nodes as the
 * queries, the calls alternating on one handle: hnsw_search_batch_by_id 0.778 ms per batch (exclude_self 1: 0.781) against 0.849 ms
 * for hnsw_search_batch over the same rows from a page-locked matrix and 1.551 ms for hnsw_index_get_rows + hnsw_search_batch with
 * k + 1 + the strip on the host; hnsw_knn_graph of all 1 M nodes 56.4 ms. */
int32_t hnsw_index_get_rows_device(hnsw_index *idx, const int32_t *d_ids, int64_t m, float *d_out, int64_t out_stride, void *stream);
int32_t hnsw_search_batch_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, const hnsw_search_params *params,
                                int32_t exclude_self, int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops);
int32_t hnsw_search_batch_by_key(hnsw_index *idx, const int64_t *keys, int64_t nq, const hnsw_search_params *params,
                                 int32_t exclude_self, int64_t missing_key, int64_t *out_keys, float *out_dist,
                                 uint32_t *out_ndist, uint32_t *out_nhops);
int32_t hnsw_brute_force_batch_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, int32_t k, int32_t fill, int32_t exclude_self,
                                     int32_t *out_ids, float *out_dist);
int32_t hnsw_knn_graph(hnsw_index *idx, const hnsw_search_params *params, int32_t exact, int32_t *out_ids /* [n][k] */,
                       float *out_dist /* [n][k] or NULL */);

/* ==== upsert: replace or add vectors in one all-or-nothing call ====
 * "Store this vector under this key, whether the key is there or not."  The index could grow (hnsw_index_insert_keyed) and shrink
 * (hnsw_index_remove_keys); changing the vector under a key took both, two table swaps, and was not atomic: a refused insert left
 * the old vectors gone and the new ones absent.
 *
 * THE DEFINITION is ONE equivalence.  Let P be the call's keys that are stored.  hnsw_index_upsert_keyed(idx, X, keys, m, ...)
 * leaves the handle exactly as this sequence leaves it:
 *   1. hnsw_index_remove_keys(idx, P in the call's order);
 *   2. hnsw_index_insert_keyed(idx, X, m, row_stride, keys, params).
 * "Exactly": link for link on every layer, row for row, level for level, key for key, entry point and max_layer, every derived
 * row copy with its parameters (hnsw_index_sq8_params, hnsw_index_sq8_dim_params, hnsw_index_bit_params), the marks, and every
 * search result bit for bit.  The one difference is the purpose of the call: the graph epoch moves on once, not twice (filters and
 * labels made before are refused afterwards), there is one table swap, one re-derivation of the row copies over the final table
 * (the sq8 kinds quantise the whole table once), one warm-up.
 * Everything else is inherited from the two calls, not restated: the m rows become the nodes n_old - |P| ... n_old - |P| + m - 1
 * (plus id_base) in the call's row order, stored or not; their levels are the draws of those positions under params->seed; the
 * repair rule of hnsw_index_remove; batching, the widening of rows narrower than 2M / M, COSINE's normalisation of the new rows,
 * expected_ef and the prepared shapes of hnsw_index_insert.  A node marked deleted whose key is upserted comes back live (it was
 * removed and inserted); the other marks move with their nodes.  The locality codes are dropped and built again on demand, as the
 * removal leaves them for the insert that follows it; with no stored key in the call they are carried over, as hnsw_index_insert_keyed
 * carries them.
 * hnsw_index_update(idx, ids, X, m, ...) is the same definition over hnsw_index_remove(ids) and hnsw_index_insert(X), for handles
 * without keys: the m stored nodes ids[i] (id_base-based) are replaced by the rows X[i].  A handle with keys is refused
 * (HNSW_ERR_BAD_ARG, pointing at the keyed call), as hnsw_index_insert refuses it.
 *
 * Outputs (both optional, written only when the call succeeds): out_replaced[i] = 1 if keys[i] was stored, else 0; out_new_id
 * [n_old] as hnsw_index_remove writes it: the id a kept node has afterwards, id_base - 1 for a replaced node.
 * Special cases: m == 0 is a no-op that fills out_new_id with the identity (the epoch does not move).  With P empty the call IS
 * hnsw_index_insert_keyed.  With every stored node in P it empties the index and then equals hnsw_build of X with the keys.
 *
 * Refused, all before anything is built, the handle untouched (HNSW_ERR_BAD_ARG unless named): two equal keys in the call, naming
 * the smallest such key as hnsw_index_set_keys does; a handle that has nodes and no keys in the keyed call (an EMPTY index without
 * keys is accepted and starts its keys here, as hnsw_index_insert_keyed accepts it); in hnsw_index_update an id out of range or
 * repeated; and everything hnsw_index_remove and hnsw_index_insert refuse: submitted requests not waited for, a replica of an
 * hnsw_multi, a shard of an hnsw_sharded, params->metric or params->id_base that differ from the index's, rows wider than 2M / M,
 * a NaN or infinite new value while a code option (sq8_rows, sq8_dim_rows, bit_rows) is on (HNSW_ERR_UNSUPPORTED), a
 * device_fallback_slab_bytes slab that holds no query of the final n.  The insert's checks are made against the index the
 * removal WILL leave (its node count and top layer are plain arithmetic).
 * All or nothing, which the two-call sequence is not: on any error at any stage -- HNSW_ERR_OOM, a value out of fp16 range under
 * half_rows, a degree overflow that exhausts its retries included -- the index is exactly as before: same graph, same keys, same
 * marks, same epoch, filters made before still accepted.
 *
 * Device memory: the call holds no more than either call alone, two copies of the index at its peak (the old tables and the new
 * ones).  The removal half builds its repaired graph straight into tables sized for the final node count and upper-row count, and
 * the insert half uploads the new rows behind the kept ones and grows the graph in place on those same tables.  A handle whose
 * rows are narrower than 2M / M (a graph flattened from elsewhere) goes through hnsw_index_insert's widening copy: a third copy for
 * the duration of the call.  A degree overflow of the builder runs the removal again (it is deterministic) before the batches get
 * four times the removal buffer.
 *
 * NOT BUILT: upsert for hnsw_sharded and hnsw_multi; an in-place update that keeps the node's id (the definition renumbers, as the
 * removal does); saved keys.
 * Rates (tools/upsert_rate.py, profiles/upsert.txt; one run), MI355X, 1 M x 128 byte rows, M 16, efC 200, calls of 1000 keys, half
 * stored and half new, against hnsw_index_remove_keys + hnsw_index_insert_keyed on a twin, the two taking turns: 131.1 ms per call
 * against 135.9 ms for the pair (minima 128.7 / 133.1; with sq8_rows on 146.7 / 141.3): the ranges overlap, the call is not
 * measurably faster -- the removal's repair is 126 ms of the pair, the whole insert call 10 ms.  Sampled peak of device memory above
 * the index: 843 MB for both (the index: 798 MB). */
int32_t hnsw_index_upsert_keyed(hnsw_index *idx, const float *vectors, const int64_t *keys, int64_t m, int64_t row_stride,
                                const hnsw_build_params *params, uint8_t *out_replaced /* optional [m] */,
                                int32_t *out_new_id /* optional [n_old] */);
int32_t hnsw_index_update(hnsw_index *idx, const int64_t *ids, const float *vectors, int64_t m, int64_t row_stride,
                          const hnsw_build_params *params, int32_t *out_new_id /* optional [n_old] */);

/* #### paged k-NN search: the NEXT k after a (distance, id) cursor ####
 * "Ten more, please."  hnsw_search_batch answers the k nearest with k <= ef <= 1024; past that it has no answer, and a caller who
 * pages by asking for a larger k throws the head away each time.  These two calls take, per query, a CURSOR -- the (distance, id)
 * of the last result the caller holds -- and return the k results that come after it.
 *
 * 0. ORDER.  D(q, v) is the float hnsw_distance_batch returns for the pair: over the float32 rows whatever row_format says, under
 *    HNSW_METRIC_COSINE over N(X) with N(q).  ord(x) is the monotone map of a float's bits that puts -0 below +0 and a positive NaN
 *    above +inf (the sign bit flipped, a negative value's other bits too).  The PAGED ORDER is (ord(D), node id).  It orders by what
 *    the caller holds: hnsw_brute_force_batch orders by (key, id), and for L2 the key is the squared sum BEFORE the square root,
 *    which maps two to three neighbouring sums onto one float -- a caller never sees keys, so a cursor cannot name one.  The paged
 *    order is a coarsening of that order and differs from it only among nodes whose returned L2 distances are equal while their
 *    squared sums are not; under inner product and cosine the two coincide.
 *    Node v is AFTER cursor c iff ord(D) > ord(c.dist), or they are equal and v + id_base > c.id, the ids compared in 64 bits.  Any
 *    c.id is legal: {r, INT32_MAX} means "strictly beyond distance r", {r, id_base - 1} "from distance r on"; HNSW_CURSOR_START is
 *    before every node.  after == NULL: HNSW_CURSOR_START for every query.  A NaN c.dist is HNSW_ERR_BAD_ARG, found on the host
 *    before any launch.
 * 1. ELIGIBLE: a node that is after the query's cursor, is allowed by f when f is given, and is not marked deleted (the live mask
 *    is ANDed as every filtered call does).
 * 2. hnsw_brute_force_batch_after: row q is the first k eligible nodes under the paged order, the rest filled per `fill` (id -1;
 *    NaN or +inf).  It needs no graph; n = 0 is HNSW_OK with filled rows; the k limits are those of hnsw_brute_force_batch.  The
 *    result never depends on option scan_slabs or on the row format.
 * 3. hnsw_search_batch_after: W_e(q) is as the range section defines it -- hnsw_search_batch at (ef = e, k = e), the host form;
 *    under inexact rows (half rows, codes) all its members re-ranked with k := e.  A_e(q) is the eligible members of W_e(q).
 *    LADDER: e_0 = ef, e_{j+1} = min(1024, 2 e_j); a query is served at the first stage with |A_e| >= k, and its row is the first k
 *    of A_e UNDER THE PAGED ORDER (W ascends in (key, id), so D is non-decreasing along it: only runs of equal D have their ids put
 *    in order).  Only the queries still short are walked again, as one compacted batch in ascending query order.  EXACT STAGE: a
 *    query still short at e = 1024 -- and every query when fewer than k nodes are allowed at all -- gets the row of point 2; its
 *    out_stage is 0xFFFFFFFF.  The walk is never modified.
 * 4. out_next[q] (optional) is (distance, id) of the row's last real entry, the input cursor when the row has none.  A row with
 *    fewer than k real entries always comes from the exact stage, so it means "exhausted".
 * 5. CONSEQUENCES.  Pages fetched by feeding out_next back are pairwise disjoint and ascending across pages; those pages of the
 *    brute-force form, concatenated, are the full paged order; with the start cursor a query served at stage 0 has the multiset of
 *    hnsw_search_batch's row, and that row bit for bit where the row's distances are distinct (rows whose walk distances are exact
 *    over the float32 rows: float32, byte and split rows; under half rows and codes the row is that of the re-ranked W_ef).
 * 6. COUNTERS are those of hnsw_search_batch_filtered: the evaluations and hops of every stage walked (inexact rows: plus the
 *    re-ranked members), the stage that served the query; the exact stage adds the number of allowed live nodes.  ERRORS are those
 *    of hnsw_search_batch_filtered -- k > ef, ef > 1024, HNSW_SEM_FUNCTOR_NEAREST_K, an empty index for the graph form, a stale or
 *    foreign filter, strides, null buffers; nq == 0 is a no-op -- and outputs are untouched on error.
 * 7. DETERMINISM: a row depends on the query's vector, its cursor, the mask and (ef, k, semantics) only -- not on the batch.
 * 8. Scratch is the handle's: one filtered, range or paged call in flight per handle.  The cursors are host arrays, 8 bytes per
 *    query, uploaded with the call.
 * 9. NOT BUILT: device-pointer forms; per-query filters; keyed output (hnsw_index_keys_of turns the ids into keys); the
 *    hnsw_sharded and hnsw_multi forms; cursors that survive hnsw_index_remove, hnsw_index_compact or an upsert -- those calls
 *    RENUMBER the nodes, and a cursor names a position by id.
 * 10. COST, plainly: results past about rank 1024 - k are exact-scan results (a pass over the whole table per page), and the last,
 *    short page walks the whole ladder first.  Rates: tools/after_rate.py, profiles/after.txt. */
typedef struct hnsw_cursor { float dist; int32_t id; } hnsw_cursor;   /* id: id_base-based */
#define HNSW_CURSOR_START { -INFINITY, INT32_MIN }                     /* an initialiser: before every node */

int32_t hnsw_search_batch_after(hnsw_index *idx, const hnsw_filter *f /* may be NULL */,
                                const hnsw_cursor *after /* [nq]; NULL: HNSW_CURSOR_START for every query */, const float *queries,
                                int64_t nq, int64_t q_stride, const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                                hnsw_cursor *out_next /* optional [nq] */, uint32_t *out_ndist, uint32_t *out_nhops,
                                uint32_t *out_stage /* each optional */);
int32_t hnsw_brute_force_batch_after(hnsw_index *idx, const hnsw_filter *f /* may be NULL */, const hnsw_cursor *after,
                                     const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill, int32_t *out_ids,
                                     float *out_dist, hnsw_cursor *out_next /* optional [nq] */);

/* ++++ diversified k-NN search: greedy maximal marginal relevance (MMR) over a pool of candidates ++++
 * On real corpora the k nearest are near-duplicates of each other: chunks of one document, re-posts, product variants.  MMR takes
 * a POOL of p > k candidates and picks k of them greedily, trading nearness to the query against nearness to what is already
 * picked.  It needs no labels (hnsw_search_batch_grouped does), only the vectors, and those are resident: the pool's ids and rows
 * never cross the link, only [nq][k] comes down.
 *
 * 0. THE OPERATOR: hnsw_diversify_batch (host arrays) and hnsw_diversify_batch_device (device pointers, asynchronous on `stream`).
 *    ONE definition; the two searches of point 4 are compositions over it.
 *    CANDIDATES are exactly hnsw_rerank_batch's: cand[q][0 .. cand_stride) id_base-based, entries < id_base are padding, the ids
 *    of a row distinct, cand_stride in 1..1024.  In the host form an id >= id_base + n is HNSW_ERR_BAD_ARG, named, refused
 *    before any launch; the device form skips it.  C is the real candidates of a row, c = |C|.
 * 1. THE NUMBERS.  r(v), the RELEVANCE, is the float hnsw_distance_batch returns for (query q, node v): over the float32 rows
 *    whatever row_format says.  rank(v) is v's position in the row hnsw_rerank_batch returns for the same candidates with
 *    k = cand_stride -- the order (key, id) of hnsw_brute_force_batch; every tie below is broken by it, no new order is invented.
 *    D(s, v), the PAIR DISTANCE, is the float hnsw_distance_batch returns with the stored float32 row of s as the query and v as
 *    the id.  Under HNSW_METRIC_COSINE the twin contract holds as everywhere: the call answers with the bits of the inner-product
 *    index over N(X) called with N(Q); the stored rows are not normalised again.
 * 2. SELECTION.  mu = fl(1.0f - lambda), computed once in float32.  Pick 1 is the candidate of rank 0.  After the picks S, for every
 *    v not yet picked m(v) = min over s in S of D(s, v) and
 *        g(v) = fl( fl(lambda * r(v)) - fl(mu * m(v)) )
 *    -- three separately rounded float32 operations, no fused multiply-add (numpy: lambda * r - mu * m on float32 arrays).  The next
 *    pick is the v with the smallest g, compared as IEEE values (-0 equals +0); among equal g the smallest rank wins.  Repeat until
 *    k are picked or C is exhausted.
 * 3. OUTPUT, in SELECTION ORDER, which is not ascending by distance: out_ids[q][j] id_base-based, out_dist[q][j] = r, out_div[q][j]
 *    (optional) = m at the moment of selection, +inf for pick 1.  Past min(k, c) ids and distances take hnsw_rerank_batch's fill
 *    (id -1; NaN or +inf) and out_div the same float.
 *    CONSEQUENCES: with lambda = 1 ids and distances are bit for bit hnsw_rerank_batch's; a query's row depends on its own
 *    candidates only, not on the batch; NaN in data or query: no promise.
 *    REFUSED (HNSW_ERR_BAD_ARG unless named; outputs untouched; nq == 0 is a no-op): a null handle or array (out_div may be null),
 *    nq < 0, q_stride < d, cand_stride < 1 (> 1024: HNSW_ERR_UNSUPPORTED), k outside 1..cand_stride, an unknown fill, lambda NaN
 *    or outside [0, 1].
 * 4. THE SEARCHES.  hnsw_search_batch_diverse is, bit for bit, hnsw_search_batch with k := pool (hnsw_search_batch_filtered when a
 *    filter is given) followed by hnsw_diversify_batch over its id rows with k = params->k, lambda, and params->fill: the inner
 *    call's rows of -1 are the padding; out_nd, out_nh and out_status are the inner call's counters unchanged (out_status: what the
 *    filtered call writes as out_stage; zero from the plain call); params->k <= pool <= params->ef, else HNSW_ERR_BAD_ARG (pool
 *    > 1024: HNSW_ERR_UNSUPPORTED).  Everything the inner call does is inherited, not restated: row formats and option refine,
 *    COSINE, marks (a marked index takes the filtered path, so no marked node is a candidate), the ordering pre-pass, the
 *    tie-overflow repair, option filter_collect, every refusal.  The selection launch follows the search on the handle's stream and
 *    reads the ids where the search left them.
 *    hnsw_brute_force_batch_diverse is the same composition over hnsw_brute_force_batch with k <= pool <= 1024.  It takes no
 *    filter: a filtered exact top-k under (key, id) does not exist as a call.
 * 5. Scratch -- the pool's rows, the selection's rows before their download -- is the handle's, sized on demand, not counted in
 *    device_bytes: one such call in flight per handle.
 * 6. NOT BUILT: per-query filters; keyed output (hnsw_index_keys_of translates the ids); device-pointer forms of the two searches
 *    (a device-resident caller composes hnsw_search_batch_device and hnsw_diversify_batch_device on one stream); the hnsw_sharded
 *    and hnsw_multi forms; a per-query lambda.
 * 7. COST, plainly: a selection evaluates c + (k - 1) * (at most c - 1) rows per query, each round re-reading the pool's rows:
 *    at pool 128, k 10 the order of one walk at ef 128.  Rates: tools/diverse_rate.py, profiles/diverse.txt. */
int32_t hnsw_diversify_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const int32_t *cand,
                             int32_t cand_stride, int32_t k, float lambda, int32_t fill, int32_t *out_ids, float *out_dist,
                             float *out_div /* may be NULL */);
int32_t hnsw_diversify_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, const int32_t *d_cand,
                                    int32_t cand_stride, int32_t k, float lambda, int32_t fill, int32_t *d_ids, float *d_dist,
                                    float *d_div /* may be NULL */, void *stream);
int32_t hnsw_search_batch_diverse(hnsw_index *idx, const hnsw_filter *filter /* may be NULL */, const float *queries, int64_t nq,
                                  int64_t q_stride, const hnsw_search_params *params, int32_t pool, float lambda, int32_t *out_ids,
                                  float *out_dist, float *out_div /* may be NULL */, uint32_t *out_nd, uint32_t *out_nh,
                                  uint32_t *out_status /* each optional */);
int32_t hnsw_brute_force_batch_diverse(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t pool,
                                       float lambda, int32_t fill, int32_t *out_ids, float *out_dist, float *out_div /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* HNSW_MI355X_H */
