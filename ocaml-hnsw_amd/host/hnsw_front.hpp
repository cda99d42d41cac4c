// hnsw_front.hpp -- C++ host-side mirror of the reference's module interface for the search path,
// over the C ABI of include/hnsw_mi355x.h (header only; link with libhnsw_mi355x.so).
//
//   Hnsw::Ohnsw::knn / knn_batch_bigarray / build_batch_bigarray / insert / distance_l2   lib/ohnsw.ml:766-899
//   Hnsw::Ohnsw::rerank                                                                    (hnsw_rerank_batch; nothing in the reference)
//   Hnsw::Filter, Hnsw::Ohnsw::knn_filtered                                                (hnsw_filter_*, hnsw_search_batch_filtered)
//   Hnsw::Filter::by_label / bits, Hnsw::Ohnsw::knn_filtered_each                          (hnsw_filter_create_by_label, hnsw_filter_bits,
//                                                                                           hnsw_search_batch_filtered_each)
//   Hnsw::Labels, Hnsw::Ohnsw::knn_grouped / brute_force_grouped                           (hnsw_labels_*, hnsw_search_batch_grouped,
//                                                                                           hnsw_brute_force_batch_grouped)
//   Hnsw::RangeResult, Hnsw::Ohnsw::range_search / brute_force_range                       (hnsw_range_*; with a Filter: the _filtered forms)
//   Hnsw::Ohnsw::mark_deleted / unmark_deleted / deleted_count / deleted_mask / compact    (hnsw_index_mark_deleted ... hnsw_index_compact)
//   Hnsw::Ohnsw::upsert_keyed / update                            hnsw_index_upsert_keyed / hnsw_index_update (replace or add, all or nothing)
//   Hnsw::Ohnsw::set_keys / clear_keys / keys_info / keys_of / find_keys / knn_keyed / insert_keyed / remove_keys /
//   mark_deleted_keys / unmark_deleted_keys, Hnsw::Filter::by_keys                         (hnsw_index_set_keys ... hnsw_filter_create_by_keys)
//   Hnsw::Ohnsw::knn_by_id / knn_by_key / brute_force_by_id / knn_graph / rows_device      (hnsw_search_batch_by_id, hnsw_search_batch_by_key,
//                                                                                           hnsw_brute_force_batch_by_id, hnsw_knn_graph,
//                                                                                           hnsw_index_get_rows_device)
//   Hnsw::Cursor, Hnsw::Ohnsw::knn_after / brute_force_after                               (hnsw_search_batch_after, hnsw_brute_force_batch_after)
//   Hnsw::Ohnsw::diversify / knn_diverse / brute_force_diverse                             (hnsw_diversify_batch, hnsw_search_batch_diverse,
//                                                                                           hnsw_brute_force_batch_diverse)
//   Hnsw::Ohnsw::brute_force_knn                                                           benchmark/dataset.ml:15-30
//   Hnsw::Ba::knn / knn_batch                                                    lib/hnsw.ml:763-777
//   Hnsw::Ohnsw::search_k / search_one, Hnsw::Ba::search                         lib/ohnsw.ml:492-588, lib/hnsw_algo.ml:350-437
//   Hnsw::MultiHgraph (one process, several GPUs)                                SURVEY 8e
//   Hnsw::Sharded, Hnsw::merge_lists (the rows partitioned over several GPUs)    (hnsw_sharded_*, hnsw_merge_lists)
//   Hnsw::ShardedFilter, Hnsw::ShardedRangeResult, Hnsw::Sharded::knn_filtered / range_search / brute_force_range,
//   Hnsw::merge_segments                                                         (hnsw_sharded_filter_*, hnsw_sharded_search_batch_filtered,
//                                                                                 hnsw_sharded_range_*, hnsw_merge_segments)
//   Hnsw::Stats::compute (Hgraph.Stats)                                        lib/hnsw.ml:353-375
//   Hnsw::HostMat (a page-locked Lacaml-shaped matrix the device accesses directly: hnsw_host_alloc)
//
// Same names, argument meaning and error behaviour: OCaml Invalid_argument -> std::invalid_argument
// ("knn: empty hgraph", lib/ohnsw.ml:862), Failure -> std::runtime_error.  A `Mat` is a
// Lacaml.S.mat (dim x n, Fortran layout): in memory n rows of dim contiguous floats.
#pragma once
#include "../../include/hnsw_mi355x.h"

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace Hnsw {

struct Mat {
    const float *data;
    int64_t dim2; // number of vectors (Lacaml.S.Mat.dim2)
    int32_t dim1; // dimension (Lacaml.S.Mat.dim1)
};

inline void check(int rc) {
    if (rc == HNSW_OK) return;
    const std::string msg = hnsw_last_error();
    if (rc == HNSW_ERR_BAD_ARG || rc == HNSW_ERR_EMPTY_INDEX || rc == HNSW_ERR_DEGREE_OVERFLOW) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

// hnsw_index_info.row_format: what the knn searches read (HNSW_ROWS_*); HALF only after hnsw_index_set_option(h, "half_rows", 1),
// which makes them search the vectors rounded to fp16; SQ8 only after hnsw_index_set_option(h, "sq8_rows", 1), which makes them
// walk 8-bit codes of the vectors and re-rank over the float32 rows; SQ8_DIM only after hnsw_index_set_option(h, "sq8_dim_rows", 1):
// the same with one affine map per dimension; BITS only after hnsw_index_set_option(h, "bit_rows", 1 or 2): one bit per dimension,
// walked under Hamming distance and re-ranked over the float32 rows
namespace Rows {
constexpr int F32 = HNSW_ROWS_F32, BYTES = HNSW_ROWS_BYTES, SPLIT = HNSW_ROWS_SPLIT, HALF = HNSW_ROWS_HALF, SQ8 = HNSW_ROWS_SQ8;
constexpr int SQ8_DIM = HNSW_ROWS_SQ8_DIM;
constexpr int BITS = HNSW_ROWS_BITS;
}

// Flattened Ohnsw.Hgraph.t / Hnsw.Ba.Hgraph.t resident on the device.
class Hgraph {
public:
    Hgraph() = default;
    Hgraph(const Hgraph &) = delete;
    Hgraph &operator=(const Hgraph &) = delete;
    Hgraph(Hgraph &&o) noexcept : h_(o.h_), id_base_(o.id_base_), d_(o.d_) { o.h_ = nullptr; }
    ~Hgraph() { if (h_) hnsw_index_destroy(h_); }

    // flatten + upload (hnsw_index_create)
    static Hgraph create(const hnsw_index_desc &desc, int device = 0) {
        Hgraph g;
        check(hnsw_index_create(&desc, device, &g.h_));
        g.id_base_ = desc.id_base; g.d_ = desc.d;
        return g;
    }
    hnsw_index *handle() const { return h_; }
    int id_base() const { return id_base_; }
    int dim() const { return d_; }

private:
    friend struct Builder;
    hnsw_index *h_ = nullptr;
    int id_base_ = 0, d_ = 0;
public:
    static Hgraph adopt(hnsw_index *h, int id_base, int d) { Hgraph g; g.h_ = h; g.id_base_ = id_base; g.d_ = d; return g; }
};

struct value_distance { int node; float distance_to_target; }; // lib/hnsw_algo.ml:85

// An allow-mask over the nodes of one index, resident on its device (hnsw_filter_create): allow[v] = node v + id_base may be
// returned by Ohnsw::knn_filtered.  One entry per node; refused by the search once the index has grown or shrunk (Ohnsw::insert, Ohnsw::remove).  Destroy
// it before its index.
class Filter {
public:
    Filter(const Hgraph &g, const std::vector<bool> &allow) {
        std::vector<uint32_t> bits((allow.size() + 31) / 32, 0u);
        for (size_t v = 0; v < allow.size(); ++v) if (allow[v]) bits[v >> 5] |= 1u << (v & 31);
        check(hnsw_filter_create(g.handle(), bits.data(), (int64_t)allow.size(), &f_));
        n_ = (int64_t)allow.size();
    }
    // ... from the packed words themselves: bit (v & 31) of word (v >> 5) = node v, n_bits = the index's n
    Filter(const Hgraph &g, const uint32_t *bits, int64_t n_bits) : n_(n_bits) { check(hnsw_filter_create(g.handle(), bits, n_bits, &f_)); }
    Filter(const Filter &) = delete;
    Filter &operator=(const Filter &) = delete;
    Filter(Filter &&o) noexcept : f_(o.f_), n_(o.n_) { o.f_ = nullptr; }
    ~Filter() { if (f_) hnsw_filter_destroy(f_); }
    const hnsw_filter *handle() const { return f_; }
    int64_t count() const { int64_t c = 0; check(hnsw_filter_count(f_, &c)); return c; }   // the allowed nodes
    // n_labels filters from one label per node (hnsw_filter_create_by_label): filter l allows node v iff labels[v] == l; a label
    // of -1 puts the node in no filter.  One entry per node of the index; all or nothing.
    static std::vector<Filter> by_label(const Hgraph &g, const std::vector<int32_t> &labels, int n_labels) {
        std::vector<hnsw_filter *> raw((size_t)(n_labels > 0 ? n_labels : 0), nullptr);
        check(hnsw_filter_create_by_label(g.handle(), labels.data(), (int64_t)labels.size(), n_labels, raw.data()));
        std::vector<Filter> out;
        out.reserve(raw.size());
        for (hnsw_filter *f : raw) out.push_back(Filter(f, (int64_t)labels.size()));
        return out;
    }
    // exactly the nodes with these keys of an index that owns keys (hnsw_filter_create_by_keys): repeats are fine, an absent key is
    // refused; ANDed with the live mask as every filter is
    static Filter by_keys(const Hgraph &g, const std::vector<int64_t> &keys) {
        hnsw_index_info inf{};
        check(hnsw_index_get_info(g.handle(), &inf));
        hnsw_filter *f = nullptr;
        check(hnsw_filter_create_by_keys(g.handle(), keys.data(), (int64_t)keys.size(), &f));
        return Filter(f, inf.n);
    }
    // the mask as the device holds it (hnsw_filter_bits): ceil(n / 32) words, bit (v & 31) of word (v >> 5) = node v
    std::vector<uint32_t> bits() const {
        std::vector<uint32_t> w((size_t)((n_ + 31) / 32) + 1, 0u);
        check(hnsw_filter_bits(f_, w.data()));
        w.pop_back();
        return w;
    }
private:
    Filter(hnsw_filter *f, int64_t n) : f_(f), n_(n) {}
    hnsw_filter *f_ = nullptr;
    int64_t n_ = 0;
};

// One label per node of one index, resident on its device (hnsw_labels_create): the groups of Ohnsw::knn_grouped.  labels[v] in
// -1 .. n_labels - 1, -1: node v is in no group.  One entry per node; refused once the index has changed (Ohnsw::insert,
// Ohnsw::remove, mark_deleted, unmark_deleted).  Destroy it before its index.
class Labels {
public:
    Labels(const Hgraph &g, const std::vector<int32_t> &labels, int n_labels) : n_((int64_t)labels.size()) {
        check(hnsw_labels_create(g.handle(), labels.data(), n_, n_labels, &l_));
    }
    Labels(const Labels &) = delete;
    Labels &operator=(const Labels &) = delete;
    Labels(Labels &&o) noexcept : l_(o.l_), n_(o.n_) { o.l_ = nullptr; }
    ~Labels() { if (l_) hnsw_labels_destroy(l_); }
    const hnsw_labels *handle() const { return l_; }
    struct Info { int32_t n_labels; int64_t n_labelled, n_groups; };
    // n_labelled: the nodes with a label >= 0; n_groups: the labels at least one node carries
    Info info() const { Info i{}; check(hnsw_labels_info(l_, &i.n_labels, &i.n_labelled, &i.n_groups)); return i; }
    // the labels as the device holds them (hnsw_labels_get): -1 where the node was marked deleted at creation
    std::vector<int32_t> get() const {
        std::vector<int32_t> out((size_t)n_ + 1, 0);
        check(hnsw_labels_get(l_, out.data()));
        out.pop_back();
        return out;
    }
private:
    hnsw_labels *l_ = nullptr;
    int64_t n_ = 0;
};

// What a range call returns, resident on one device: lims [nq + 1], ids and distances [total]; query q's segment is [lims[q],
// lims[q + 1]), ascending under (distance, id).  Owns its device buffers; any number may be alive.  Id and R: the id type and the
// ABI's result type, whose four functions follow.
template <class Id, class R, int32_t (*Size)(const R *, int64_t *, int64_t *),
          int32_t (*Fetch)(R *, int64_t *, Id *, float *, uint32_t *, uint32_t *, uint32_t *),
          int32_t (*Device)(R *, const int64_t **, const Id **, const float **), int32_t (*Destroy)(R *)>
class RangeResultOf {
public:
    static constexpr uint32_t exact_stage = 0xFFFFFFFFu;
    struct Host { std::vector<int64_t> lims; std::vector<Id> ids; std::vector<float> dist; std::vector<uint32_t> ndist, nhops, stage; };
    explicit RangeResultOf(R *r) : r_(r) {}
    RangeResultOf(const RangeResultOf &) = delete;
    RangeResultOf &operator=(const RangeResultOf &) = delete;
    RangeResultOf(RangeResultOf &&o) noexcept : r_(o.r_) { o.r_ = nullptr; }
    ~RangeResultOf() { if (r_) Destroy(r_); }
    R *handle() const { return r_; }
    int64_t nq() const { int64_t a = 0, b = 0; check(Size(r_, &a, &b)); return a; }
    int64_t total() const { int64_t a = 0, b = 0; check(Size(r_, &a, &b)); return b; }
    // everything on the host (the _fetch function)
    Host fetch() const {
        const size_t n = (size_t)nq(), t = (size_t)total();
        Host h{std::vector<int64_t>(n + 1, 0), std::vector<Id>(t), std::vector<float>(t), std::vector<uint32_t>(n), std::vector<uint32_t>(n),
               std::vector<uint32_t>(n)};
        check(Fetch(r_, h.lims.data(), h.ids.data(), h.dist.data(), h.ndist.data(), h.nhops.data(), h.stage.data()));
        return h;
    }
    // borrowed device pointers, valid while this object lives (the _device function)
    void device(const int64_t **d_lims, const Id **d_ids, const float **d_dist) const { check(Device(r_, d_lims, d_ids, d_dist)); }
private:
    R *r_ = nullptr;
};
// ... of one index (hnsw_range_result): int32 ids, on the index's device
using RangeResultBase = RangeResultOf<int32_t, hnsw_range_result, hnsw_range_result_size, hnsw_range_result_fetch, hnsw_range_result_device,
                                      hnsw_range_result_destroy>;
class RangeResult : public RangeResultBase { using RangeResultBase::RangeResultBase; };

// The sq8 copy of an index (hnsw_index_set_option(h, "sq8_rows", 1)): x ~ lo + scale * code; codes: [n][d] bytes.  Throws
// std::invalid_argument when the index has no such copy.
struct Sq8 { float lo, scale; std::vector<uint8_t> codes; };
inline Sq8 sq8(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    Sq8 out{0.0f, 1.0f, std::vector<uint8_t>((size_t)inf.n * (size_t)inf.d)};
    check(hnsw_index_sq8_params(g.handle(), &out.lo, &out.scale));
    check(hnsw_index_sq8_codes(g.handle(), out.codes.data()));
    return out;
}

// The per-dimension sq8 copy of an index (hnsw_index_set_option(h, "sq8_dim_rows", 1)): x[i] ~ lo[i] + scale[i] * code[i]; lo, scale:
// [d]; codes: [n][d] bytes.  Throws std::invalid_argument when the index has no such copy.
struct Sq8Dim { std::vector<float> lo, scale; std::vector<uint8_t> codes; };
inline Sq8Dim sq8_dim(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    Sq8Dim out{std::vector<float>((size_t)inf.d), std::vector<float>((size_t)inf.d), std::vector<uint8_t>((size_t)inf.n * (size_t)inf.d)};
    check(hnsw_index_sq8_dim_params(g.handle(), out.lo.data(), out.scale.data()));
    check(hnsw_index_sq8_dim_codes(g.handle(), out.codes.data()));
    return out;
}

// The 1-bit copy of an index (hnsw_index_set_option(h, "bit_rows", 1 or 2)): bit i of a row is x[i] > t[i]; t: [d]; codes:
// [n][words] uint32 with words = ceil(d / 32), dimension i in bit i % 32 of word i / 32.  Throws std::invalid_argument while the
// option is off.
struct Bits { std::vector<float> t; std::vector<uint32_t> codes; size_t words; };
inline Bits bits(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    const size_t words = ((size_t)inf.d + 31) / 32;
    Bits out{std::vector<float>((size_t)inf.d), std::vector<uint32_t>((size_t)inf.n * words), words};
    check(hnsw_index_bit_params(g.handle(), out.t.data()));
    check(hnsw_index_bit_codes(g.handle(), out.codes.data()));
    return out;
}

// The 4-bit query codes of option "bit_query_bits" (hnsw_index_set_option(h, "bit_query_bits", 4): the walk over the bit rows keeps
// the query at 4 bits a dimension): for Q, [nq][d] floats, the [nq][d] codes in -7..7 the walk would use.  Throws
// std::invalid_argument while option "bit_rows" is off.
inline std::vector<int8_t> bit_query_codes(const Hgraph &g, const std::vector<float> &Q) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    const size_t d = (size_t)inf.d, nq = d ? Q.size() / d : 0;
    std::vector<int8_t> out(nq * d);
    check(hnsw_index_bit_query_codes(g.handle(), Q.data(), (int64_t)nq, (int64_t)d, out.data()));
    return out;
}

// N(X) (hnsw_normalise_batch): every vector of `batch` scaled to unit length by the normaliser the header defines -- the rows a
// HNSW_METRIC_COSINE index stores for X and searches for a query batch X -- as [n][dim] floats; norms (optional): the n norms.  A
// zero vector stays zero, a vector whose sum of squares is not finite becomes NaN.  The metric itself is accepted wherever one is:
// hnsw_index_desc.metric (Hgraph::create), Ohnsw::build_batch_bigarray, hnsw_build_params.metric (Sharded::build).
inline std::vector<float> normalise(const Mat &batch, int device = 0, std::vector<float> *norms = nullptr) {
    std::vector<float> out((size_t)batch.dim2 * (size_t)batch.dim1);
    if (norms) norms->assign((size_t)batch.dim2, 0.f);
    check(hnsw_normalise_batch(device, batch.data, batch.dim2, batch.dim1, batch.dim1, out.data(), batch.dim1, norms ? norms->data() : nullptr));
    return out;
}

// A Lacaml-shaped float32 matrix (dim x n) in page-locked memory the library allocates (hnsw_host_alloc): knn_batch*
// reads such a query matrix straight from the device, without an upload step.
class HostMat {
public:
    HostMat(int32_t dim, int64_t n) : dim_(dim), n_(n) {
        void *p = nullptr;
        check(hnsw_host_alloc(&p, (int64_t)sizeof(float) * dim * (n > 0 ? n : 1)));
        data_ = static_cast<float *>(p);
    }
    HostMat(const HostMat &) = delete;
    HostMat &operator=(const HostMat &) = delete;
    ~HostMat() { if (data_) hnsw_host_free(data_); }
    float *data() { return data_; }
    float *col(int64_t j) { return data_ + j * dim_; }          // Lacaml.S.Mat.col m (j + 1)
    Mat mat() const { return Mat{data_, n_, dim_}; }
private:
    float *data_ = nullptr;
    int32_t dim_;
    int64_t n_;
};

// Hgraph.Stats (lib/hnsw.ml:353-375): per layer its size and the mima record {min; max; mean; isolated}; `isolated` is the
// reference's list -- node ids, descending (consed during the ascending fold of min_max_connectivity).
// a position in the paged order (hnsw_cursor): the (distance, id) of the last result a caller holds; start(): before every node
struct Cursor : hnsw_cursor {
    Cursor() : hnsw_cursor(HNSW_CURSOR_START) {}
    Cursor(float dist_, int32_t id_) : hnsw_cursor{dist_, id_} {}
    static Cursor start() { return Cursor(); }
};
static_assert(sizeof(Cursor) == sizeof(hnsw_cursor), "Hnsw::Cursor is laid out as hnsw_cursor");

namespace Stats {
struct mima { int min, max; double mean; std::vector<int64_t> isolated; };
struct t { int64_t num_nodes; std::vector<int64_t> layer_sizes; std::vector<mima> layer_connectivity; };
inline t compute(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    t out{inf.n, {}, {}};
    for (int layer = 0; layer <= inf.max_layer; ++layer) {
        hnsw_layer_stats s{};
        check(hnsw_index_layer_stats(g.handle(), layer, &s));
        mima m{s.min_degree, s.max_degree, s.mean_degree, std::vector<int64_t>((size_t)s.num_isolated)};
        int64_t cnt = 0;
        check(hnsw_index_layer_isolated(g.handle(), layer, m.isolated.data(), s.num_isolated, &cnt));
        out.layer_sizes.push_back(s.num_nodes);
        out.layer_connectivity.push_back(std::move(m));
    }
    return out;
}
} // namespace Stats

namespace detail {
inline void search(const Hgraph &g, const Mat &batch, int ef, int k, int fill, std::vector<int32_t> &ids, std::vector<float> &dist, int sem = HNSW_SEM_OHNSW) {
    ids.assign((size_t)batch.dim2 * k, -1);
    dist.assign((size_t)batch.dim2 * k, 0.f);
    hnsw_search_params p{ef, k, fill, sem};
    check(hnsw_search_batch(g.handle(), batch.data, batch.dim2, batch.dim1, &p, ids.data(), dist.data(), nullptr, nullptr));
}
} // namespace detail

namespace Ohnsw {

// Ohnsw.build_batch_bigarray distance batch ~num_connections ~num_nodes_search_construction
// (lib/ohnsw.ml:840-857), batched on the device.
inline Hgraph build_batch_bigarray(const Mat &batch, int num_connections, int num_nodes_search_construction,
                                   uint64_t seed = 0, int metric = HNSW_METRIC_L2, int device = 0, int expected_ef = 0) {
    hnsw_build_params p{num_connections, num_nodes_search_construction, metric, 0, seed, 0, 0, expected_ef, HNSW_SEM_OHNSW};
    hnsw_index *h = nullptr;
    check(hnsw_build(batch.data, batch.dim2, batch.dim1, batch.dim1, &p, device, &h));
    return Hgraph::adopt(h, 0, batch.dim1);
}

// Ohnsw.insert (lib/ohnsw.ml:766-837) for every vector of `batch`, in order, into g on the device (hnsw_index_insert): the
// graph grows in place, the new ids follow the old ones.  Returns the first new id.  Levels are the draws
// build_batch_bigarray with the same seed gives those positions.
inline int64_t insert(Hgraph &g, const Mat &batch, int num_connections, int num_nodes_search_construction,
                      uint64_t seed = 0, int max_batch = 0, int expected_ef = 0) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    hnsw_build_params p{num_connections, num_nodes_search_construction, inf.metric, inf.id_base, seed, max_batch, 0, expected_ef, HNSW_SEM_OHNSW};
    check(hnsw_index_insert(g.handle(), batch.data, batch.dim2, batch.dim1, &p));
    return inf.n + inf.id_base;
}

// The float32 rows g holds for the nodes `ids` (id_base-based; hnsw_index_get_rows) as [ids.size()][dim] floats, or -- no ids --
// all n rows in order.  For a HNSW_METRIC_COSINE index these are N(X), not the vectors it was handed.
inline std::vector<float> rows(const Hgraph &g, const std::vector<int64_t> &ids) {
    std::vector<float> out(ids.size() * (size_t)g.dim());
    if (ids.empty()) return out;
    check(hnsw_index_get_rows(g.handle(), ids.data(), (int64_t)ids.size(), out.data(), g.dim()));
    return out;
}
inline std::vector<float> rows(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<float> out((size_t)inf.n * (size_t)inf.d);
    check(hnsw_index_get_rows(g.handle(), nullptr, inf.n, out.data(), inf.d));
    return out;
}

// Hard deletion on the device (hnsw_index_remove): the stored nodes `ids` (id_base-based, distinct) leave g, the others keep
// their order and are renumbered, the graph is repaired by the three-pass rule the header defines.  Returns the new id of every
// old node (id_base - 1 for a removed one).
inline std::vector<int32_t> remove(Hgraph &g, const std::vector<int64_t> &ids) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<int32_t> new_id((size_t)inf.n);
    check(hnsw_index_remove(g.handle(), ids.data(), (int64_t)ids.size(), new_id.data()));
    return new_id;
}

// Soft deletion owned by the index (hnsw_index_mark_deleted): the stored nodes `ids` (id_base-based, distinct) stay in the graph but
// no search returns them any more -- while any node is marked the knn, brute-force and range searches answer under the mask of the
// live nodes.  unmark_deleted makes them live again; compact is remove() of the marked nodes (the new id of every old node).
inline void mark_deleted(Hgraph &g, const std::vector<int64_t> &ids) { check(hnsw_index_mark_deleted(g.handle(), ids.data(), (int64_t)ids.size())); }
inline void unmark_deleted(Hgraph &g, const std::vector<int64_t> &ids) { check(hnsw_index_unmark_deleted(g.handle(), ids.data(), (int64_t)ids.size())); }
inline int64_t deleted_count(const Hgraph &g) { int64_t c = 0; check(hnsw_index_deleted_count(g.handle(), &c)); return c; }
// one entry per node: node v + id_base is marked (hnsw_index_deleted_bits)
inline std::vector<bool> deleted_mask(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<uint32_t> w((size_t)((inf.n + 31) / 32) + 1, 0u);
    check(hnsw_index_deleted_bits(g.handle(), w.data()));
    std::vector<bool> out((size_t)inf.n);
    for (int64_t v = 0; v < inf.n; ++v) out[(size_t)v] = (w[(size_t)(v >> 5)] >> (v & 31)) & 1u;
    return out;
}
inline std::vector<int32_t> compact(Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<int32_t> new_id((size_t)inf.n);
    check(hnsw_index_compact(g.handle(), new_id.data()));
    return new_id;
}

// Ohnsw.knn hgraph visited ~k target (lib/ohnsw.ml:859-875): the MinQueue popped ascending.
inline std::vector<value_distance> knn(const Hgraph &g, int k, const float *target) {
    std::vector<int32_t> ids; std::vector<float> dist;
    detail::search(g, Mat{target, 1, g.dim()}, k, k, HNSW_FILL_OHNSW, ids, dist);
    std::vector<value_distance> out;
    for (int i = 0; i < k && ids[(size_t)i] >= g.id_base(); ++i) out.push_back({ids[(size_t)i], dist[(size_t)i]});
    return out;
}

// Ohnsw.knn_batch_bigarray hgraph ~k batch -> (ids, distances) (lib/ohnsw.ml:877-897):
// ids nq x k (-1 filled), distances k x nq Fortran = [nq][k] (NaN filled).
inline std::pair<std::vector<std::vector<int>>, std::vector<float>> knn_batch_bigarray(const Hgraph &g, int k, const Mat &batch) {
    std::vector<int32_t> ids; std::vector<float> dist;
    detail::search(g, batch, k, k, HNSW_FILL_OHNSW, ids, dist);
    std::vector<std::vector<int>> out((size_t)batch.dim2, std::vector<int>((size_t)k));
    for (int64_t j = 0; j < batch.dim2; ++j) for (int i = 0; i < k; ++i) out[(size_t)j][(size_t)i] = ids[(size_t)(j * k + i)];
    return {std::move(out), std::move(dist)};
}

// Ohnsw.search_k layer distance value visited start_nodes target k (lib/ohnsw.ml:543-588): one target,
// the start queue as a list of nodes; result_minq popped ascending.  `sem` = HNSW_SEM_FUNCTOR gives
// Hnsw_algo.Search.search (lib/hnsw_algo.ml:350-391).
inline std::vector<value_distance> search_k(const Hgraph &g, int layer, const std::vector<int64_t> &start_nodes,
                                            const float *target, int k, int sem = HNSW_SEM_OHNSW) {
    std::vector<int32_t> ids((size_t)k); std::vector<float> dist((size_t)k);
    int32_t cnt = 0;
    hnsw_search_params p{k, k, HNSW_FILL_OHNSW, sem};
    check(hnsw_search_layer_batch(g.handle(), layer, target, 1, g.dim(), start_nodes.data(), (int32_t)start_nodes.size(), &p,
                                  ids.data(), dist.data(), &cnt, nullptr, nullptr));
    std::vector<value_distance> out;
    for (int i = 0; i < cnt; ++i) out.push_back({ids[(size_t)i], dist[(size_t)i]});
    return out;
}

// Ohnsw.search_one layer distance value visited start_node target (lib/ohnsw.ml:492-512)
inline value_distance search_one(const Hgraph &g, int layer, int64_t start_node, const float *target) {
    int64_t node = 0; float d = 0.f;
    check(hnsw_search_one_batch(g.handle(), layer, target, 1, g.dim(), &start_node, &node, &d));
    return {(int)node, d};
}

// brute_force_knn_l2 (benchmark/dataset.ml:15-30) over the vectors the index holds (hnsw_brute_force_batch): for each query the k
// smallest of all stored vectors under (distance, id), ascending -> (ids, distances), both [nq][k] (-1 / NaN where k > n)
inline std::pair<std::vector<int32_t>, std::vector<float>> brute_force_knn(const Hgraph &g, int k, const Mat &batch) {
    std::vector<int32_t> ids((size_t)batch.dim2 * (size_t)(k > 0 ? k : 0));
    std::vector<float> dist(ids.size());
    check(hnsw_brute_force_batch(g.handle(), batch.data, batch.dim2, batch.dim1, k, HNSW_FILL_OHNSW, ids.data(), dist.data()));
    return {std::move(ids), std::move(dist)};
}

// EVERY node within `radius` of each query (hnsw_range_search_batch): W grows ef, 2 ef, ... 1024 until it is not saturated (fewer
// than e members, or the last one out of range) and its in-range prefix is the answer; a query saturated at 1024 gets the exact
// range scan (stage == RangeResult::exact_stage).  Distances are over the float32 vectors whatever rows the index searches.
inline RangeResult range_search(const Hgraph &g, float radius, const Mat &batch, int ef = 64, int sem = HNSW_SEM_OHNSW) {
    hnsw_range_params p{radius, ef, sem};
    hnsw_range_result *r = nullptr;
    check(hnsw_range_search_batch(g.handle(), batch.data, batch.dim2, batch.dim1, &p, &r));
    return RangeResult(r);
}

// ... its exact form (hnsw_range_brute_force_batch): per query the in-range prefix of the full order over all stored vectors
inline RangeResult brute_force_range(const Hgraph &g, float radius, const Mat &batch) {
    hnsw_range_result *r = nullptr;
    check(hnsw_range_brute_force_batch(g.handle(), batch.data, batch.dim2, batch.dim1, radius, &r));
    return RangeResult(r);
}

// ... both under an allow-mask (hnsw_range_search_batch_filtered, hnsw_range_brute_force_batch_filtered): each segment is the
// unfiltered one with the nodes the Filter does not allow left out; stage and hops are the unfiltered call's
inline RangeResult range_search(const Hgraph &g, const Filter &f, float radius, const Mat &batch, int ef = 64, int sem = HNSW_SEM_OHNSW) {
    hnsw_range_params p{radius, ef, sem};
    hnsw_range_result *r = nullptr;
    check(hnsw_range_search_batch_filtered(g.handle(), f.handle(), batch.data, batch.dim2, batch.dim1, &p, &r));
    return RangeResult(r);
}
inline RangeResult brute_force_range(const Hgraph &g, const Filter &f, float radius, const Mat &batch) {
    hnsw_range_result *r = nullptr;
    check(hnsw_range_brute_force_batch_filtered(g.handle(), f.handle(), batch.data, batch.dim2, batch.dim1, radius, &r));
    return RangeResult(r);
}

// knn_batch_bigarray among the nodes a Filter allows (hnsw_search_batch_filtered): W grows ef, 2 ef, ... 1024 until it holds k
// allowed nodes, a query still short gets the exact scan over the allowed nodes; distances are over the float32 vectors whatever
// rows the index searches.  ids / distances [nq][k] (-1 / NaN where fewer than k nodes are allowed); stage[q] = how often W
// doubled for query q, exact_stage = the exact scan.
// After hnsw_index_set_option(h, "filter_collect", 1) (off by default; k <= 128, float32 / byte / split rows) the answer comes from every
// node the layer-0 walk evaluates, not from the final W only: a query is served at the first stage whose walk evaluated k allowed
// nodes (the C header: WITH OPTION filter_collect).
struct Filtered {
    static constexpr uint32_t exact_stage = 0xFFFFFFFFu;
    std::vector<int32_t> ids; std::vector<float> dist; std::vector<uint32_t> stage;
};
inline Filtered knn_filtered(const Hgraph &g, const Filter &f, int k, const Mat &batch, int ef = 0, int sem = HNSW_SEM_OHNSW,
                             int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2;
    Filtered out{std::vector<int32_t>(nq * (size_t)(k > 0 ? k : 0), -1), std::vector<float>(nq * (size_t)(k > 0 ? k : 0), 0.f),
                 std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_filtered(g.handle(), f.handle(), batch.data, batch.dim2, batch.dim1, &p, out.ids.data(), out.dist.data(),
                                     nullptr, nullptr, out.stage.data()));
    return out;
}

// ... with one filter per query (hnsw_search_batch_filtered_each): query q is answered under filters[which[q]], its row the row
// knn_filtered gives it under that filter; a mixed batch of many tenants in one call.
inline Filtered knn_filtered_each(const Hgraph &g, const std::vector<Filter> &filters, const std::vector<int32_t> &which, int k, const Mat &batch,
                                  int ef = 0, int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2;
    if (which.size() != nq) throw std::invalid_argument("knn_filtered_each: one filter position per query");
    std::vector<const hnsw_filter *> table;
    for (const Filter &f : filters) table.push_back(f.handle());
    Filtered out{std::vector<int32_t>(nq * (size_t)(k > 0 ? k : 0), -1), std::vector<float>(nq * (size_t)(k > 0 ? k : 0), 0.f),
                 std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_filtered_each(g.handle(), table.data(), (int32_t)table.size(), which.data(), batch.data, batch.dim2, batch.dim1, &p,
                                          out.ids.data(), out.dist.data(), nullptr, nullptr, out.stage.data()));
    return out;
}

// The k nearest GROUPS, one node per label (hnsw_search_batch_grouped): W grows ef, 2 ef, ... 1024 until it holds nodes of k distinct
// labels, each label represented by its first eligible member of W; a query still short gets the exact grouped scan.  f (optional):
// only the nodes it allows count.  ids / distances / labels [nq][k] (-1 / NaN / -1 where there are fewer than k groups); stage as
// knn_filtered's.
struct Grouped {
    static constexpr uint32_t exact_stage = 0xFFFFFFFFu;
    std::vector<int32_t> ids; std::vector<float> dist; std::vector<int32_t> labels; std::vector<uint32_t> stage;
};
inline Grouped knn_grouped(const Hgraph &g, const Labels &l, int k, const Mat &batch, int ef = 0, const Filter *f = nullptr,
                           int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2, cells = nq * (size_t)(k > 0 ? k : 0);
    Grouped out{std::vector<int32_t>(cells, -1), std::vector<float>(cells, 0.f), std::vector<int32_t>(cells, -1), std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_grouped(g.handle(), l.handle(), f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, &p, out.ids.data(),
                                    out.dist.data(), out.labels.data(), nullptr, nullptr, out.stage.data()));
    return out;
}
// ... its exact form (hnsw_brute_force_batch_grouped): per label its nearest node under (distance, id) over all stored vectors, of
// those the k nearest, ascending.  Needs no graph; every stage reads exact_stage.
inline Grouped brute_force_grouped(const Hgraph &g, const Labels &l, int k, const Mat &batch, const Filter *f = nullptr,
                                   int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2, cells = nq * (size_t)(k > 0 ? k : 0);
    Grouped out{std::vector<int32_t>(cells, -1), std::vector<float>(cells, 0.f), std::vector<int32_t>(cells, -1),
                std::vector<uint32_t>(nq, Grouped::exact_stage)};
    check(hnsw_brute_force_batch_grouped(g.handle(), l.handle(), f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, k, fill,
                                         out.ids.data(), out.dist.data(), out.labels.data()));
    return out;
}

// ---- keys the index owns: one caller-chosen int64 per stored node, pairwise distinct, kept on the device in row order and moved with
// the nodes through insert_keyed, remove and compact (hnsw_index_set_keys ...; the definitions: include/hnsw_mi355x.h) ----
inline void set_keys(Hgraph &g, const std::vector<int64_t> &keys) { check(hnsw_index_set_keys(g.handle(), keys.data(), (int64_t)keys.size())); }
inline void clear_keys(Hgraph &g) { check(hnsw_index_clear_keys(g.handle())); }
// (has keys?, their bytes on the device: not part of hnsw_index_info.device_bytes)
inline std::pair<bool, int64_t> keys_info(const Hgraph &g) {
    int32_t has = 0; int64_t bytes = 0;
    check(hnsw_index_keys_info(g.handle(), &has, &bytes));
    return {has != 0, bytes};
}
// the keys of the nodes `ids` (id_base-based; `missing` where an id names no node, the searches' fill id -1 included) ...
inline std::vector<int64_t> keys_of(const Hgraph &g, const std::vector<int32_t> &ids, int64_t missing = -1) {
    std::vector<int64_t> out(ids.size());
    if (!ids.empty()) check(hnsw_index_keys_of(g.handle(), ids.data(), (int64_t)ids.size(), missing, out.data()));
    return out;
}
// ... and of all n nodes in row order
inline std::vector<int64_t> keys_of(const Hgraph &g) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<int64_t> out((size_t)inf.n + 1);
    check(hnsw_index_keys_of(g.handle(), nullptr, inf.n, 0, out.data()));
    out.pop_back();
    return out;
}
// the id_base-based ids of the nodes with these keys, id_base - 1 where no node has the key
inline std::vector<int64_t> find_keys(const Hgraph &g, const std::vector<int64_t> &keys) {
    std::vector<int64_t> out(keys.size());
    if (!keys.empty()) check(hnsw_index_find_keys(g.handle(), keys.data(), (int64_t)keys.size(), out.data()));
    return out;
}
// knn_batch_bigarray answered in keys (hnsw_search_batch_keyed): keys / distances [nq][k], `missing` / NaN where fewer than k were
// found; f (optional): the rows of knn_filtered under it.  stage as knn_filtered's, zero for the plain path.
struct Keyed {
    std::vector<int64_t> keys; std::vector<float> dist; std::vector<uint32_t> stage;
};
inline Keyed knn_keyed(const Hgraph &g, int k, const Mat &batch, int ef = 0, const Filter *f = nullptr, int64_t missing = -1,
                       int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2, cells = nq * (size_t)(k > 0 ? k : 0);
    Keyed out{std::vector<int64_t>(cells, missing), std::vector<float>(cells, 0.f), std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_keyed(g.handle(), f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, &p, missing, out.keys.data(),
                                  out.dist.data(), nullptr, nullptr, out.stage.data()));
    return out;
}
// insert() into an index that owns keys (hnsw_index_insert_keyed): keys[i] names vector i of `batch`; a stored or repeated key
// refuses the call before anything is built.  An empty index without keys starts its keys here.  Returns the first new id.
inline int64_t insert_keyed(Hgraph &g, const Mat &batch, const std::vector<int64_t> &keys, int num_connections, int num_nodes_search_construction,
                            uint64_t seed = 0, int max_batch = 0, int expected_ef = 0) {
    if ((int64_t)keys.size() != batch.dim2) throw std::invalid_argument("insert_keyed: one key per vector");
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    hnsw_build_params p{num_connections, num_nodes_search_construction, inf.metric, inf.id_base, seed, max_batch, 0, expected_ef, HNSW_SEM_OHNSW};
    check(hnsw_index_insert_keyed(g.handle(), batch.data, batch.dim2, batch.dim1, keys.data(), &p));
    return inf.n + inf.id_base;
}
// remove() / mark_deleted() / unmark_deleted() of the nodes with these keys: an absent key refuses the call, nothing changed
inline std::vector<int32_t> remove_keys(Hgraph &g, const std::vector<int64_t> &keys) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<int32_t> new_id((size_t)inf.n);
    check(hnsw_index_remove_keys(g.handle(), keys.data(), (int64_t)keys.size(), new_id.data()));
    return new_id;
}
inline void mark_deleted_keys(Hgraph &g, const std::vector<int64_t> &keys) { check(hnsw_index_mark_deleted_keys(g.handle(), keys.data(), (int64_t)keys.size())); }
inline void unmark_deleted_keys(Hgraph &g, const std::vector<int64_t> &keys) { check(hnsw_index_unmark_deleted_keys(g.handle(), keys.data(), (int64_t)keys.size())); }
// Replace or add vectors by key in one all-or-nothing call (hnsw_index_upsert_keyed): vector i of `batch` becomes the vector under
// keys[i], stored or not.  g afterwards is exactly what remove_keys(the stored ones among keys) + insert_keyed(batch, keys) leaves,
// with one table swap and one epoch step; on any error it is exactly as before.  Two equal keys in the call are refused.
struct Upserted { std::vector<uint8_t> replaced; std::vector<int32_t> new_id; };   // [m]: keys[i] was stored; [n_old]: as remove() returns it
inline Upserted upsert_keyed(Hgraph &g, const Mat &batch, const std::vector<int64_t> &keys, int num_connections, int num_nodes_search_construction,
                             uint64_t seed = 0, int max_batch = 0, int expected_ef = 0) {
    if ((int64_t)keys.size() != batch.dim2) throw std::invalid_argument("upsert_keyed: one key per vector");
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    hnsw_build_params p{num_connections, num_nodes_search_construction, inf.metric, inf.id_base, seed, max_batch, 0, expected_ef, HNSW_SEM_OHNSW};
    Upserted out{std::vector<uint8_t>(keys.size(), 0), std::vector<int32_t>((size_t)inf.n)};
    check(hnsw_index_upsert_keyed(g.handle(), batch.data, keys.data(), batch.dim2, batch.dim1, &p, out.replaced.data(), out.new_id.data()));
    return out;
}
// ... and for an index without keys (hnsw_index_update): the stored nodes `ids` (id_base-based, distinct) are replaced by the vectors
// of `batch`: exactly remove(ids) + insert(batch).  An index with keys is refused.  Returns new_id as remove() does.
inline std::vector<int32_t> update(Hgraph &g, const std::vector<int64_t> &ids, const Mat &batch, int num_connections, int num_nodes_search_construction,
                                   uint64_t seed = 0, int max_batch = 0, int expected_ef = 0) {
    if ((int64_t)ids.size() != batch.dim2) throw std::invalid_argument("update: one id per vector");
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    hnsw_build_params p{num_connections, num_nodes_search_construction, inf.metric, inf.id_base, seed, max_batch, 0, expected_ef, HNSW_SEM_OHNSW};
    std::vector<int32_t> new_id((size_t)inf.n);
    check(hnsw_index_update(g.handle(), ids.data(), batch.data, batch.dim2, batch.dim1, &p, new_id.data()));
    return new_id;
}
// ... and for ids already on the device, queued on `stream` (hnsw_index_keys_of_device)
inline void keys_of_device(Hgraph &g, const int32_t *d_ids, int64_t m, int64_t missing, int64_t *d_out, void *stream = nullptr) {
    check(hnsw_index_keys_of_device(g.handle(), d_ids, m, missing, d_out, stream));
}

// ---- search by stored item: the queries are rows the index holds, named by id or by key; only the ids cross the link (the
// definition: include/hnsw_mi355x.h, the last section) ----
// knn_batch_bigarray with the stored vectors of the nodes `ids` (int32, id_base-based: a search's output fits) as the queries
// (hnsw_search_batch_by_id) -> (ids, distances) [ids.size()][k].  exclude_self: the search runs k + 1 wide with ef' = max(ef, k + 1)
// and each row loses the node's own id (the first k entries if it is not among them); false: exactly the search over rows(ids).
inline std::pair<std::vector<int32_t>, std::vector<float>> knn_by_id(const Hgraph &g, int k, const std::vector<int32_t> &ids, int ef = 0,
                                                                      bool exclude_self = true, int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    std::vector<int32_t> out(ids.size() * (size_t)(k > 0 ? k : 0), -1);
    std::vector<float> dist(out.size(), 0.f);
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_by_id(g.handle(), ids.data(), (int64_t)ids.size(), &p, exclude_self ? 1 : 0, out.data(), dist.data(), nullptr, nullptr));
    return {std::move(out), std::move(dist)};
}
// ... for the nodes stored under `keys`, answered in keys (hnsw_search_batch_by_key); an absent key refuses the call
inline std::pair<std::vector<int64_t>, std::vector<float>> knn_by_key(const Hgraph &g, int k, const std::vector<int64_t> &keys, int ef = 0,
                                                                       bool exclude_self = true, int64_t missing = -1, int sem = HNSW_SEM_OHNSW,
                                                                       int fill = HNSW_FILL_OHNSW) {
    std::vector<int64_t> out(keys.size() * (size_t)(k > 0 ? k : 0), missing);
    std::vector<float> dist(out.size(), 0.f);
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_by_key(g.handle(), keys.data(), (int64_t)keys.size(), &p, exclude_self ? 1 : 0, missing, out.data(), dist.data(), nullptr, nullptr));
    return {std::move(out), std::move(dist)};
}
// ... the exact form (hnsw_brute_force_batch_by_id): brute_force_knn over the stored vectors of the nodes `ids`
inline std::pair<std::vector<int32_t>, std::vector<float>> brute_force_by_id(const Hgraph &g, int k, const std::vector<int32_t> &ids,
                                                                              bool exclude_self = true, int fill = HNSW_FILL_OHNSW) {
    std::vector<int32_t> out(ids.size() * (size_t)(k > 0 ? k : 0), -1);
    std::vector<float> dist(out.size(), 0.f);
    check(hnsw_brute_force_batch_by_id(g.handle(), ids.data(), (int64_t)ids.size(), k, fill, exclude_self ? 1 : 0, out.data(), dist.data()));
    return {std::move(out), std::move(dist)};
}
// the k-NN graph of the whole index (hnsw_knn_graph): row v = the row of knn_by_id (exact: of brute_force_by_id) for node
// id_base + v without the node itself -> (ids, distances) [n][k]
inline std::pair<std::vector<int32_t>, std::vector<float>> knn_graph(const Hgraph &g, int k, int ef = 0, bool exact = false, int sem = HNSW_SEM_OHNSW,
                                                                      int fill = HNSW_FILL_OHNSW) {
    hnsw_index_info inf{};
    check(hnsw_index_get_info(g.handle(), &inf));
    std::vector<int32_t> out((size_t)inf.n * (size_t)(k > 0 ? k : 0), -1);
    std::vector<float> dist(out.size(), 0.f);
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_knn_graph(g.handle(), &p, exact ? 1 : 0, out.data(), dist.data()));
    return {std::move(out), std::move(dist)};
}
// the stored float32 rows of the nodes d_ids (device int32, id_base-based) into the device matrix d_out, queued on `stream`
// (hnsw_index_get_rows_device); an id outside the index gives a row of zeros
inline void rows_device(Hgraph &g, const int32_t *d_ids, int64_t m, float *d_out, int64_t out_stride, void *stream = nullptr) {
    check(hnsw_index_get_rows_device(g.handle(), d_ids, m, d_out, out_stride, stream));
}

// ---- paged search: the NEXT k after a (distance, id) cursor (the definition: include/hnsw_mi355x.h, the last section) ----
// knn_after (hnsw_search_batch_after): `after` holds one cursor per query (empty: Cursor::start() for all, the first page); the
// order is (distance, id) over the returned float distances.  W grows ef, 2 ef, ... 1024 until it holds k nodes after the cursor
// (stage[q] = how often it doubled); a query still short gets the exact paged scan (exact_stage).  next[q] is the cursor to hand
// back for the page after; a row with fewer than k real entries means "exhausted".  f (optional): only allowed nodes count.
// Cursors do not survive remove(), compact() or an upsert: those renumber the nodes.
struct Paged {
    static constexpr uint32_t exact_stage = 0xFFFFFFFFu;
    std::vector<int32_t> ids; std::vector<float> dist; std::vector<Cursor> next; std::vector<uint32_t> stage;
};
inline Paged knn_after(const Hgraph &g, int k, const Mat &batch, const std::vector<Cursor> &after = {}, int ef = 0, const Filter *f = nullptr,
                       int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2;
    if (!after.empty() && after.size() != nq) throw std::invalid_argument("knn_after: one cursor per query");
    Paged out{std::vector<int32_t>(nq * (size_t)(k > 0 ? k : 0), -1), std::vector<float>(nq * (size_t)(k > 0 ? k : 0), 0.f),
              std::vector<Cursor>(nq, Cursor::start()), std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : k, k, fill, sem};
    check(hnsw_search_batch_after(g.handle(), f ? f->handle() : nullptr, after.empty() ? nullptr : after.data(), batch.data, batch.dim2, batch.dim1,
                                  &p, out.ids.data(), out.dist.data(), out.next.data(), nullptr, nullptr, out.stage.data()));
    return out;
}
// ... the exact form (hnsw_brute_force_batch_after): the first k nodes after each cursor over all stored vectors; needs no graph
inline Paged brute_force_after(const Hgraph &g, int k, const Mat &batch, const std::vector<Cursor> &after = {}, const Filter *f = nullptr,
                               int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2;
    if (!after.empty() && after.size() != nq) throw std::invalid_argument("brute_force_after: one cursor per query");
    Paged out{std::vector<int32_t>(nq * (size_t)(k > 0 ? k : 0), -1), std::vector<float>(nq * (size_t)(k > 0 ? k : 0), 0.f),
              std::vector<Cursor>(nq, Cursor::start()), std::vector<uint32_t>(nq, Paged::exact_stage)};
    check(hnsw_brute_force_batch_after(g.handle(), f ? f->handle() : nullptr, after.empty() ? nullptr : after.data(), batch.data, batch.dim2,
                                       batch.dim1, k, fill, out.ids.data(), out.dist.data(), out.next.data()));
    return out;
}

// ---- diversified search: greedy maximal marginal relevance over a pool (the definition: include/hnsw_mi355x.h, the last section) ----
// Rows are in SELECTION order: ids (-1 past the real candidates), dist = the distance to the query, div = the distance to the nearest
// earlier pick at the moment of selection (+inf for pick 1); status: the inner search's out_status (the graph form).
struct Diverse {
    std::vector<int32_t> ids; std::vector<float> dist, div; std::vector<uint32_t> status;
};
// diversify (hnsw_diversify_batch): k of ITS candidates cand[q][0 .. cand_stride) per query (entries below id_base are padding); pick 1
// is the nearest, every further pick minimises lambda * distance - (1 - lambda) * distance to the nearest pick.  lambda = 1 is rerank.
inline Diverse diversify(const Hgraph &g, int k, const Mat &batch, const int32_t *cand, int cand_stride, float lambda = 0.5f,
                         int fill = HNSW_FILL_OHNSW) {
    const size_t cells = (size_t)batch.dim2 * (size_t)(k > 0 ? k : 0);
    Diverse out{std::vector<int32_t>(cells, -1), std::vector<float>(cells, 0.f), std::vector<float>(cells, 0.f), {}};
    check(hnsw_diversify_batch(g.handle(), batch.data, batch.dim2, batch.dim1, cand, cand_stride, k, lambda, fill, out.ids.data(), out.dist.data(),
                               out.div.data()));
    return out;
}
// knn_diverse (hnsw_search_batch_diverse): the search at k := pool (under f: the filtered search), then diversify over its rows on the
// device; k <= pool <= ef (ef 0: pool)
inline Diverse knn_diverse(const Hgraph &g, int k, const Mat &batch, int pool, float lambda = 0.5f, int ef = 0, const Filter *f = nullptr,
                           int sem = HNSW_SEM_OHNSW, int fill = HNSW_FILL_OHNSW) {
    const size_t nq = (size_t)batch.dim2, cells = nq * (size_t)(k > 0 ? k : 0);
    Diverse out{std::vector<int32_t>(cells, -1), std::vector<float>(cells, 0.f), std::vector<float>(cells, 0.f), std::vector<uint32_t>(nq, 0u)};
    hnsw_search_params p{ef > 0 ? ef : pool, k, fill, sem};
    check(hnsw_search_batch_diverse(g.handle(), f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, &p, pool, lambda, out.ids.data(),
                                    out.dist.data(), out.div.data(), nullptr, nullptr, out.status.data()));
    return out;
}
// ... the exact form (hnsw_brute_force_batch_diverse): the pool is the exact scan's first `pool` nodes; needs no graph
inline Diverse brute_force_diverse(const Hgraph &g, int k, const Mat &batch, int pool, float lambda = 0.5f, int fill = HNSW_FILL_OHNSW) {
    const size_t cells = (size_t)batch.dim2 * (size_t)(k > 0 ? k : 0);
    Diverse out{std::vector<int32_t>(cells, -1), std::vector<float>(cells, 0.f), std::vector<float>(cells, 0.f), {}};
    check(hnsw_brute_force_batch_diverse(g.handle(), batch.data, batch.dim2, batch.dim1, k, pool, lambda, fill, out.ids.data(), out.dist.data(),
                                         out.div.data()));
    return out;
}

// The exact re-rank (hnsw_rerank_batch): for each query the k nearest of ITS candidates cand[q][0 .. cand_stride) (entries below
// id_base are padding) over the float32 vectors, under (distance, id), ascending -> (ids, distances), both [nq][k] (-1 / NaN past
// a query's real candidates).  What option "refine" does to the half-row searches' candidates.
inline std::pair<std::vector<int32_t>, std::vector<float>> rerank(const Hgraph &g, int k, const Mat &batch, const int32_t *cand, int cand_stride) {
    std::vector<int32_t> ids((size_t)batch.dim2 * (size_t)(k > 0 ? k : 0));
    std::vector<float> dist(ids.size());
    check(hnsw_rerank_batch(g.handle(), batch.data, batch.dim2, batch.dim1, cand, cand_stride, k, HNSW_FILL_OHNSW, ids.data(), dist.data()));
    return {std::move(ids), std::move(dist)};
}

// Ohnsw.distance_l2 a b (lib/ohnsw.ml:899), batched: out[q][j] = distance(batch[q], value ids[q][j])
inline std::vector<float> distance_l2(const Hgraph &g, const Mat &batch, const int32_t *ids, int m) {
    std::vector<float> out((size_t)batch.dim2 * m);
    check(hnsw_distance_batch(g.handle(), batch.data, batch.dim2, batch.dim1, ids, m, out.data()));
    return out;
}

} // namespace Ohnsw

namespace Ba {

// Hnsw.Ba.knn hgraph point ~num_neighbours_search ~num_neighbours (lib/hnsw.ml:763-767)
inline std::vector<value_distance> knn(const Hgraph &g, const float *point, int num_neighbours_search, int num_neighbours) {
    std::vector<int32_t> ids; std::vector<float> dist;
    detail::search(g, Mat{point, 1, g.dim()}, num_neighbours_search, num_neighbours, HNSW_FILL_BA, ids, dist, HNSW_SEM_FUNCTOR);
    std::vector<value_distance> out;
    for (int i = 0; i < num_neighbours && ids[(size_t)i] >= g.id_base(); ++i) out.push_back({ids[(size_t)i], dist[(size_t)i]});
    return out;
}

// Hnsw.Ba.knn_batch hgraph batch ~num_neighbours_search ~num_neighbours -> distances
// (lib/hnsw.ml:769-777): k x nq, +inf filled.
inline std::vector<float> knn_batch(const Hgraph &g, const Mat &batch, int num_neighbours_search, int num_neighbours) {
    std::vector<int32_t> ids; std::vector<float> dist;
    detail::search(g, batch, num_neighbours_search, num_neighbours, HNSW_FILL_BA, ids, dist, HNSW_SEM_FUNCTOR);
    return dist;
}

// Hnsw_algo.Search.search hgraph layer visited ~start_nodes target ~size_nearest (lib/hnsw_algo.ml:350-391)
inline std::vector<value_distance> search(const Hgraph &g, int layer, const std::vector<int64_t> &start_nodes,
                                          const float *target, int size_nearest) {
    return Ohnsw::search_k(g, layer, start_nodes, target, size_nearest, HNSW_SEM_FUNCTOR);
}

} // namespace Ba

// A batch in flight (hnsw_search_submit / hnsw_search_wait): wait() returns what knn_batch_bigarray would have.
class Pending {
public:
    Pending(const Hgraph &g, const Mat &batch, int ef, int k, int fill = HNSW_FILL_OHNSW, int sem = HNSW_SEM_OHNSW) : nq_(batch.dim2), k_(k) {
        hnsw_search_params p{ef, k, fill, sem};
        check(hnsw_search_submit(g.handle(), batch.data, batch.dim2, batch.dim1, &p, &r_));
    }
    Pending(const Pending &) = delete;
    Pending &operator=(const Pending &) = delete;
    Pending(Pending &&o) noexcept : r_(o.r_), nq_(o.nq_), k_(o.k_) { o.r_ = nullptr; }
    std::pair<std::vector<int32_t>, std::vector<float>> wait() {
        std::vector<int32_t> ids((size_t)nq_ * k_); std::vector<float> dist((size_t)nq_ * k_);
        hnsw_request *r = r_; r_ = nullptr;
        check(hnsw_search_wait(r, ids.data(), dist.data(), nullptr, nullptr));
        return {std::move(ids), std::move(dist)};
    }
private:
    hnsw_request *r_ = nullptr;
    int64_t nq_ = 0;
    int k_ = 0;
};

// One host process, several GPUs: the flattened graph replicated on every listed device, batches split
// into contiguous shards (hnsw_multi_*).
class MultiHgraph {
public:
    MultiHgraph(const hnsw_index_desc &desc, const std::vector<int32_t> &devices) : d_(desc.d) {
        check(hnsw_multi_create(&desc, devices.data(), (int32_t)devices.size(), &m_));
    }
    MultiHgraph(const MultiHgraph &) = delete;
    MultiHgraph &operator=(const MultiHgraph &) = delete;
    ~MultiHgraph() { if (m_) hnsw_multi_destroy(m_); }
    int num_replicas() const { int32_t c = 0; check(hnsw_multi_num_replicas(m_, &c)); return c; }

    // Ohnsw.knn_batch_bigarray over all replicas: ids and distances [nq][k]
    std::pair<std::vector<int32_t>, std::vector<float>> knn_batch_bigarray(int k, const Mat &batch, int ef = 0) const {
        std::vector<int32_t> ids((size_t)batch.dim2 * k, -1); std::vector<float> dist((size_t)batch.dim2 * k, 0.f);
        hnsw_search_params p{ef > 0 ? ef : k, k, HNSW_FILL_OHNSW, HNSW_SEM_OHNSW};
        check(hnsw_multi_search_batch(m_, batch.data, batch.dim2, batch.dim1, &p, ids.data(), dist.data(), nullptr, nullptr));
        return {std::move(ids), std::move(dist)};
    }

private:
    hnsw_multi *m_ = nullptr;
    int d_ = 0;
};

class Sharded;

// An allow-mask over the GLOBAL rows of one Sharded (hnsw_sharded_filter_create): allow[v] = global row v may be returned.  One
// ordinary filter per shard, cut on the host; never stale (shards cannot change).  Destroy it before its Sharded.
class ShardedFilter {
public:
    ShardedFilter(const Sharded &s, const std::vector<bool> &allow);
    ShardedFilter(const ShardedFilter &) = delete;
    ShardedFilter &operator=(const ShardedFilter &) = delete;
    ShardedFilter(ShardedFilter &&o) noexcept : f_(o.f_) { o.f_ = nullptr; }
    ~ShardedFilter() { if (f_) hnsw_sharded_filter_destroy(f_); }
    const hnsw_sharded_filter *handle() const { return f_; }
    int64_t count() const { int64_t c = 0; check(hnsw_sharded_filter_count(f_, &c)); return c; }   // the allowed rows of all shards
    // shard g's part (borrowed): an ordinary filter of that shard's handle
    const hnsw_filter *part(int g) const { const hnsw_filter *p = nullptr; check(hnsw_sharded_filter_part(f_, g, &p)); return p; }
private:
    hnsw_sharded_filter *f_ = nullptr;
};

// What a sharded range call and merge_segments return (hnsw_sharded_range_result): as RangeResult with int64 global ids, on the
// first device of its Sharded, which it outlives.
using ShardedRangeResultBase = RangeResultOf<int64_t, hnsw_sharded_range_result, hnsw_sharded_range_result_size, hnsw_sharded_range_result_fetch,
                                             hnsw_sharded_range_result_device, hnsw_sharded_range_result_destroy>;
class ShardedRangeResult : public ShardedRangeResultBase { using ShardedRangeResultBase::ShardedRangeResultBase; };

// One data set PARTITIONED over several GPUs (hnsw_sharded_*): shard g holds the rows [first_row(g), first_row(g + 1)) with a graph
// of its own on devices[g]; every query visits all shards and the per-shard answers are merged on devices[0] under (distance,
// global id).  Global ids are int64: first_row(g) + local node + id_base.
class Sharded {
public:
    struct Info { int64_t n; int32_t d, metric, id_base; int64_t device_bytes; };
    // hnsw_sharded_build: shard g = hnsw_build of the rows [floor(n g / G), floor(n (g + 1) / G)) with seed + g
    static Sharded build(const Mat &batch, const hnsw_build_params &params, const std::vector<int32_t> &devices) {
        Sharded s;
        check(hnsw_sharded_build(batch.data, batch.dim2, batch.dim1, batch.dim1, &params, devices.data(), (int32_t)devices.size(), &s.s_));
        return s;
    }
    // hnsw_sharded_create: one flattened graph with LOCAL ids per shard
    static Sharded create(const std::vector<const hnsw_index_desc *> &descs, const std::vector<int32_t> &devices) {
        if (descs.size() != devices.size()) throw std::invalid_argument("one device per shard");
        Sharded s;
        check(hnsw_sharded_create(descs.data(), devices.data(), (int32_t)devices.size(), &s.s_));
        return s;
    }
    // hnsw_sharded_load: one index file per shard (hnsw_index_save of every shard(g) writes them)
    static Sharded load(const std::vector<std::string> &paths, const std::vector<int32_t> &devices) {
        if (paths.size() != devices.size()) throw std::invalid_argument("one device per path");
        std::vector<const char *> p;
        for (const std::string &x : paths) p.push_back(x.c_str());
        Sharded s;
        check(hnsw_sharded_load(p.data(), devices.data(), (int32_t)devices.size(), &s.s_));
        return s;
    }
    Sharded(const Sharded &) = delete;
    Sharded &operator=(const Sharded &) = delete;
    Sharded(Sharded &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    ~Sharded() { if (s_) hnsw_sharded_destroy(s_); }
    hnsw_sharded *handle() const { return s_; }
    int num_shards() const { int32_t c = 0; check(hnsw_sharded_num_shards(s_, &c)); return c; }
    // shard g's handle (borrowed: read-only calls only) and the global row of its local node 0
    std::pair<hnsw_index *, int64_t> shard(int g) const {
        hnsw_index *h = nullptr; int64_t lo = 0;
        check(hnsw_sharded_shard(s_, g, &h, &lo));
        return {h, lo};
    }
    Info info() const {
        Info i{};
        check(hnsw_sharded_get_info(s_, &i.n, &i.d, &i.metric, &i.id_base, &i.device_bytes));
        return i;
    }
    void set_option(const char *name, int64_t value) { check(hnsw_sharded_set_option(s_, name, value)); }
    // hnsw_sharded_search_batch: ids (int64, global) and distances [nq][k]
    std::pair<std::vector<int64_t>, std::vector<float>> knn_batch(const Mat &batch, int ef, int k, int fill = HNSW_FILL_OHNSW,
                                                                  int sem = HNSW_SEM_OHNSW) const {
        std::vector<int64_t> ids((size_t)batch.dim2 * k, -1); std::vector<float> dist((size_t)batch.dim2 * k, 0.f);
        hnsw_search_params p{ef, k, fill, sem};
        check(hnsw_sharded_search_batch(s_, batch.data, batch.dim2, batch.dim1, &p, ids.data(), dist.data(), nullptr, nullptr));
        return {std::move(ids), std::move(dist)};
    }
    // hnsw_sharded_brute_force_batch: the exact k nearest of all rows
    std::pair<std::vector<int64_t>, std::vector<float>> brute_force_knn(int k, const Mat &batch, int fill = HNSW_FILL_OHNSW) const {
        std::vector<int64_t> ids((size_t)batch.dim2 * k, -1); std::vector<float> dist((size_t)batch.dim2 * k, 0.f);
        check(hnsw_sharded_brute_force_batch(s_, batch.data, batch.dim2, batch.dim1, k, fill, ids.data(), dist.data()));
        return {std::move(ids), std::move(dist)};
    }
    // hnsw_sharded_search_batch_filtered: the first k under (distance, global id) of the shards' own filtered rows; stage[q] = the
    // maximum over the shards (exact_stage as soon as one shard answered q from its exact scan)
    struct Filtered {
        static constexpr uint32_t exact_stage = 0xFFFFFFFFu;
        std::vector<int64_t> ids; std::vector<float> dist; std::vector<uint32_t> stage;
    };
    Filtered knn_filtered(const ShardedFilter &f, const Mat &batch, int ef, int k, int fill = HNSW_FILL_OHNSW, int sem = HNSW_SEM_OHNSW) const {
        const size_t nq = (size_t)batch.dim2, kk = (size_t)(k > 0 ? k : 0);
        Filtered out{std::vector<int64_t>(nq * kk, -1), std::vector<float>(nq * kk, 0.f), std::vector<uint32_t>(nq, 0u)};
        hnsw_search_params p{ef, k, fill, sem};
        check(hnsw_sharded_search_batch_filtered(s_, f.handle(), batch.data, batch.dim2, batch.dim1, &p, out.ids.data(), out.dist.data(), nullptr,
                                                 nullptr, out.stage.data()));
        return out;
    }
    // hnsw_sharded_range_search_batch / hnsw_sharded_range_brute_force_batch: per query the union of the shards' own segments under
    // (distance, global id); f (optional): under the shards' parts of a ShardedFilter
    ShardedRangeResult range_search(float radius, const Mat &batch, int ef = 64, int sem = HNSW_SEM_OHNSW, const ShardedFilter *f = nullptr) const {
        hnsw_range_params p{radius, ef, sem};
        hnsw_sharded_range_result *r = nullptr;
        check(hnsw_sharded_range_search_batch(s_, f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, &p, &r));
        return ShardedRangeResult(r);
    }
    ShardedRangeResult brute_force_range(float radius, const Mat &batch, const ShardedFilter *f = nullptr) const {
        hnsw_sharded_range_result *r = nullptr;
        check(hnsw_sharded_range_brute_force_batch(s_, f ? f->handle() : nullptr, batch.data, batch.dim2, batch.dim1, radius, &r));
        return ShardedRangeResult(r);
    }
private:
    Sharded() = default;
    hnsw_sharded *s_ = nullptr;
};

inline ShardedFilter::ShardedFilter(const Sharded &s, const std::vector<bool> &allow) {
    std::vector<uint32_t> bits((allow.size() + 31) / 32 + 1, 0u);
    for (size_t v = 0; v < allow.size(); ++v) if (allow[v]) bits[v >> 5] |= 1u << (v & 31);
    check(hnsw_sharded_filter_create(s.handle(), bits.data(), (int64_t)allow.size(), &f_));
}

// hnsw_merge_segments: n_lists range results over the same queries (lims[g]: nq + 1 entries from 0; ids[g] / dist[g]: lims[g][nq]
// entries, each segment ascending under (distance, id)) merged per query under (distance, first_row[list] + id); the same global id
// in two lists: the lower list first
inline ShardedRangeResult merge_segments(const std::vector<std::vector<int64_t>> &lims, const std::vector<std::vector<int32_t>> &ids,
                                         const std::vector<std::vector<float>> &dist, const std::vector<int64_t> &first_row, int id_base = 0,
                                         int device = 0) {
    const size_t n = lims.size();
    if (ids.size() != n || dist.size() != n || first_row.size() != n) throw std::invalid_argument("merge_segments: one lims, ids, dist and first_row per list");
    std::vector<const int64_t *> pl; std::vector<const int32_t *> pi; std::vector<const float *> pd;
    for (size_t g = 0; g < n; ++g) {
        if (lims[g].empty() || lims[g].size() != lims[0].size() || ids[g].size() != (size_t)lims[g].back() || dist[g].size() != ids[g].size())
            throw std::invalid_argument("merge_segments: lims[g] has nq + 1 entries, ids[g] and dist[g] lims[g][nq]");
        pl.push_back(lims[g].data()); pi.push_back(ids[g].data()); pd.push_back(dist[g].data());
    }
    hnsw_sharded_range_result *r = nullptr;
    check(hnsw_merge_segments(device, (int32_t)n, n ? (int64_t)lims[0].size() - 1 : 0, pl.data(), pi.data(), pd.data(), first_row.data(), id_base, &r));
    return ShardedRangeResult(r);
}

// hnsw_merge_lists: n_lists result lists per query (ids / dist [n_lists][nq][k_in], each ascending under (distance, id), padding
// below id_base at the end) merged under (distance, first_row[list] + id) into ids (int64) and distances [nq][k_out]
inline std::pair<std::vector<int64_t>, std::vector<float>> merge_lists(const std::vector<int32_t> &ids, const std::vector<float> &dist,
                                                                       const std::vector<int64_t> &first_row, int64_t nq, int k_in, int k_out,
                                                                       int id_base = 0, int fill = HNSW_FILL_OHNSW, int device = 0) {
    if (ids.size() != first_row.size() * (size_t)nq * (size_t)k_in || dist.size() != ids.size()) throw std::invalid_argument("merge_lists: ids and dist must be [n_lists][nq][k_in]");
    std::vector<int64_t> out((size_t)nq * k_out, -1); std::vector<float> od((size_t)nq * k_out, 0.f);
    check(hnsw_merge_lists(device, ids.data(), dist.data(), first_row.data(), (int32_t)first_row.size(), nq, k_in, k_out, id_base, fill,
                           out.data(), od.data()));
    return {std::move(out), std::move(od)};
}

} // namespace Hnsw
