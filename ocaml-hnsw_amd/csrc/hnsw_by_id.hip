// hnsw_by_id.hip -- search by stored item (the contract: include/hnsw_mi355x.h, the last section): the queries of a call are rows
// of the index, named by id or by key, and only the ids cross the link.  Every call here IS the public host call over the gathered
// rows (knn_host_call, filtered_host_call under the live mask, the exact scan): row formats, refine, COSINE's N(Q), the ladder, the
// ordering pre-pass and the tie-overflow repair are inherited, not restated.  What is new is the two ends of the call.
//
// Kernels (plain HIP).
//   gather_rows16_kernel   one 16-lane group per row, four rows per wave: out row j = the first `width` floats of the float32 row
//                          (tables.X, always resident) of node ids[j] - id_base, zeros where that is no node.  VEC: out is 16-byte
//                          aligned and its stride a multiple of four floats -- whole chunks move as one dwordx4 (the table's rows
//                          always allow it); otherwise value by value, the split of cosine_normalise_kernel.  No division anywhere.
//   drop_self_kernel       one wave per result row over the inner [nq][k + 1] ids and distances where the search left them: p by
//                          one ballot per 64-entry pass (k + 1 <= 1024: at most 16), then the row with position p deleted
//                          (drop_self_source, hnsw_by_id_plan.h) as ids, or as the index's keys in the same pass
//                          (keys_translate_kernel's rule), into the handle's scratch or straight into page-locked host matrices.
#include "hnsw_internal.h"

namespace hnsw_dev {

constexpr int GATHER_WAVES = 4;
constexpr int GATHER_ROWS = 4 * GATHER_WAVES;    // rows per workgroup
constexpr int DROP_WAVES = 4;                    // result rows per workgroup

template <bool VEC>
__global__ void __launch_bounds__(64 * GATHER_WAVES)
gather_rows16_kernel(const float *X, int64_t n, int64_t stride, int32_t id_base, const int32_t *ids, int64_t m, int32_t width, float *out,
                     int64_t out_stride) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * GATHER_ROWS + (threadIdx.x >> 4);
    if (row >= m) return;
    const int64_t v = (int64_t)ids[row] - id_base;
    const bool node = v >= 0 && v < n;            // (uniform over the group: a row that is no node is never read)
    const float *src = X + (node ? v : 0) * stride;
    float *dst = out + row * out_stride;
    if (VEC) {
        for (int e0 = 4 * l16; e0 < width; e0 += 64) {
            if (e0 + 4 <= width) {
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (node) x = *reinterpret_cast<const float4 *>(src + e0);
                *reinterpret_cast<float4 *>(dst + e0) = x;
            } else {
                for (int e = e0; e < width; ++e) dst[e] = node ? src[e] : 0.f;
            }
        }
    } else {
        for (int e = l16; e < width; e += 16) dst[e] = node ? src[e] : 0.f;
    }
}

// Id: int32_t -- the ids as they are; int64_t -- the key of each id, `missing` where the id is no node (the search's fill id)
template <class Id>
__global__ void __launch_bounds__(64 * DROP_WAVES)
drop_self_kernel(const int32_t *ids, const float *dist, const int32_t *self, int64_t nq, int32_t k, Id *out_ids, float *out_dist,
                 const int64_t *key_of, int64_t n, int32_t id_base, int64_t missing) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * DROP_WAVES + (threadIdx.x >> 6);
    if (row >= nq) return;                        // (a whole wave leaves)
    const int32_t *r = ids + row * ((int64_t)k + 1);
    const float *rd = dist + row * ((int64_t)k + 1);
    const int32_t me = self[row];
    int32_t p = k;                                // the smallest j in [0, k] with r[j] == me, else k
    for (int32_t j0 = 0; j0 <= k; j0 += 64) {
        const int32_t j = j0 + lane;
        const unsigned long long hits = __ballot(j <= k && r[j] == me);
        if (hits) { p = j0 + __ffsll((long long)hits) - 1; break; }     // (hits is the wave's: every lane leaves together)
    }
    for (int32_t j = lane; j < k; j += 64) {
        const int32_t s = hnsw_host::drop_self_source(j, p);
        const int32_t id = r[s];
        out_dist[row * k + j] = rd[s];
        if constexpr (sizeof(Id) == 8) {
            const int64_t v = (int64_t)id - id_base;
            out_ids[row * k + j] = v >= 0 && v < n ? key_of[v] : missing;
        } else
            out_ids[row * k + j] = id;
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

int gather_rows(const hnsw_index *idx, const int32_t *d_ids, int64_t m, int32_t width, float *d_out, int64_t out_stride, hipStream_t st) {
    if (m <= 0) return HNSW_OK;
    if (width < 1 || width > idx->iv.stride || out_stride < width) return fail(HNSW_ERR_BAD_ARG, "gather: %d floats of a row of %lld", width, (long long)idx->iv.stride);
    // (the table's rows start 64-byte aligned: only the output decides)
    const bool vec = out_stride % 4 == 0 && (uintptr_t)d_out % 16 == 0;
    const dim3 grid((unsigned)((m + hnsw_dev::GATHER_ROWS - 1) / hnsw_dev::GATHER_ROWS)), block(64 * hnsw_dev::GATHER_WAVES);
    const float *X = (const float *)idx->tables.X.p;
    if (vec) hipLaunchKernelGGL(hnsw_dev::gather_rows16_kernel<true>, grid, block, 0, st, X, idx->iv.n, idx->iv.stride, idx->iv.id_base, d_ids, m, width, d_out, out_stride);
    else hipLaunchKernelGGL(hnsw_dev::gather_rows16_kernel<false>, grid, block, 0, st, X, idx->iv.n, idx->iv.stride, idx->iv.id_base, d_ids, m, width, d_out, out_stride);
    return launched("gather rows kernel");
}

int drop_self_rows(const hnsw_index *idx, const int32_t *d_ids, const float *d_dist, const int32_t *d_self, int64_t nq, int32_t k,
                   int32_t *out_ids, int64_t *out_keys, int64_t missing, float *out_dist, hipStream_t st) {
    if (nq <= 0) return HNSW_OK;
    if (!drop_self_k_ok(k) || (!out_ids && !out_keys) || !out_dist) return fail(HNSW_ERR_BAD_ARG, "drop self: k=%d or a null output", k);
    const dim3 grid((unsigned)((nq + hnsw_dev::DROP_WAVES - 1) / hnsw_dev::DROP_WAVES)), block(64 * hnsw_dev::DROP_WAVES);
    if (out_keys) {
        const KeyTables &kt = *idx->keys;
        hipLaunchKernelGGL(hnsw_dev::drop_self_kernel<int64_t>, grid, block, 0, st, d_ids, d_dist, d_self, nq, k, out_keys, out_dist,
                           (const int64_t *)kt.key_of.p, kt.n, idx->iv.id_base, missing);
    } else
        hipLaunchKernelGGL(hnsw_dev::drop_self_kernel<int32_t>, grid, block, 0, st, d_ids, d_dist, d_self, nq, k, out_ids, out_dist,
                           (const int64_t *)nullptr, (int64_t)0, idx->iv.id_base, (int64_t)0);
    return launched("drop self kernel");
}

} // namespace hnsw_host

using namespace hnsw_host;

namespace {

// what every call by id checks before the search's own checks: the handle, exclude_self, and that P exists (*inner: the params the
// public call runs with -- the caller's, or P = {max(ef, k + 1), k + 1, fill, semantics})
int check_exclude(const hnsw_index *idx, int32_t exclude_self, int32_t k, int32_t semantics, const char *call) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (exclude_self != 0 && exclude_self != 1) return fail(HNSW_ERR_BAD_ARG, "%s: exclude_self must be 0 or 1 (exclude_self=%d)", call, exclude_self);
    if (!exclude_self) return HNSW_OK;
    if (semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "%s: exclude_self = 1 with HNSW_SEM_FUNCTOR_NEAREST_K: the k farthest of a W one wider have no meaning", call);
    if (k >= 1 && !drop_self_k_ok(k)) return fail(HNSW_ERR_UNSUPPORTED, "%s: exclude_self = 1 searches k + 1 wide and k + 1 = %lld > 1024 is not supported", call, (long long)k + 1);
    return HNSW_OK;
}

// the ids of a call: each in [id_base, id_base + n), else HNSW_ERR_BAD_ARG naming the first by position
int check_ids(const hnsw_index *idx, const int32_t *ids, int64_t nq, const char *call) {
    const int64_t lo = idx->iv.id_base, hi = lo + idx->iv.n;
    for (int64_t i = 0; i < nq; ++i)
        if (ids[i] < lo || ids[i] >= hi)
            return fail(HNSW_ERR_BAD_ARG, "%s: ids[%lld]=%d is out of range (the first by position): nothing written", call, (long long)i, ids[i]);
    return HNSW_OK;
}

// hnsw_search_batch_by_id and, ko not null, the tail of hnsw_search_batch_by_key: ids are host ids not yet checked
int search_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, const hnsw_search_params *params, int32_t exclude_self, int32_t *out_ids,
                 float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, const KeysOut *ko, const char *call) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!params) return fail(HNSW_ERR_BAD_ARG, "null params");
    int rc = check_exclude(idx, exclude_self, params->k, params->semantics, call);
    if (rc) return rc;
    hnsw_search_params p = *params;
    if (exclude_self && p.k >= 1) { p.ef = drop_self_inner_ef(params->ef, params->k); p.k = drop_self_inner_k(params->k); }
    const int64_t q_stride = padded_stride(idx->iv.d);
    if ((rc = check_batch(idx, &p, nq, q_stride, ids && (ko ? ko->keys != nullptr : out_ids != nullptr) && out_dist)) || nq == 0) return rc;
    if ((rc = check_ids(idx, ids, nq, call))) return rc;
    const RowsIn rows{ids, exclude_self == 1};
    return knn_host_call(idx, nullptr, nq, q_stride, &p, out_ids, out_dist, out_ndist, out_nhops, nullptr, ko, &rows);
}

// hnsw_brute_force_batch_by_id for ids already checked: hnsw_brute_force_batch over the gathered rows, k + 1 wide and through the
// epilogue when exclude_self
int scan_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, int32_t k, int32_t fill, int32_t exclude_self, int32_t *out_ids, float *out_dist) {
    HIP_TRY(hipSetDevice(idx->device));
    const int32_t kin = exclude_self ? drop_self_inner_k(k) : k;
    const RowsIn rows{ids, exclude_self == 1};
    HostCall c;
    c.rows = &rows;
    int rc;
    if ((rc = c.begin(idx, nullptr, nq, padded_stride(idx->iv.d), kin, out_ids, out_dist, nullptr, nullptr, false))) return rc;
    const hnsw_filter *const live = live_filter(idx);
    rc = scan_search(idx, c.b, kin, fill, idx->hs[0], live ? live->table() : nullptr);
    if (rc) { (void)hipStreamSynchronize(idx->hs[0]); return rc; }
    return c.finish(idx, "scan", idx->hs[0]);
}

int check_scan_by_id(const hnsw_index *idx, const int32_t *ids, int64_t nq, int32_t k, int32_t fill, int32_t exclude_self, bool outputs, const char *call) {
    int rc = check_exclude(idx, exclude_self, k, HNSW_SEM_OHNSW, call);
    if (rc) return rc;
    return check_scan(idx, nq, padded_stride(idx->iv.d), exclude_self && k >= 1 ? drop_self_inner_k(k) : k, fill, ids && outputs);
}

} // namespace

extern "C" {

int32_t hnsw_index_get_rows_device(hnsw_index *idx, const int32_t *d_ids, int64_t m, float *d_out, int64_t out_stride, void *stream) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0 || m > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "m=%lld out of range", (long long)m);
    if (m == 0) return HNSW_OK;
    if (!d_ids || !d_out) return fail(HNSW_ERR_BAD_ARG, "null d_ids or null d_out");
    if (out_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "out_stride < d");
    HIP_TRY(hipSetDevice(idx->device));
    return gather_rows(idx, d_ids, m, idx->iv.d, d_out, out_stride, (hipStream_t)stream);
}

int32_t hnsw_search_batch_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, const hnsw_search_params *params, int32_t exclude_self,
                                int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops) {
    return search_by_id(idx, ids, nq, params, exclude_self, out_ids, out_dist, out_ndist, out_nhops, nullptr, "hnsw_search_batch_by_id");
}

int32_t hnsw_search_batch_by_key(hnsw_index *idx, const int64_t *keys, int64_t nq, const hnsw_search_params *params, int32_t exclude_self,
                                 int64_t missing_key, int64_t *out_keys, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops) {
    const char *const call = "hnsw_search_batch_by_key";
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "%s: the index has no keys (hnsw_index_set_keys)", call);
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    const KeysOut ko{out_keys, missing_key};
    // (nothing to look up: the by-id call's checks and its no-op)
    if (nq == 0 || !keys) return search_by_id(idx, nullptr, nq, params, exclude_self, nullptr, out_dist, out_ndist, out_nhops, &ko, call);
    std::vector<int32_t> nodes;
    int rc = keys_find_nodes(idx, keys, nq, nodes);
    if (rc) return rc;
    for (int64_t i = 0; i < nq; ++i) {
        if (nodes[(size_t)i] < 0)
            return fail(HNSW_ERR_BAD_ARG, "%s: keys[%lld]=%lld is not a stored key (the first by position): nothing written", call, (long long)i, (long long)keys[i]);
        nodes[(size_t)i] += idx->iv.id_base;
    }
    return search_by_id(idx, nodes.data(), nq, params, exclude_self, nullptr, out_dist, out_ndist, out_nhops, &ko, call);
}

int32_t hnsw_brute_force_batch_by_id(hnsw_index *idx, const int32_t *ids, int64_t nq, int32_t k, int32_t fill, int32_t exclude_self,
                                     int32_t *out_ids, float *out_dist) {
    const char *const call = "hnsw_brute_force_batch_by_id";
    int rc = check_scan_by_id(idx, ids, nq, k, fill, exclude_self, out_ids && out_dist, call);
    if (rc || nq == 0) return rc;
    if ((rc = check_ids(idx, ids, nq, call))) return rc;
    return scan_by_id(idx, ids, nq, k, fill, exclude_self, out_ids, out_dist);
}

int32_t hnsw_knn_graph(hnsw_index *idx, const hnsw_search_params *params, int32_t exact, int32_t *out_ids, float *out_dist) {
    const char *const call = "hnsw_knn_graph";
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!params) return fail(HNSW_ERR_BAD_ARG, "null params");
    if (exact != 0 && exact != 1) return fail(HNSW_ERR_BAD_ARG, "%s: exact must be 0 or 1 (exact=%d)", call, exact);
    const int64_t n = idx->iv.n, chunk = idx->graph_chunk_rows;
    if (n == 0) return HNSW_OK;
    if (!out_ids) return fail(HNSW_ERR_BAD_ARG, "null out_ids");
    const int32_t k = params->k;
    // (the inner call's own checks of the params, on an empty batch: nothing below is sized by a k they refuse)
    int rc = exact ? hnsw_brute_force_batch_by_id(idx, nullptr, 0, k, params->fill, 1, nullptr, nullptr)
                   : search_by_id(idx, nullptr, 0, params, 1, nullptr, nullptr, nullptr, nullptr, nullptr, call);
    if (rc) return rc;
    // row v is the row of the by-id call for id_base + v with exclude_self = 1: one such call per chunk of nodes, so that the
    // handle's scratch is a chunk's; the distances of a caller who wants none go to a chunk-sized block of ours
    std::vector<int32_t> ids((size_t)std::min(n, chunk));
    std::vector<float> dist;
    if (!out_dist) dist.resize(ids.size() * (size_t)k);
    for (int64_t c = 0; c < graph_chunks(n, chunk); ++c) {
        int64_t v0, m;
        graph_chunk(n, chunk, c, &v0, &m);
        for (int64_t j = 0; j < m; ++j) ids[(size_t)j] = (int32_t)(idx->iv.id_base + v0 + j);
        int32_t *const oi = out_ids + v0 * k;
        float *const od = out_dist ? out_dist + v0 * k : dist.data();
        rc = exact ? hnsw_brute_force_batch_by_id(idx, ids.data(), m, k, params->fill, 1, oi, od)
                   : search_by_id(idx, ids.data(), m, params, 1, oi, od, nullptr, nullptr, nullptr, call);
        if (rc) return rc;
    }
    return HNSW_OK;
}

} // extern "C"
