// hnsw_keys.hip -- stable 64-bit keys the index owns (the contract: include/hnsw_mi355x.h).  A keyed handle holds two device tables
// (KeyTables, hnsw_internal.h): key_of, the key of node v in row order, and the lookup table, the n pairs (key, node) in ascending
// SIGNED key order (hipcub::DeviceRadixSort::SortPairs over int64_t keys, whose bit twiddling gives the signed order; keys_dup_kernel
// checks the order it got as well).  Keys are distinct, so that table is unique; it is rebuilt from key_of, never patched, whenever
// key_of changes: hnsw_index_set_keys, and adopt_graph (renumbered_keys), which moves the keys with their nodes through
// hnsw_index_insert_keyed, hnsw_index_remove and hnsw_index_compact before the swap.  Nothing depends on an atomic arrival order.
//
// Kernels (plain HIP, one lane per entry).
//   keys_iota_kernel        node[i] = i: the values the sort carries beside the keys.
//   keys_dup_kernel         over the sorted keys: position i flags sorted[i] == sorted[i + 1] and offers the key to a min-reduction
//                           (atomicMin over the keys with the sign bit flipped: unsigned order = signed order), so the duplicate
//                           that is reported is the smallest, not the first to arrive; sorted[i] > sorted[i + 1] sets a second flag.
//   keys_find_kernel        one lane per looked-up key: binary search of the sorted keys (keys_position, hnsw_keys_plan.h: signed
//                           compares, 64-bit bounds, no lo + hi), writes the node or -1.
//   keys_translate_kernel   one lane per result entry: out[i] = 0 <= ids[i] - id_base < n ? key_of[ids[i] - id_base] : missing.
//                           The tail of every keyed search: nq k ids read, as many 8-byte stores, the gather from key_of (8 n bytes,
//                           L2-resident at 1 M nodes).
//   keys_renumber_kernel    new_key_of[new_id[v]] = key_of[v] for every surviving v; the lanes past n_old write the keys an upsert
//                           appends behind the survivors (new_key_of[kept + i] = append[i]): one launch for both.
//   keys_allow_kernel       sets the mask bits of a list of nodes (hnsw_filter_create_by_keys), as mark_bits_kernel does.
#include "hnsw_internal.h"

#include <hipcub/hipcub.hpp>

namespace hnsw_dev {

constexpr unsigned long long KEY_SIGN = 0x8000000000000000ull;

__global__ void __launch_bounds__(256)
keys_iota_kernel(int32_t *node, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) node[i] = (int32_t)i;
}

// out[0]: the smallest duplicated key, sign bit flipped (the caller sets all ones); flags: bit 0 a duplicate, bit 1 a descent
__global__ void __launch_bounds__(256)
keys_dup_kernel(const int64_t *sorted, int64_t n, unsigned long long *out, uint32_t *flags) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = sorted[i], b = sorted[i + 1];
        if (a == b) {
            atomicMin(out, (unsigned long long)a ^ KEY_SIGN);
            atomicOr(flags, 1u);
        } else if (a > b)
            atomicOr(flags, 2u);
    }
}

__global__ void __launch_bounds__(256)
keys_find_kernel(const int64_t *sorted, const int32_t *node, int64_t n, const int64_t *keys, int64_t m, int32_t *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pos = hnsw_host::keys_position(sorted, n, keys[i]);
        out[i] = pos < 0 ? -1 : node[pos];
    }
}

__global__ void __launch_bounds__(256)
keys_translate_kernel(const int64_t *key_of, int64_t n, int32_t id_base, const int32_t *ids, int64_t m, int64_t missing, int64_t *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = (int64_t)ids[i] - id_base;
        out[i] = v >= 0 && v < n ? key_of[v] : missing;
    }
}

__global__ void __launch_bounds__(256)
keys_renumber_kernel(const int64_t *key_of, const int32_t *new_id, int64_t n_old, int64_t n_new, int64_t *out, const int64_t *append,
                     int64_t kept, int64_t n_append) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_old + n_append; v += (int64_t)gridDim.x * blockDim.x) {
        if (v < n_old) {
            const int64_t j = new_id[v];        // 0-based, -1 = removed; survivors map one to one onto [0, kept), kept <= n_new
            if (j >= 0 && j < n_new) out[j] = key_of[v];
        } else {
            const int64_t j = kept + (v - n_old);       // the appended keys, behind the survivors (kept + n_append == n_new: the host)
            if (j < n_new) out[j] = append[v - n_old];
        }
    }
}

__global__ void __launch_bounds__(256)
keys_allow_kernel(uint32_t *mask, const int32_t *nodes, int64_t m) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = nodes[i];             // 0-based, found by keys_find_kernel: 0 <= v < n (checked on the host)
        atomicOr(mask + (v >> 5), 1u << (v & 31));
    }
}

} // namespace hnsw_dev

using namespace hnsw_host;

namespace {

// the blocks of a one-lane-per-entry launch over m entries (the kernels stride over what is left)
unsigned blocks_for(int64_t m) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, 65536)); }

// kt.key_of holds kt.n keys: the lookup table made from them on the null stream, waited for.  HNSW_ERR_BAD_ARG "<what>: ..." naming
// the smallest duplicated key when two nodes have one key.
int build_lookup(KeyTables &kt, const char *what) {
    const int64_t n = kt.n;
    hipError_t e = kt.sorted.alloc((size_t)n * 8);
    if (e == hipSuccess) e = kt.node.alloc((size_t)n * 4);
    if (e != hipSuccess) return hip_fail(e, "key lookup table allocation");
    if (n == 0) return HNSW_OK;
    DevBuf iota, temp, verdict;
    int rc;
    if ((rc = iota.ensure((size_t)n * 4)) || (rc = verdict.ensure(16))) return rc;
    hipLaunchKernelGGL(hnsw_dev::keys_iota_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, (int32_t *)iota.p, n);
    if ((rc = launched("keys iota kernel"))) return rc;
    size_t bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int64_t *)kt.key_of.p, (int64_t *)kt.sorted.p, (const int32_t *)iota.p,
                                               (int32_t *)kt.node.p, (int)n, 0, 64, nullptr));
    if ((rc = temp.ensure(std::max<size_t>(bytes, 16)))) return rc;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, bytes, (const int64_t *)kt.key_of.p, (int64_t *)kt.sorted.p, (const int32_t *)iota.p,
                                               (int32_t *)kt.node.p, (int)n, 0, 64, nullptr));
    const unsigned long long init[2] = {~0ull, 0ull};
    unsigned long long got[2] = {0, 0};
    HIP_TRY(hipMemcpy(verdict.p, init, 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hnsw_dev::keys_dup_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, (const int64_t *)kt.sorted.p, n,
                       (unsigned long long *)verdict.p, (uint32_t *)((char *)verdict.p + 8));
    if ((rc = launched("keys dup kernel"))) return rc;
    HIP_TRY(hipMemcpy(got, verdict.p, 16, hipMemcpyDeviceToHost));
    const uint32_t flags = (uint32_t)got[1];
    if (flags & 2u) return fail(HNSW_ERR_HIP, "%s: the sorted keys are not in ascending signed order", what);
    if (flags & 1u)
        return fail(HNSW_ERR_BAD_ARG, "%s: keys must be pairwise distinct: key %lld is the smallest duplicated key", what,
                    (long long)(int64_t)(got[0] ^ hnsw_dev::KEY_SIGN));
    return HNSW_OK;
}

// the 0-based nodes of m keys (host arrays; -1: no node has the key), through keys_find_kernel
int find_nodes(const hnsw_index *idx, const int64_t *keys, int64_t m, std::vector<int32_t> &nodes) {
    nodes.assign((size_t)m, -1);
    if (m == 0) return HNSW_OK;
    const KeyTables &kt = *idx->keys;
    HIP_TRY(hipSetDevice(idx->device));
    DevBuf d_keys, d_nodes;
    int rc;
    if ((rc = d_keys.ensure((size_t)m * 8)) || (rc = d_nodes.ensure((size_t)m * 4))) return rc;
    HIP_TRY(hipMemcpy(d_keys.p, keys, (size_t)m * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hnsw_dev::keys_find_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, (const int64_t *)kt.sorted.p,
                       (const int32_t *)kt.node.p, kt.n, (const int64_t *)d_keys.p, m, (int32_t *)d_nodes.p);
    if ((rc = launched("keys find kernel"))) return rc;
    HIP_TRY(hipMemcpy(nodes.data(), d_nodes.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

// what the calls "by key" check first: a keyed handle and a list; then the list's ids (id_base-based), every key present --
// else HNSW_ERR_BAD_ARG naming the first absent key by position
int ids_of_keys(const hnsw_index *idx, const int64_t *keys, int64_t m, const char *call, std::vector<int64_t> &ids, std::vector<int32_t> *nodes_out = nullptr) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "%s: the index has no keys (hnsw_index_set_keys)", call);
    if (m > 0 && !keys) return fail(HNSW_ERR_BAD_ARG, "null keys");
    std::vector<int32_t> nodes;
    const int rc = find_nodes(idx, keys, m, nodes);
    if (rc) return rc;
    ids.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        if (nodes[(size_t)i] < 0)
            return fail(HNSW_ERR_BAD_ARG, "%s: keys[%lld]=%lld is not a stored key: nothing changed", call, (long long)i, (long long)keys[i]);
        ids[(size_t)i] = (int64_t)nodes[(size_t)i] + idx->iv.id_base;
    }
    if (nodes_out) *nodes_out = std::move(nodes);
    return HNSW_OK;
}

} // namespace

namespace hnsw_host {

int renumbered_keys(const hnsw_index *idx, const int32_t *new_id, int64_t n_new, const int64_t *append_keys, std::unique_ptr<KeyTables> &out) {
    out.reset();
    if (!idx->keys && !append_keys) return HNSW_OK;
    const int64_t n_old = idx->iv.n, kept = idx->keys ? n_old : 0;
    if (!new_id && (n_new < kept || (n_new > kept && !append_keys)))
        return fail(HNSW_ERR_BAD_ARG, "a keyed index must never hold a node without a key (%lld nodes, %lld keys)", (long long)n_new, (long long)kept);
    std::unique_ptr<KeyTables> kt(new KeyTables());
    kt->n = n_new;
    const hipError_t e = kt->key_of.alloc((size_t)n_new * 8);
    if (e != hipSuccess) return hip_fail(e, "key table allocation");
    int rc;
    if (new_id) {
        // the survivors keep their keys under new_id; append_keys (the upsert: both at once) go behind them in the same launch
        const int64_t n_have = kept;                    // nodes that have a key to carry: none on a handle without keys
        int64_t survivors = 0;
        for (int64_t v = 0; v < n_have; ++v) survivors += new_id[v] >= 0;
        const int64_t n_append = append_keys ? n_new - survivors : 0;
        if (survivors + n_append != n_new || n_append < 0)
            return fail(HNSW_ERR_BAD_ARG, "a keyed index must never hold a node without a key (%lld nodes, %lld keys)", (long long)n_new,
                        (long long)(survivors + std::max<int64_t>(n_append, 0)));
        if (n_new > 0) {
            DevBuf d_new, d_app;
            if ((rc = d_new.ensure((size_t)std::max<int64_t>(n_have, 1) * 4)) || (rc = d_app.ensure((size_t)std::max<int64_t>(n_append, 1) * 8))) return rc;
            if (n_have > 0) HIP_TRY(hipMemcpy(d_new.p, new_id, (size_t)n_have * 4, hipMemcpyHostToDevice));
            if (n_append > 0) HIP_TRY(hipMemcpy(d_app.p, append_keys, (size_t)n_append * 8, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(hnsw_dev::keys_renumber_kernel, dim3(blocks_for(n_have + n_append)), dim3(256), 0, nullptr,
                               n_have > 0 ? (const int64_t *)idx->keys->key_of.p : nullptr, (const int32_t *)d_new.p, n_have, n_new,
                               (int64_t *)kt->key_of.p, (const int64_t *)d_app.p, survivors, n_append);
            if ((rc = launched("keys renumber kernel"))) return rc;
            HIP_TRY(hipDeviceSynchronize());        // (d_new and d_app are freed on return)
        }
    } else {
        if (kept > 0) HIP_TRY(hipMemcpy(kt->key_of.p, idx->keys->key_of.p, (size_t)kept * 8, hipMemcpyDeviceToDevice));
        if (n_new > kept) HIP_TRY(hipMemcpy((int64_t *)kt->key_of.p + kept, append_keys, (size_t)(n_new - kept) * 8, hipMemcpyHostToDevice));
    }
    if ((rc = build_lookup(*kt, "keys"))) return rc;
    out = std::move(kt);
    return HNSW_OK;
}

int keys_find_nodes(const hnsw_index *idx, const int64_t *keys, int64_t m, std::vector<int32_t> &nodes) { return find_nodes(idx, keys, m, nodes); }

int keys_translate(const hnsw_index *idx, const int32_t *d_ids, int64_t m, int64_t missing, int64_t *d_out, hipStream_t st) {
    if (m <= 0) return HNSW_OK;
    const KeyTables &kt = *idx->keys;
    hipLaunchKernelGGL(hnsw_dev::keys_translate_kernel, dim3(blocks_for(m)), dim3(256), 0, st, (const int64_t *)kt.key_of.p, kt.n, idx->iv.id_base,
                       d_ids, m, missing, d_out);
    return launched("keys translate kernel");
}

} // namespace hnsw_host

extern "C" {

int32_t hnsw_index_set_keys(hnsw_index *idx, const int64_t *keys, int64_t n) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (n != idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "%lld keys, the index has %lld nodes", (long long)n, (long long)idx->iv.n);
    if (n > 0 && !keys) return fail(HNSW_ERR_BAD_ARG, "null keys");
    if (idx->multi_replica) return fail(HNSW_ERR_BAD_ARG, "the index is a replica of an hnsw_multi or a shard of an hnsw_sharded: keys for those are not built");
    HIP_TRY(hipSetDevice(idx->device));
    // the new tables, complete before the handle's are touched: on any error it keeps the keys it had, or none
    std::unique_ptr<KeyTables> kt(new KeyTables());
    kt->n = n;
    const hipError_t e = kt->key_of.alloc((size_t)n * 8);
    if (e != hipSuccess) return hip_fail(e, "key table allocation");
    if (n > 0) HIP_TRY(hipMemcpy(kt->key_of.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    int rc;
    if ((rc = build_lookup(*kt, "hnsw_index_set_keys"))) { kt.reset(); (void)hipGetLastError(); return rc; }
    HIP_TRY(hipDeviceSynchronize());            // (hnsw_index_keys_of_device calls in flight on caller streams read the old table)
    idx->keys = std::move(kt);
    return HNSW_OK;
}

int32_t hnsw_index_clear_keys(hnsw_index *idx) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!idx->keys) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipDeviceSynchronize());
    idx->keys.reset();
    idx->key_scratch.release();
    return HNSW_OK;
}

int32_t hnsw_index_keys_info(const hnsw_index *idx, int32_t *has_keys, int64_t *bytes) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (has_keys) *has_keys = idx->keys ? 1 : 0;
    if (bytes) *bytes = idx->keys ? (int64_t)idx->keys->bytes() : 0;
    return HNSW_OK;
}

int32_t hnsw_index_keys_of(const hnsw_index *idx, const int32_t *ids, int64_t m, int64_t missing_key, int64_t *out) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "hnsw_index_keys_of: the index has no keys (hnsw_index_set_keys)");
    if (!ids && m != idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "null ids ask for all %lld rows in order: m=%lld", (long long)idx->iv.n, (long long)m);
    if (m == 0) return HNSW_OK;
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    HIP_TRY(hipSetDevice(idx->device));
    if (!ids) {
        HIP_TRY(hipMemcpy(out, idx->keys->key_of.p, (size_t)m * 8, hipMemcpyDeviceToHost));
        return HNSW_OK;
    }
    DevBuf d_ids, d_out;
    int rc;
    if ((rc = d_ids.ensure((size_t)m * 4)) || (rc = d_out.ensure((size_t)m * 8))) return rc;
    HIP_TRY(hipMemcpy(d_ids.p, ids, (size_t)m * 4, hipMemcpyHostToDevice));
    if ((rc = keys_translate(idx, (const int32_t *)d_ids.p, m, missing_key, (int64_t *)d_out.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)m * 8, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

int32_t hnsw_index_keys_of_device(hnsw_index *idx, const int32_t *d_ids, int64_t m, int64_t missing_key, int64_t *d_out, void *stream) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "hnsw_index_keys_of_device: the index has no keys (hnsw_index_set_keys)");
    if (m == 0) return HNSW_OK;
    if (!d_ids || !d_out) return fail(HNSW_ERR_BAD_ARG, "null d_ids or null d_out");
    HIP_TRY(hipSetDevice(idx->device));
    return keys_translate(idx, d_ids, m, missing_key, d_out, (hipStream_t)stream);
}

int32_t hnsw_index_find_keys(const hnsw_index *idx, const int64_t *keys, int64_t m, int64_t *out_ids) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "hnsw_index_find_keys: the index has no keys (hnsw_index_set_keys)");
    if (m == 0) return HNSW_OK;
    if (!keys || !out_ids) return fail(HNSW_ERR_BAD_ARG, "null keys or null out_ids");
    std::vector<int32_t> nodes;
    const int rc = find_nodes(idx, keys, m, nodes);
    if (rc) return rc;
    for (int64_t i = 0; i < m; ++i) out_ids[i] = (int64_t)nodes[(size_t)i] + idx->iv.id_base;        // absent: id_base - 1
    return HNSW_OK;
}

int32_t hnsw_search_batch_keyed(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                const hnsw_search_params *params, int64_t missing_key, int64_t *out_keys, float *out_dist,
                                uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!idx->keys) return fail(HNSW_ERR_BAD_ARG, "hnsw_search_batch_keyed: the index has no keys (hnsw_index_set_keys)");
    const KeysOut ko{out_keys, missing_key};
    if (f) return filtered_host_call(idx, f, queries, nq, q_stride, params, nullptr, out_dist, out_ndist, out_nhops, out_stage, &ko);
    return knn_host_call(idx, queries, nq, q_stride, params, nullptr, out_dist, out_ndist, out_nhops, out_stage, &ko);
}

int32_t hnsw_index_insert_keyed(hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const int64_t *keys,
                                const hnsw_build_params *params) {
    if (!idx || !params) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys && idx->iv.n > 0)
        return fail(HNSW_ERR_BAD_ARG, "hnsw_index_insert_keyed: the index has %lld nodes and no keys (hnsw_index_set_keys first)", (long long)idx->iv.n);
    if (m == 0) return HNSW_OK;
    if (!keys) return fail(HNSW_ERR_BAD_ARG, "null keys");
    // refused before anything is built: two equal keys in the call (the smallest such key), a key that is stored (the first by position)
    std::vector<int64_t> sorted(keys, keys + m);
    std::sort(sorted.begin(), sorted.end());
    int64_t dup = 0;
    if (smallest_duplicate(sorted.data(), m, &dup))
        return fail(HNSW_ERR_BAD_ARG, "hnsw_index_insert_keyed: key %lld appears twice in the call (the smallest duplicated key): nothing inserted", (long long)dup);
    if (idx->keys) {
        std::vector<int32_t> nodes;
        const int rc = find_nodes(idx, keys, m, nodes);
        if (rc) return rc;
        for (int64_t i = 0; i < m; ++i)
            if (nodes[(size_t)i] >= 0)
                return fail(HNSW_ERR_BAD_ARG, "hnsw_index_insert_keyed: keys[%lld]=%lld is a stored key already (node %lld): nothing inserted", (long long)i,
                            (long long)keys[i], (long long)nodes[(size_t)i] + idx->iv.id_base);
    }
    return insert_vectors(idx, vectors, m, row_stride, params, keys);
}

int32_t hnsw_index_remove_keys(hnsw_index *idx, const int64_t *keys, int64_t m, int32_t *out_new_id) {
    std::vector<int64_t> ids;
    const int rc = ids_of_keys(idx, keys, m, "hnsw_index_remove_keys", ids);
    if (rc) return rc;
    return hnsw_index_remove(idx, ids.data(), m, out_new_id);
}

int32_t hnsw_index_mark_deleted_keys(hnsw_index *idx, const int64_t *keys, int64_t m) {
    std::vector<int64_t> ids;
    const int rc = ids_of_keys(idx, keys, m, "hnsw_index_mark_deleted_keys", ids);
    if (rc) return rc;
    return hnsw_index_mark_deleted(idx, ids.data(), m);
}

int32_t hnsw_index_unmark_deleted_keys(hnsw_index *idx, const int64_t *keys, int64_t m) {
    std::vector<int64_t> ids;
    const int rc = ids_of_keys(idx, keys, m, "hnsw_index_unmark_deleted_keys", ids);
    if (rc) return rc;
    return hnsw_index_unmark_deleted(idx, ids.data(), m);
}

int32_t hnsw_filter_create_by_keys(hnsw_index *idx, const int64_t *keys, int64_t m, hnsw_filter **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    std::vector<int64_t> ids;
    std::vector<int32_t> nodes;
    int rc = ids_of_keys(idx, keys, m, "hnsw_filter_create_by_keys", ids, &nodes);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    std::unique_ptr<hnsw_filter> f;
    if ((rc = new_filter(idx, idx->iv.n, f))) return rc;
    const int64_t words = (idx->iv.n + 31) / 32;
    if (words > 0) {
        HIP_TRY(hipMemset(f->bits.p, 0, (size_t)words * 4));
        if (m > 0) {
            DevBuf d_nodes;
            if ((rc = d_nodes.ensure((size_t)m * 4))) return rc;
            HIP_TRY(hipMemcpy(d_nodes.p, nodes.data(), (size_t)m * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(hnsw_dev::keys_allow_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, (uint32_t *)f->bits.p, (const int32_t *)d_nodes.p, m);
            if ((rc = launched("keys allow kernel"))) return rc;
            HIP_TRY(hipDeviceSynchronize());    // (d_nodes is freed on return)
        }
        // (ANDed with the live mask, as hnsw_filter_create's mask is: a current filter never allows a marked node)
        const hnsw_filter *const live = live_filter(idx);
        if ((rc = count_filter(f.get(), live ? (const uint32_t *)live->bits.p : nullptr))) return rc;
    }
    *out = f.release();
    return HNSW_OK;
}

} // extern "C"
