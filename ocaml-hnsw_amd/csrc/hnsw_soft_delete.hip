// hnsw_soft_delete.hip -- soft deletion owned by the index: hnsw_index_mark_deleted / hnsw_index_unmark_deleted flip bits of a device
// mask of the LIVE nodes that the handle owns (hnsw_index::live, an ordinary hnsw_filter over it), hnsw_index_deleted_count /
// hnsw_index_deleted_bits read it back, hnsw_index_compact hands the marked nodes to hnsw_index_remove (the contract:
// include/hnsw_mi355x.h).  Nothing here touches a graph table: marked nodes stay in the graph and every walk still goes through
// them; what honours the marks is the entry points' dispatch (live_filter: hnsw_capi.hip, hnsw_scan.hip, hnsw_range.hip,
// hnsw_filter.hip) and adopt_graph, which carries the mask through an insert or a removal (renumbered_live_filter, hnsw_mark_plan.h).
//
// Kernel.
//   mark_bits_kernel        one lane per id of the call: sets (unmark) or clears (mark) the node's bit of the live mask.  Two ids of
//                           one call may share a word: vector atomics (atomicOr / atomicAnd) on the words.
// The count afterwards comes from filter_popcount_kernel (count_filter).
#include "hnsw_internal.h"

namespace hnsw_dev {

__global__ void __launch_bounds__(256)
mark_bits_kernel(uint32_t *live, const int32_t *nodes, int64_t m, int32_t make_live) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t v = nodes[i];            // 0-based, checked on the host: 0 <= v < n
    const uint32_t bit = 1u << (v & 31);
    if (make_live) atomicOr(live + (v >> 5), bit);
    else atomicAnd(live + (v >> 5), ~bit);
}

} // namespace hnsw_dev

using namespace hnsw_host;

namespace hnsw_host {

int renumbered_live_filter(const hnsw_index *idx, const int32_t *new_id, int64_t n_new, std::unique_ptr<hnsw_filter> &out) {
    out.reset();
    if (idx->n_deleted <= 0 || !idx->live) return HNSW_OK;
    const int64_t n_old = idx->iv.n;
    std::vector<uint32_t> old((size_t)((n_old + 31) / 32));
    if (!old.empty()) HIP_TRY(hipMemcpy(old.data(), idx->live->bits.p, old.size() * 4, hipMemcpyDeviceToHost));
    const std::vector<uint32_t> words = renumber_live_mask(old.data(), n_old, new_id, n_new);
    int rc;
    if ((rc = new_filter(idx, n_new, out))) { out.reset(); return rc; }
    if (!words.empty()) {
        const hipError_t e = hipMemcpy(out->bits.p, words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) { out.reset(); return hip_fail(e, "live mask upload"); }
    }
    if ((rc = count_filter(out.get(), nullptr))) { out.reset(); return rc; }
    if (out->n_allowed == n_new) out.reset();          // every marked node is gone: the handle is one never marked again
    return HNSW_OK;
}

} // namespace hnsw_host

namespace {

// both calls: the bits of `ids` cleared (mark) or set (unmark) in the live mask, the count and the epoch after them
int32_t change_marks(hnsw_index *idx, const int64_t *ids, int64_t m, bool mark) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (m == 0) return HNSW_OK;
    if (!ids) return fail(HNSW_ERR_BAD_ARG, "null ids");
    const int64_t n = idx->iv.n;
    const int32_t base = idx->iv.id_base;
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<int32_t> nodes((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t v = ids[i] - base;
        if (v < 0 || v >= n) return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld is not a stored node", (long long)i, (long long)ids[i]);
        if (seen[(size_t)v]) return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld appears twice", (long long)i, (long long)ids[i]);
        seen[(size_t)v] = 1;
        nodes[(size_t)i] = (int32_t)v;
    }
    if (idx->live_requests > 0) return fail(HNSW_ERR_BAD_ARG, "%d submitted requests not waited for (hnsw_search_wait first)", idx->live_requests);
    if (idx->multi_replica) return fail(HNSW_ERR_BAD_ARG, "the index is a replica of an hnsw_multi: marking nodes of one replica would desynchronise the others");
    if (!mark && !idx->live) return HNSW_OK;            // never marked: every node is live already
    HIP_TRY(hipSetDevice(idx->device));
    int rc;
    if (!idx->live) {           // the first mark: a mask with every node live
        std::unique_ptr<hnsw_filter> f;
        if ((rc = new_filter(idx, n, f))) return rc;
        HIP_TRY(hipMemset(f->bits.p, 0xFF, (size_t)((n + 31) / 32) * 4));
        if ((rc = count_filter(f.get(), nullptr))) return rc;
        idx->live = std::move(f);
    }
    hnsw_filter *const live = idx->live.get();
    DevBuf d_nodes;
    if ((rc = d_nodes.ensure((size_t)m * 4))) return rc;
    HIP_TRY(hipMemcpy(d_nodes.p, nodes.data(), (size_t)m * 4, hipMemcpyHostToDevice));
    // (searches still in flight on caller streams -- hnsw_brute_force_batch_device -- read the mask: they finish first)
    HIP_TRY(hipDeviceSynchronize());
    const int64_t before = live->n_allowed;
    hipLaunchKernelGGL(hnsw_dev::mark_bits_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, (uint32_t *)live->bits.p,
                       (const int32_t *)d_nodes.p, m, mark ? 0 : 1);
    if ((rc = launched("mark bits kernel")) || (rc = count_filter(live, nullptr))) return rc;
    idx->n_deleted = n - live->n_allowed;
    // a call only clears bits or only sets them: a bit changed iff the count did
    if (live->n_allowed != before) {
        idx->epoch++;           // filters made before are refused from now on: their masks may allow a node that is marked now
        live->epoch = idx->epoch;
    }
    return HNSW_OK;
}

// the live mask's words on the host (all ones below n on a handle never marked)
int live_words(const hnsw_index *idx, std::vector<uint32_t> &w) {
    const int64_t n = idx->iv.n;
    w.assign((size_t)((n + 31) / 32), ~0u);
    if (w.empty()) return HNSW_OK;
    if (idx->live && idx->n_deleted > 0) {
        HIP_TRY(hipSetDevice(idx->device));
        HIP_TRY(hipMemcpy(w.data(), idx->live->bits.p, w.size() * 4, hipMemcpyDeviceToHost));
    }
    if (n & 31) w.back() |= ~((1u << (n & 31)) - 1u);   // (positions >= n: never reported as marked)
    return HNSW_OK;
}

} // namespace

extern "C" {

int32_t hnsw_index_mark_deleted(hnsw_index *idx, const int64_t *ids, int64_t m) { return change_marks(idx, ids, m, true); }

int32_t hnsw_index_unmark_deleted(hnsw_index *idx, const int64_t *ids, int64_t m) { return change_marks(idx, ids, m, false); }

int32_t hnsw_index_deleted_count(const hnsw_index *idx, int64_t *n_deleted) {
    if (!idx || !n_deleted) return fail(HNSW_ERR_BAD_ARG, "null index or null n_deleted");
    *n_deleted = idx->n_deleted;
    return HNSW_OK;
}

int32_t hnsw_index_deleted_bits(const hnsw_index *idx, uint32_t *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null index or null out");
    std::vector<uint32_t> w;
    const int rc = live_words(idx, w);
    if (rc) return rc;
    for (size_t i = 0; i < w.size(); ++i) out[i] = ~w[i];
    return HNSW_OK;
}

int32_t hnsw_index_compact(hnsw_index *idx, int32_t *out_new_id) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    std::vector<uint32_t> w;
    const int rc = live_words(idx, w);
    if (rc) return rc;
    const std::vector<int64_t> ids = marked_ids(w.data(), idx->iv.n, idx->iv.id_base);
    // hnsw_index_remove of the marked nodes: its repair, its refusals, all or nothing; its swap leaves nothing marked
    return hnsw_index_remove(idx, ids.data(), (int64_t)ids.size(), out_new_id);
}

} // extern "C"
