// hnsw_mark_plan.h -- the index arithmetic of soft deletion that is plain numbers (host only, no HIP): how the mask of the live
// (not marked) nodes follows a renumbering of the nodes -- hnsw_index_remove's new ids, or hnsw_index_insert's "ids kept, new nodes
// behind them" -- and the marked ids of a mask in ascending order (what hnsw_index_compact removes).
// tests/cpp/test_mark_plan.cpp checks it against a naive restatement under AddressSanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hnsw_host {

// live: ceil(n_old / 32) words, bit v & 31 of word v >> 5 set = node v is live.  new_id [n_old]: the 0-based id node v has afterwards,
// -1 = the node is gone; null: every node keeps its id (nodes >= n_new are gone).  The mask of the n_new nodes afterwards: a node that
// was marked stays marked under its new id, every other node -- the ones no old node maps to included: they are new -- is live; the
// positions >= n_new of the last word are clear.
inline std::vector<uint32_t> renumber_live_mask(const uint32_t *live, int64_t n_old, const int32_t *new_id, int64_t n_new) {
    const int64_t words = (n_new + 31) / 32;
    std::vector<uint32_t> out((size_t)words, ~0u);
    if (n_new & 31) out[(size_t)words - 1] = (1u << (n_new & 31)) - 1u;
    for (int64_t v = 0; v < n_old; ++v) {
        if ((live[v >> 5] >> (v & 31)) & 1u) continue;
        const int64_t j = new_id ? (int64_t)new_id[v] : v;
        if (j >= 0 && j < n_new) out[(size_t)(j >> 5)] &= ~(1u << (j & 31));
    }
    return out;
}

// the nodes of [0, n) whose bit of `live` is clear, ascending, plus id_base
inline std::vector<int64_t> marked_ids(const uint32_t *live, int64_t n, int64_t id_base) {
    std::vector<int64_t> ids;
    for (int64_t v = 0; v < n; ++v)
        if (!((live[v >> 5] >> (v & 31)) & 1u)) ids.push_back(v + id_base);
    return ids;
}

} // namespace hnsw_host
