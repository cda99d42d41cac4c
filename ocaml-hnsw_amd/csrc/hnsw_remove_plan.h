// hnsw_remove_plan.h -- the index arithmetic of hnsw_index_remove that is plain numbers (host only, no HIP): the new ids of the
// live nodes, the upper-row layout they get, the new top layer and the new entry point.  tests/cpp/test_remove_plan.cpp checks it
// against a naive restatement under AddressSanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hnsw_host {

struct RemovePlan {
    int64_t n = 0;                     // live nodes
    std::vector<int32_t> new_id;       // [n_old]: the 0-based id node v has afterwards (v minus the removed nodes below it), -1 = removed
    std::vector<int32_t> upper_row;    // [n]: first upper row of the live node (its rows of layers 1..level side by side, nodes in order), -1 = none
    std::vector<uint8_t> level;        // [n]: the live node's level (kept)
    int64_t rowsU = 0;                 // upper rows in all
    int32_t max_layer = 0;             // the highest live level (0 for the empty index)
    int32_t entry = -1;                // new 0-based id: the old entry point if it is live, else the lowest-id live node of the highest
                                       // live level; -1 = the empty index
};

// level[v] / dead[v] (non-zero = removed) of the n_old nodes, entry_old 0-based (-1: none)
inline RemovePlan remove_plan(const uint8_t *level, const uint8_t *dead, int64_t n_old, int64_t entry_old) {
    RemovePlan p;
    p.new_id.assign((size_t)n_old, -1);
    int32_t first_of_top = -1;
    for (int64_t v = 0; v < n_old; ++v) {
        if (dead[v]) continue;
        const int32_t id = (int32_t)p.n++;
        p.new_id[(size_t)v] = id;
        const uint8_t l = level[v];
        p.level.push_back(l);
        p.upper_row.push_back(l ? (int32_t)p.rowsU : -1);
        p.rowsU += l;
        if (first_of_top < 0 || (int32_t)l > p.max_layer) { first_of_top = id; p.max_layer = l; }
    }
    if (p.n == 0) return p;
    p.entry = entry_old >= 0 && entry_old < n_old && !dead[entry_old] ? p.new_id[(size_t)entry_old] : first_of_top;
    return p;
}

} // namespace hnsw_host
