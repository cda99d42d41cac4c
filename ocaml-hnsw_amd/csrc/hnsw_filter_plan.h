// hnsw_filter_plan.h -- how the exact stage of a filtered search whose queries carry different filters (hnsw_filter.hip,
// hnsw_search_batch_filtered_each) lays its queries out for ONE masked scan: ordered by (filter, query), each filter's group
// padded to a whole number of scan tiles, so that no tile of T queries spans two filters and the scan takes its mask per tile.
// Plain arithmetic on plain numbers, so that a host program can check it (tests/cpp/test_filter_plan.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace hnsw_host {

struct FilterRows {
    std::vector<int32_t> row_query;      // [rows], rows a multiple of T: the query a row belongs to, -1 for a padding row
    std::vector<int32_t> tile_filter;    // [rows / T]: the filter of the tile's queries
};

// pairs: (filter, query), one per query, in any order.  Fewer than T padding rows per filter that has a query, none for one
// without.
inline FilterRows filter_plan(std::vector<std::pair<int32_t, int32_t>> pairs, int T) {
    std::sort(pairs.begin(), pairs.end());
    FilterRows r;
    r.row_query.reserve(pairs.size() + (size_t)T);
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        for (; j < pairs.size() && pairs[j].first == pairs[i].first; ++j) r.row_query.push_back(pairs[j].second);
        while (r.row_query.size() % (size_t)T) r.row_query.push_back(-1);
        r.tile_filter.insert(r.tile_filter.end(), (j - i + (size_t)T - 1) / (size_t)T, pairs[i].first);
        i = j;
    }
    return r;
}

} // namespace hnsw_host
