// hnsw_by_id_plan.h -- the arithmetic of the searches whose queries are stored rows (hnsw_by_id.hip) that is plain numbers (no HIP
// call): the drop-self rule on one result row, the inner call's (ef', k') and their limits, and how hnsw_knn_graph cuts the index
// into chunks.  drop_self_kernel takes its source position from drop_self_source and its p agrees with drop_self_position (the
// kernel finds it by ballot), so the host test checks the rule the device runs.
// tests/cpp/test_by_id_plan.cpp checks it against a naive restatement under AddressSanitizer and UBSan.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HNSW_BY_ID_HD __host__ __device__
#else
#define HNSW_BY_ID_HD
#endif

namespace hnsw_host {

// the widest inner row: k + 1 entries where the search's own limit is 1024 (k <= ef <= 1024)
constexpr int32_t BY_ID_MAX_WIDTH = 1024;
// may a call with exclude_self = 1 ask for k?  (k + 1 is never formed for a k that large: no overflow at INT32_MAX)
HNSW_BY_ID_HD inline bool drop_self_k_ok(int32_t k) { return k >= 1 && k <= BY_ID_MAX_WIDTH - 1; }
// the inner call of exclude_self = 1: k' = k + 1, ef' = max(ef, k + 1); drop_self_k_ok(k) holds
HNSW_BY_ID_HD inline int32_t drop_self_inner_k(int32_t k) { return k + 1; }
HNSW_BY_ID_HD inline int32_t drop_self_inner_ef(int32_t ef, int32_t k) { return ef > k + 1 ? ef : k + 1; }

// p of the inner row `row` (k + 1 ids): the smallest j in [0, k] with row[j] == self, or k if there is none
HNSW_BY_ID_HD inline int32_t drop_self_position(const int32_t *row, int32_t k, int32_t self) {
    for (int32_t j = 0; j <= k; ++j)
        if (row[j] == self) return j;
    return k;
}
// ... and where entry j in [0, k) of the output row comes from: the inner row with position p deleted
HNSW_BY_ID_HD inline int32_t drop_self_source(int32_t j, int32_t p) { return j < p ? j : j + 1; }
// the whole rule on one row on the host: out_ids / out_dist [k] from ids / dist [k + 1]
inline void drop_self_row(const int32_t *ids, const float *dist, int32_t k, int32_t self, int32_t *out_ids, float *out_dist) {
    const int32_t p = drop_self_position(ids, k, self);
    for (int32_t j = 0; j < k; ++j) {
        const int32_t s = drop_self_source(j, p);
        out_ids[j] = ids[s];
        if (out_dist) out_dist[j] = dist[s];
    }
}

// hnsw_knn_graph: the n nodes in chunks of chunk_rows >= 1 (option "graph_chunk_rows"), the last one shorter; n == 0: no chunk
constexpr int64_t GRAPH_CHUNK_ROWS = 65536;
inline int64_t graph_chunks(int64_t n, int64_t chunk_rows) { return n <= 0 ? 0 : (n - 1) / chunk_rows + 1; }
// chunk c in [0, graph_chunks): its first node (0-based) and how many
inline void graph_chunk(int64_t n, int64_t chunk_rows, int64_t c, int64_t *first, int64_t *rows) {
    *first = c * chunk_rows;
    *rows = n - *first < chunk_rows ? n - *first : chunk_rows;
}

} // namespace hnsw_host
