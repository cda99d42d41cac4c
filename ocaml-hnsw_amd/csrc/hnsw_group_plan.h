// hnsw_group_plan.h -- how the grouped exact stage (hnsw_group.hip) cuts its queries into pieces.  Plain arithmetic on plain
// numbers, so that a host program can check it (tests/cpp/test_group_plan.cpp).  A piece's scratch is best[piece][n_labels] 64-bit
// words, one cell per (query, label); results never depend on the cut: every cell is the exact minimum of its label for its query.
#pragma once
#include "hnsw_scan_plan.h"

namespace hnsw_host {

struct GroupPlan {
    int64_t piece = 0;       // queries per launch: a multiple of the scan's tile T
    int64_t slab_rows = 0;   // the rows' cut of one launch: scan_plan's for a piece of that many queries
    int64_t slabs = 0;       // 0 when the table has no rows
};

// Queries per launch for m >= 1 queries in tiles of T under n_labels >= 1 labels: the m queries rounded up to whole tiles, at most
// what SCAN_SCRATCH holds (8 * n_labels bytes per query) rounded down to whole tiles, never below one tile.
inline int64_t group_piece(int T, int64_t m, int64_t n_labels) {
    const int64_t whole = (m + T - 1) / T * T;
    const int64_t fit = SCAN_SCRATCH / (8 * n_labels) / T * T;
    return std::max<int64_t>(T, std::min(whole, fit));
}

// ... and the rows' cut of such a launch (no cell of the scan's own: the cut never shrinks the piece)
inline GroupPlan group_plan(int64_t n, int scan_slabs, int T, int64_t m, int64_t n_labels, int k) {
    GroupPlan g;
    g.piece = group_piece(T, m, n_labels);
    const ScanPlan p = scan_plan(n, scan_slabs, T, g.piece, k, 0, g.piece);
    g.slab_rows = p.slab_rows;
    g.slabs = p.slabs;
    return g;
}

} // namespace hnsw_host
