// hnsw_scan_plan.h -- how an exact scan (hnsw_scan.hip, hnsw_range.hip) cuts its queries into pieces and the table into row slabs.
// Plain arithmetic on plain numbers, so that a host program can check it (tests/cpp/test_scan_plan.cpp).  Results never depend on
// the cut: every (query, slab) cell is exact for its slab.
#pragma once
#include <algorithm>
#include <cstdint>

namespace hnsw_host {

constexpr int64_t SCAN_SCRATCH = 256ll << 20;   // bytes of the handle's scratch one piece's (query, slab) cells may take

struct ScanPlan {
    int64_t piece = 0;       // queries per launch
    int64_t slab_rows = 0;   // slab s = rows [s * slab_rows, min(n, (s + 1) * slab_rows))
    int64_t slabs = 0;       // 0 when the table has no rows
};

// Rows per slab for a launch of `tiles` query tiles over n rows: enough (tile, slab) waves to fill the chip twice over, slabs of
// 256 rows at least, no more cells per query than their reader takes quickly (slabs * k <= 65 536, 1024 slabs).  scan_slabs > 0
// (option "scan_slabs") overrides the count.
inline int64_t scan_slab_rows(int64_t n, int scan_slabs, int64_t tiles, int k) {
    constexpr int64_t SCAN_TARGET_WAVES = 8192;
    int64_t slabs = scan_slabs > 0 ? scan_slabs : (SCAN_TARGET_WAVES + tiles - 1) / tiles;
    if (scan_slabs <= 0) slabs = std::min(slabs, std::max<int64_t>(1, n / 256));
    slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slabs, 1024), std::max<int64_t>(1, 65536 / k)));
    return std::max<int64_t>(1, (n + slabs - 1) / slabs);
}

// The cut for m >= 1 queries in tiles of T: the first piece is min(m, cap) queries, a (query, slab) cell takes cell_bytes.
inline ScanPlan scan_plan(int64_t n, int scan_slabs, int T, int64_t m, int k, int64_t cell_bytes, int64_t cap) {
    ScanPlan p{std::min(m, cap), 0, 0};
    for (;;) {      // (a smaller piece has fewer tiles and may be cut into more slabs: settle on a piece that fits)
        p.slab_rows = scan_slab_rows(n, scan_slabs, (p.piece + T - 1) / T, k);
        p.slabs = n > 0 ? (n + p.slab_rows - 1) / p.slab_rows : 0;
        const int64_t per_query = std::max<int64_t>(p.slabs, 1) * cell_bytes;
        if (p.piece * per_query <= SCAN_SCRATCH || p.piece <= T) return p;
        p.piece = std::max<int64_t>(T, SCAN_SCRATCH / per_query / T * T);
    }
}

} // namespace hnsw_host
