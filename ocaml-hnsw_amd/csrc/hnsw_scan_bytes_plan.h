// hnsw_scan_bytes_plan.h -- the host arithmetic of the exact scan over the byte rows (hnsw_scan_bytes.hip; option "scan_bytes"): when
// scan_search may take it, the layout of its query codes, and its scratch.  Plain arithmetic on plain numbers, so that a host
// program can check it (tests/cpp/test_scan_bytes_plan.cpp).
#pragma once
#include <cstdint>

namespace hnsw_host {

constexpr int SCAN_BYTES_TILE = 32;     // queries per tile: the N of one 32x32x32 matrix instruction
constexpr int SCAN_BYTES_WAVES = 2;     // waves per workgroup, one slab each
constexpr int SCAN_BYTES_MAX_D = 256;   // 256 * 255^2 < 2^24: every sum is an integer a float holds exactly

// what hnsw_index_scan_path reports
constexpr int32_t SCAN_PATH_NONE = 0, SCAN_PATH_FLOAT = 1, SCAN_PATH_BYTES = 2;

// May a scan of this handle try the matrix kernels?  (Whether it runs them is then the queries' business: the prepass's word.)
inline bool scan_bytes_eligible(int option, bool has_byte_rows, int d, bool per_query_filters) {
    return option == 1 && has_byte_rows && d >= 1 && d <= SCAN_BYTES_MAX_D && !per_query_filters;
}
// bytes of a byte row, and of a query's codes: 64 * pick_nch(ceil(d / 4)) for d <= 256
inline int scan_bytes_row_bytes(int d) { return d <= 64 ? 64 : d <= 128 ? 128 : 256; }

// One piece's scratch: the codes of its queries ([piece][row_bytes] int8), then their integer terms ([piece] int32, 16-byte aligned)
struct ScanBytesScratch {
    int64_t codes = 0, terms_at = 0, total = 0;
};
inline ScanBytesScratch scan_bytes_scratch(int64_t piece, int d) {
    ScanBytesScratch s;
    s.codes = piece * scan_bytes_row_bytes(d);
    s.terms_at = (s.codes + 15) / 16 * 16;
    s.total = s.terms_at + piece * 4;
    return s;
}
// the grid of a launch of nq queries over `slabs` row slabs: (tiles, groups of SCAN_BYTES_WAVES slabs)
inline int64_t scan_bytes_tiles(int64_t nq) { return (nq + SCAN_BYTES_TILE - 1) / SCAN_BYTES_TILE; }
inline int64_t scan_bytes_slab_groups(int64_t slabs) { return (slabs + SCAN_BYTES_WAVES - 1) / SCAN_BYTES_WAVES; }

} // namespace hnsw_host
