// hnsw_scan_bytes_plan.h -- the host arithmetic of the exact scan over the byte rows (hnsw_scan_bytes.hip; option "scan_bytes"): when
// scan_search may take it, the layout of its query codes, and its scratch; at the end what the range scan's form of it adds
// (hnsw_range_bytes.hip).  Plain arithmetic on plain numbers, so that a host program can check it (tests/cpp/test_scan_bytes_plan.cpp,
// tests/cpp/test_range_bytes_plan.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HNSW_SCAN_BYTES_FN __host__ __device__ inline
#else
#define HNSW_SCAN_BYTES_FN inline
#endif

namespace hnsw_host {

constexpr int SCAN_BYTES_TILE = 32;     // queries per tile: the N of one 32x32x32 matrix instruction
constexpr int SCAN_BYTES_WAVES = 2;     // waves per workgroup, one slab each
constexpr int SCAN_BYTES_MAX_D = 256;   // 256 * 255^2 < 2^24: every sum is an integer a float holds exactly

// what hnsw_index_scan_path reports
constexpr int32_t SCAN_PATH_NONE = 0, SCAN_PATH_FLOAT = 1, SCAN_PATH_BYTES = 2;

// May a scan of this handle try the matrix kernels?  (Whether it runs them is then the queries' business: the prepass's word.)
// Option values: 1 = the k-scans; 2 = the k-scans and the range scans (range_bytes_eligible, below).
inline bool scan_bytes_eligible(int option, bool has_byte_rows, int d, bool per_query_filters) {
    return (option == 1 || option == 2) && has_byte_rows && d >= 1 && d <= SCAN_BYTES_MAX_D && !per_query_filters;
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

// ---- the range scan over the byte rows (hnsw_range_bytes.hip; option value 2) ---------------------------------------------------
// Tile, operands and row terms are the k-scan's; a wave keeps no lists and no buffers (128 bytes of LDS), so registers set the
// occupancy and a workgroup holds one wave per SIMD.  The bound's functions are the ones the kernel calls.
constexpr int RANGE_BYTES_WAVES = 4;                // waves per workgroup, one slab each
inline bool range_bytes_eligible(int option, bool has_byte_rows, int d, bool per_query_filters) {
    return option == 2 && scan_bytes_eligible(option, has_byte_rows, d, per_query_filters);
}
inline int64_t range_bytes_slab_groups(int64_t slabs) { return (slabs + RANGE_BYTES_WAVES - 1) / RANGE_BYTES_WAVES; }

// A pair's integer rank value m -- L2: the squared distance, in [0, 2^24]; IP: minus the inner product, in [-2^24, 0] -- and the key
// the scans make of it (dist_to_key of the float the integer is, exactly): monotone in m.
constexpr int32_t RANGE_BYTES_MAX_M = 1 << 24;
HNSW_SCAN_BYTES_FN uint32_t range_bytes_key(int metric, int32_t m) {
    if (metric == 0) return __builtin_bit_cast(uint32_t, (float)m);
    const uint32_t b = __builtin_bit_cast(uint32_t, 1.0f - (float)(-m));    // (exact: an integer in [1 - 2^24, 1])
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// The hits of a radius whose keys are [klo, khi] (range_key_bounds) are the m <= *bound: the largest m of the metric's range with
// klo <= key(m) <= khi, by bisection on the keys themselves (at most 25 steps), never by float arithmetic on the radius.  false: no m.
HNSW_SCAN_BYTES_FN bool range_bytes_bound(int metric, uint32_t klo, uint32_t khi, int32_t *bound) {
    int32_t a = metric == 0 ? 0 : -RANGE_BYTES_MAX_M, b = metric == 0 ? RANGE_BYTES_MAX_M : 0;
    if (khi < klo || range_bytes_key(metric, a) > khi) return false;
    while (a < b) {             // a is in range; the answer lies in [a, b]
        const int32_t mid = a + (b - a + 1) / 2;
        if (range_bytes_key(metric, mid) <= khi) a = mid; else b = mid - 1;
    }
    if (range_bytes_key(metric, a) < klo) return false;     // (klo is the first key of all: only a NaN's key lies below it)
    *bound = a;
    return true;
}
// A lane compares v = (row term) - (1 or 2) acc against (bound - query term).  Real row and query terms lie within +-2^25 and
// |acc| <= 2^22, so |v| < 2^27 and |bound - query term| < 2^26: the row term of a row that is no candidate puts v above every lane
// bound, the lane bound of a query without hits lies below every v, and no subtraction overflows.  The k-scan makes the same values
// and its row sentinel is the same: above every bound that a full list sets (a list still short of k words takes every candidate row
// and tests the candidate word itself).
constexpr int32_t SCAN_BYTES_NO_ROW = 0x3FFFFFFF, RANGE_BYTES_NO_HIT = -0x40000000;
constexpr int32_t RANGE_BYTES_NO_ROW = SCAN_BYTES_NO_ROW;      // (the name the range scan's host test knows)

} // namespace hnsw_host
