// hnsw_scan_matrix_plan.h -- the host arithmetic of the exact scan of float rows through fp32 matrix instructions
// (hnsw_scan_matrix.hip; option "scan_matrix"): when scan_search may take it, its LDS layout, waves, scratch and grid, and the
// screening rule with its margins; at the end what the range scan's form of it adds (hnsw_range_matrix.hip).  Plain arithmetic on
// plain numbers, so that a host program can check it (tests/cpp/test_scan_matrix_plan.cpp, tests/cpp/test_range_matrix_plan.cpp);
// the rule's functions are the ones the kernels call.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HNSW_SCAN_MATRIX_FN __host__ __device__ inline
#else
#define HNSW_SCAN_MATRIX_FN inline
#endif

namespace hnsw_host {

constexpr int SCAN_MATRIX_TILE = 32;        // queries per tile: the N of one 32x32x2 matrix instruction
constexpr int SCAN_MATRIX_MAX_D = 512;      // the tile of a wider row does not fit beside four waves' buffers in 160 KB of LDS
constexpr int SCAN_MATRIX_PAD = 4;          // floats between the tile's rows: the 16 lanes of one ds_read_b128 pass hit 16 different bank quads
constexpr int SCAN_MATRIX_LDS_MAX = 160 * 1024;
constexpr int32_t SCAN_PATH_MATRIX = 3;     // hnsw_index_scan_path: beside SCAN_PATH_NONE / _FLOAT / _BYTES (hnsw_scan_bytes_plan.h)

// May a scan of this handle try the float matrix kernels?  (Whether it runs them is then the queries' business: the prepass's word.)
// bytes_eligible: scan_bytes_eligible said yes -- the byte path takes precedence and its float fallback stays the float kernels.
inline bool scan_matrix_eligible(int option, bool bytes_eligible, int d, bool per_query_filters) {
    return option == 1 && !bytes_eligible && d >= 1 && d <= SCAN_MATRIX_MAX_D && !per_query_filters;
}
// float4 chunks per lane of the float scan's grid for this d (pick_nch for d <= 512), and the floats of a padded row
inline int scan_matrix_nch(int d) { const int per_lane = ((d + 3) / 4 + 15) / 16; return per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : 8; }
constexpr int scan_matrix_width(int nch) { return 64 * nch; }
constexpr int scan_matrix_pitch(int nch) { return scan_matrix_width(nch) + SCAN_MATRIX_PAD; }      // floats per row of the tile in LDS
// the floats of a row that one stage of the software pipeline holds (piece / 2 VGPRs per lane and stage, two stages): 64 where two
// waves share a SIMD's registers (scan_matrix_waves 8), 128 where one has them all
constexpr int scan_matrix_piece(int nch) { return nch <= 2 ? 64 : 128; }
// LDS: the tile, then per wave 32 buffers of 64 words, 64 words `sorted`, 32 counters, 32 row terms
constexpr int scan_matrix_tile_bytes(int nch) { return SCAN_MATRIX_TILE * scan_matrix_pitch(nch) * 4; }
constexpr int SCAN_MATRIX_WAVE_BYTES = SCAN_MATRIX_TILE * 64 * 8 + 64 * 8 + SCAN_MATRIX_TILE * 4 + 32 * 4;
// waves per workgroup, one slab each: eight (two per SIMD) while they fit, else four
constexpr int scan_matrix_waves(int nch) { return scan_matrix_tile_bytes(nch) + 8 * SCAN_MATRIX_WAVE_BYTES <= SCAN_MATRIX_LDS_MAX ? 8 : 4; }
constexpr int scan_matrix_lds_bytes(int nch) { return scan_matrix_tile_bytes(nch) + scan_matrix_waves(nch) * SCAN_MATRIX_WAVE_BYTES; }

// One piece's scratch: a float term per query
inline int64_t scan_matrix_scratch(int64_t piece) { return piece * 4; }
// the grid of a launch of nq queries over `slabs` row slabs: (tiles, groups of scan_matrix_waves slabs)
inline int64_t scan_matrix_tiles(int64_t nq) { return (nq + SCAN_MATRIX_TILE - 1) / SCAN_MATRIX_TILE; }
inline int64_t scan_matrix_slab_groups(int64_t slabs, int nch) { return (slabs + scan_matrix_waves(nch) - 1) / scan_matrix_waves(nch); }

// ---- the screen (DESIGN.md section 3 derives it) -------------------------------------------------------------------------------
// With u = 2^-24, nx / nq the computed squared norms of the row and the query and acc the matrix unit's sum of x_i q_i:
//   L2  the scan's key f >= (nx + nq)(1 - eps) - 2 acc - A,            IP  the scan's sum f <= acc + eps (nx + nq) / 2 + A
// for eps = scan_matrix_eps(d) and every order and rounding (to nearest or truncating, fused or not, subnormals kept or flushed) of the
// unit.  A pair is DROPPED only when value > bound; written so that a NaN anywhere keeps the pair.
HNSW_SCAN_MATRIX_FN float scan_matrix_eps(int d) { return (float)(8 * d + 320) * 0x1p-24f; }
// what the row brings: NaN (the pair survives) for a norm that is not finite
HNSW_SCAN_MATRIX_FN float scan_matrix_row_term(int metric, float nx, float eps) {
    if (!(nx <= FLT_MAX)) return NAN;
    return metric == 0 ? nx * (1.0f - eps) : -0.5f * eps * nx;
}
// what the query brings, written by the prepass
HNSW_SCAN_MATRIX_FN float scan_matrix_query_term(int metric, float nq, float eps) { return metric == 0 ? nq * (1.0f - eps) : 0.5f * eps * nq; }
HNSW_SCAN_MATRIX_FN float scan_matrix_value(int metric, float row_term, float acc) {
    return metric == 0 ? __builtin_fmaf(-2.0f, acc, row_term) : row_term - acc;
}
// thr: the k-th word's squared-distance sum (L2) or distance 1 - sum (IP) as the float the key was made from
HNSW_SCAN_MATRIX_FN float scan_matrix_bound(int metric, float thr, float query_term) {
    if (!(query_term <= FLT_MAX)) return NAN;
    if (metric == 0) return __builtin_fmaf(thr, 1.0f + 0x1p-20f, 0x1p-98f) - query_term;
    const float t = thr - 1.0f;         // drop when -(acc + margin) > thr+ - 1, thr+ above the next float after thr
    return __builtin_fmaf(__builtin_fabsf(t) + 1.0f, 0x1p-20f, t) + query_term;
}
HNSW_SCAN_MATRIX_FN bool scan_matrix_survives(float value, float bound) { return !(value > bound); }

// ---- the range scan through the same screen (hnsw_range_matrix.hip) -------------------------------------------------------------
// The tile, the operands and the pipeline are the k-scan's; what a wave keeps beside them is smaller: survivors are bare 32-bit row
// numbers (no word is built before the exact evaluation, no list is merged, so no `sorted` scratch either).
constexpr int RANGE_MATRIX_BUF = 64;        // survivor rows per query and wave: one more block's 32 fit up to 32
// LDS per wave: 32 buffers of 64 row numbers (8 KB), 32 counters, 32 row terms
constexpr int RANGE_MATRIX_WAVE_BYTES = SCAN_MATRIX_TILE * RANGE_MATRIX_BUF * 4 + SCAN_MATRIX_TILE * 4 + 32 * 4;
// waves per workgroup, one slab each: the pipeline's stage decides, not the LDS -- a stage of 64 floats per row leaves room for two
// waves per SIMD, one of 128 takes a SIMD's whole register file (scan_matrix_piece)
constexpr int range_matrix_waves(int nch) { return scan_matrix_piece(nch) == 64 ? 8 : 4; }
constexpr int range_matrix_lds_bytes(int nch) { return scan_matrix_tile_bytes(nch) + range_matrix_waves(nch) * RANGE_MATRIX_WAVE_BYTES; }
inline int64_t range_matrix_slab_groups(int64_t slabs, int nch) { return (slabs + range_matrix_waves(nch) - 1) / range_matrix_waves(nch); }
// The float the key `khi` -- the largest key in range (range_key_bounds) -- was made from: the squared-distance sum (L2) or the
// distance 1 - sum (IP), what scan_matrix_bound takes for its threshold.  The bound is then fixed for the whole slab, and a pair is
// dropped only when its exact key is proven above khi; the interval's lower end only excludes NaN keys, at the exact evaluation.
HNSW_SCAN_MATRIX_FN float range_matrix_threshold(int metric, uint32_t khi) {
    const uint32_t bits = metric == 0 ? khi : (khi & 0x80000000u) ? (khi & 0x7FFFFFFFu) : ~khi;       // (IP: key_to_dist)
    return __builtin_bit_cast(float, bits);
}

} // namespace hnsw_host
