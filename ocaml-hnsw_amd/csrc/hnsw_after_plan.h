// hnsw_after_plan.h -- the arithmetic of the paged searches (hnsw_search_batch_after / hnsw_brute_force_batch_after, hnsw_after.hip)
// that is plain numbers: the order ord over the floats a caller holds, the word of a (distance, node) pair and of a cursor, the test
// "after", the next cursor of a row, and the L2 key bound hi(D).  Host and device share these functions, so that a host program can
// check what the kernels compute (tests/cpp/test_after_plan.cpp, plainly and under AddressSanitizer and UBSan).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define HNSW_AFTER_HD __host__ __device__ inline
#else
#define HNSW_AFTER_HD inline
#endif

namespace hnsw_after {

HNSW_AFTER_HD uint32_t float_bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
HNSW_AFTER_HD float bits_float(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

// ord: the monotone map of a float's bits that dist_to_key<1> applies to a distance -- the sign flipped, a negative value's other
// bits too: -inf < ... < -0 < +0 < ... < +inf < a positive NaN.  Injective: equal ord = equal bits.
HNSW_AFTER_HD uint32_t ord(float x) {
    const uint32_t b = float_bits(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
HNSW_AFTER_HD float ord_inverse(uint32_t o) { return bits_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// the word of (distance D, 0-based node v): ascending words = the paged order (ord(D), node id)
HNSW_AFTER_HD uint64_t word(float D, uint32_t v) { return ((uint64_t)ord(D) << 32) | v; }

// Node v (0-based) at distance D is AFTER the cursor (c_dist, c_id; c_id id_base-based, any value) iff ord(D) > ord(c_dist), or they
// are equal and v + id_base > c_id, the ids compared in 64 bits.  (A NaN c_dist is refused before this is asked.)
HNSW_AFTER_HD bool is_after(float D, int64_t v, int32_t id_base, float c_dist, int32_t c_id) {
    const uint32_t a = ord(D), c = ord(c_dist);
    return a > c || (a == c && v + (int64_t)id_base > (int64_t)c_id);
}

// The cursor as a bound in word space: is_after(D, v, ..) == (word(D, v) > cursor_word(..)) for every node v in [0, 2^32) and every D.
// With t = c_id - id_base the first word after the cursor is (ord << 32) + 0 for t < 0, (ord << 32) + t + 1 for t + 1 < 2^32 and
// ((ord + 1) << 32) beyond; the bound is that word minus one.  ord(c_dist) is neither 0 nor all ones (those are NaNs), so neither
// step leaves 64 bits.
HNSW_AFTER_HD uint64_t cursor_word(float c_dist, int32_t c_id, int32_t id_base) {
    const uint64_t o = ord(c_dist);
    const int64_t t = (int64_t)c_id - (int64_t)id_base;
    const uint64_t first = t < 0 ? (o << 32) : t + 1 <= 0xFFFFFFFFll ? ((o << 32) | (uint64_t)(t + 1)) : ((o + 1) << 32);
    return first - 1;
}

// out_next of a row: (distance, id) of its last real entry (ids below id_base are fill), the input cursor when it has none
HNSW_AFTER_HD void next_cursor(const int32_t *ids, const float *dist, int32_t k, int32_t id_base, float c_dist, int32_t c_id, float *n_dist,
                               int32_t *n_id) {
    *n_dist = c_dist;
    *n_id = c_id;
    for (int32_t j = k - 1; j >= 0; --j)
        if (ids[j] >= id_base) { *n_dist = dist[j]; *n_id = ids[j]; return; }
}

// hi(D) = max{s : sqrtf(s) <= D} over the L2 keys s (the bits of the non-negative floats up to +inf), -1 when there is none (D < 0;
// D = -0 has s = 0).  sqrtf is monotone and maps two to three neighbouring s onto one D, so the rounded square is within a few
// steps of the answer and the definition itself settles them.  D must not be NaN.
HNSW_AFTER_HD int64_t l2_key_hi(float D) {
    if (!(D >= 0.f)) return -1;
    const float sq = D * D;                 // (+inf where the square overflows)
    uint32_t s = float_bits(sq) & 0x7FFFFFFFu;
    while (s > 0u && sqrtf(bits_float(s)) > D) --s;
    while (s < 0x7F800000u && sqrtf(bits_float(s + 1u)) <= D) ++s;
    return (int64_t)s;
}

} // namespace hnsw_after
