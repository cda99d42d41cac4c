// hnsw_shard_plan.h -- the index arithmetic of the multi-device handles that is plain numbers (host only, no HIP): the contiguous
// partition bound of hnsw_multi's query shards and hnsw_sharded_build's row shards, the cut of a global allow-mask into one mask
// per shard (hnsw_sharded_filter_create), and where the lists of a segment merge lie in its tables and when it is refused (the
// sharded range calls, hnsw_merge_segments).  The callers word the error messages.
// tests/cpp/test_shard_plan.cpp checks it against a naive restatement under AddressSanitizer.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hnsw_host {

// part g of G over n items is [shard_lo(n, g, G), shard_lo(n, g + 1, G)): contiguous, sizes that differ by at most 1 -- the same
// bounds as sharding.shard_bounds
inline int64_t shard_lo(int64_t n, int g, int G) { return (int64_t)((__int128)n * g / G); }

// The bits [lo, lo + n) of a mask of n_bits bits (bits: ceil(n_bits / 32) words, bit v & 31 of word v >> 5) moved down to bit 0 of
// out: a funnel shift over two source words, the positions >= n of the last word clear.  out has max(ceil(n / 32), 1) words (an
// empty part still has a word, which is 0).
inline void cut_mask(const uint32_t *bits, int64_t n_bits, int64_t lo, int64_t n, uint32_t *out) {
    const int64_t src_words = (n_bits + 31) / 32, words = (n + 31) / 32, w0 = lo >> 5;
    const int sh = (int)(lo & 31);
    out[0] = 0u;
    for (int64_t w = 0; w < words; ++w) {
        const uint64_t a = bits[w0 + w], b = w0 + w + 1 < src_words ? bits[w0 + w + 1] : 0u;
        out[w] = (uint32_t)((a | (b << 32)) >> sh);
    }
    if (n & 31) out[words - 1] &= (1u << (n & 31)) - 1u;
}

// ---- the segment merge's lists -------------------------------------------------------------------------------------------------------
constexpr int SEG_LISTS = 64;                       // lists of one merge at most (the merge kernels' MERGE_LISTS)
constexpr int64_t SEG_ENTRIES = 0x7FFFFFFFLL;       // entries of one list, and of the merged result, at most: 2^31 - 1
enum SegRefusal { SEG_OK = 0, SEG_LIST_TOO_LONG = 1, SEG_SUM_TOO_LONG = 2 };

// The lists are added in order (at most SEG_LISTS: the callers check their count first).  List g's entries lie from entry base[g]
// on in the one table per kind -- the exclusive sum of the totals -- and its local id 0 is the global row first_row[g].
struct SegPlan {
    int32_t n_lists = 0;
    int64_t sum = 0, longest = 0;                   // of the totals added so far
    int64_t base[SEG_LISTS] = {}, first_row[SEG_LISTS] = {}, total[SEG_LISTS] = {};
    // the next list (number n_lists).  SEG_LIST_TOO_LONG: more than SEG_ENTRIES entries, the list is not added
    SegRefusal add(int64_t entries, int64_t first) {
        if (entries > SEG_ENTRIES) return SEG_LIST_TOO_LONG;
        base[n_lists] = sum;
        first_row[n_lists] = first;
        total[n_lists] = entries;
        sum += entries;
        if (entries > longest) longest = entries;
        ++n_lists;
        return SEG_OK;
    }
    // after the last list.  SEG_SUM_TOO_LONG: the merged result would have more than SEG_ENTRIES entries
    SegRefusal close() const { return sum > SEG_ENTRIES ? SEG_SUM_TOO_LONG : SEG_OK; }
};

// one list's prefix sums (lims, nq + 1 entries): they start at 0 and never step down.  *at: the query whose step does.
enum LimsRefusal { LIMS_OK = 0, LIMS_START = 1, LIMS_DECREASE = 2 };
inline LimsRefusal check_lims(const int64_t *lims, int64_t nq, int64_t *at) {
    if (lims[0] != 0) return LIMS_START;
    for (int64_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) { *at = q; return LIMS_DECREASE; }
    return LIMS_OK;
}

} // namespace hnsw_host
