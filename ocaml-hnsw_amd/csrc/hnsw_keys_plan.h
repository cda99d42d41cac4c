// hnsw_keys_plan.h -- the arithmetic of the keys an index owns that is plain numbers (no HIP call): where a key lies in the
// lookup table (the keys in ascending SIGNED order), how key_of follows a renumbering of the nodes (hnsw_index_remove's new ids),
// and the smallest key that occurs twice in a sorted list.  keys_find_kernel runs keys_lower_bound itself (hnsw_keys.hip), so the
// host test checks the code the device runs.
// tests/cpp/test_keys_plan.cpp checks it against a naive restatement under AddressSanitizer and UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define HNSW_KEYS_HD __host__ __device__
#else
#define HNSW_KEYS_HD
#endif

namespace hnsw_host {

// the position of `key` in sorted[0..n) (ascending as signed 64-bit numbers, pairwise distinct), or -1 if it is not there.  The
// bounds are 64-bit and the middle is lo + (hi - lo) / 2: no sum of two positions is formed.
HNSW_KEYS_HD inline int64_t keys_position(const int64_t *sorted, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;                 // the first position whose key is >= key lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == key ? lo : -1;
}

// new_key_of[new_id[v]] = key_of[v] for every surviving v (new_id[v] >= 0); n_new = the number of survivors
inline std::vector<int64_t> renumber_keys(const int64_t *key_of, int64_t n_old, const int32_t *new_id, int64_t n_new) {
    std::vector<int64_t> out((size_t)n_new, 0);
    for (int64_t v = 0; v < n_old; ++v) {
        const int64_t j = new_id[v];
        if (j >= 0 && j < n_new) out[(size_t)j] = key_of[v];
    }
    return out;
}

// sorted[0..n) ascending: is a key there twice?  *key = the smallest such key
inline bool smallest_duplicate(const int64_t *sorted, int64_t n, int64_t *key) {
    for (int64_t i = 0; i + 1 < n; ++i)
        if (sorted[i] == sorted[i + 1]) { *key = sorted[i]; return true; }
    return false;
}

} // namespace hnsw_host
