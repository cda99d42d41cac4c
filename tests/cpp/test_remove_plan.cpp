// remove_plan (ocaml-hnsw_amd/csrc/hnsw_remove_plan.h): the plain numbers of hnsw_index_remove -- new ids, the upper layout of the
// live nodes, the new top layer and entry point -- over a grid of n, level patterns and removal sets (none, all, the entry point,
// the whole top layer, random fractions, contiguous blocks), against a naive restatement of the header's definition.  A host
// program: built and run by tests/test_remove_api.py under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../ocaml-hnsw_amd/csrc/hnsw_remove_plan.h"

#include <cstdio>
#include <random>

using hnsw_host::RemovePlan;
using hnsw_host::remove_plan;

static long cases = 0, bad = 0;

static void check(const std::vector<uint8_t> &level, const std::vector<uint8_t> &dead, int64_t entry_old) {
    ++cases;
    const int64_t n_old = (int64_t)level.size();
    const RemovePlan p = remove_plan(level.data(), dead.data(), n_old, entry_old);
    bool ok = (int64_t)p.new_id.size() == n_old;
    // NUMBERING: new(v) = v - |{d in D : d < v}|, counted the slow way
    int64_t live = 0;
    for (int64_t v = 0; ok && v < n_old; ++v) {
        int64_t below = 0;
        for (int64_t d = 0; d < v; ++d) below += dead[(size_t)d] != 0;
        ok = p.new_id[(size_t)v] == (dead[(size_t)v] ? -1 : (int32_t)(v - below));
        live += !dead[(size_t)v];
    }
    ok = ok && p.n == live && (int64_t)p.level.size() == live && (int64_t)p.upper_row.size() == live;
    // levels kept; rows of the live nodes side by side in node order; the top is the highest live level
    int64_t rows = 0;
    int top = 0;
    int64_t first_of_top = -1;
    for (int64_t v = 0; ok && v < n_old; ++v) {
        if (dead[(size_t)v]) continue;
        const size_t j = (size_t)p.new_id[(size_t)v];
        ok = p.level[j] == level[(size_t)v] && p.upper_row[j] == (level[(size_t)v] ? (int32_t)rows : -1);
        rows += level[(size_t)v];
        if ((int)level[(size_t)v] > top) top = level[(size_t)v];
    }
    for (int64_t v = 0; v < n_old && first_of_top < 0; ++v)
        if (!dead[(size_t)v] && (int)level[(size_t)v] == top) first_of_top = v;
    ok = ok && p.rowsU == rows && p.max_layer == (live ? top : 0);
    // ENTRY: the old one if live, else the lowest-id live node of the highest live level; none for the empty index
    int32_t want = -1;
    if (live) want = entry_old >= 0 && !dead[(size_t)entry_old] ? p.new_id[(size_t)entry_old] : p.new_id[(size_t)first_of_top];
    ok = ok && p.entry == want;
    if (!ok) {
        ++bad;
        if (bad <= 5) std::printf("FAIL n %lld entry %lld\n", (long long)n_old, (long long)entry_old);
    }
}

int main() {
    std::mt19937 rng(4711);
    for (int n : {1, 2, 3, 5, 8, 33, 64, 65, 200}) {
        for (int pattern = 0; pattern < 5; ++pattern) {
            std::vector<uint8_t> level((size_t)n, 0);
            for (int v = 0; v < n; ++v) {
                switch (pattern) {
                case 0: break;                                                              // flat
                case 1: level[(size_t)v] = (uint8_t)(v % 4 == 0) + (uint8_t)(v % 16 == 0); break;
                case 2: level[(size_t)v] = (uint8_t)(rng() % 8 == 0 ? 1 + rng() % 3 : 0); break;
                case 3: level[(size_t)v] = (uint8_t)(v == n / 2 ? 15 : 0); break;           // one node alone on the top layers
                default: level[(size_t)v] = (uint8_t)(rng() % 4); break;                    // several nodes on the top layer
                }
            }
            int top = 0;
            for (uint8_t l : level) top = l > top ? l : top;
            std::vector<int64_t> tops;
            for (int v = 0; v < n; ++v) if (level[(size_t)v] == top) tops.push_back(v);
            for (int64_t entry : {tops.front(), tops.back()}) {
                std::vector<uint8_t> dead((size_t)n, 0);
                check(level, dead, entry);                                                  // none
                dead.assign((size_t)n, 1);
                check(level, dead, entry);                                                  // all
                dead.assign((size_t)n, 0); dead[(size_t)entry] = 1;
                check(level, dead, entry);                                                  // the entry point
                dead.assign((size_t)n, 0);
                for (int64_t v : tops) dead[(size_t)v] = 1;
                check(level, dead, entry);                                                  // the whole top layer
                dead.assign((size_t)n, 1); dead[(size_t)(n - 1)] = 0;
                check(level, dead, entry);                                                  // all but the last
                for (int pct : {1, 20, 50, 90})
                    for (int rep = 0; rep < 3; ++rep) {
                        for (int v = 0; v < n; ++v) dead[(size_t)v] = (int)(rng() % 100) < pct;
                        check(level, dead, entry);
                    }
                for (int b0 : {0, n / 3, n - n / 4 - 1}) {                                  // a contiguous block
                    dead.assign((size_t)n, 0);
                    for (int v = b0; v < n && v <= b0 + n / 4; ++v) dead[(size_t)v] = 1;
                    check(level, dead, entry);
                }
            }
        }
    }
    std::printf("remove plan ok: %ld cases, %ld differ\n", cases, bad);
    return bad ? 1 : 0;
}
