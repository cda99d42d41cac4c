// renumber_live_mask and marked_ids (ocaml-hnsw_amd/csrc/hnsw_mark_plan.h) against a naive restatement, over a grid of n, marked
// sets and renumberings (identity with growth = an insert; a removal set that takes some, all or none of the marked nodes).  A host
// program: tests/test_soft_delete_api.py builds it with -fsanitize=address,undefined and runs it.
#include "../../ocaml-hnsw_amd/csrc/hnsw_mark_plan.h"
#include "../../ocaml-hnsw_amd/csrc/hnsw_remove_plan.h"

#include <cstdio>

using namespace hnsw_host;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

int main() {
    long cases = 0, differ = 0;
    for (int64_t n : {0, 1, 2, 31, 32, 33, 63, 64, 65, 100, 517, 2003}) {
        for (int mark_pct : {0, 1, 50, 99, 100}) {
            for (int dead_pct : {-1, 0, 10, 50, 100}) {         // -1: an insert of `grow` nodes instead of a removal
                for (int64_t grow : {0, 1, 40}) {
                    if (dead_pct >= 0 && grow) continue;
                    std::vector<uint8_t> marked((size_t)n), dead((size_t)n, 0), level((size_t)n, 0);
                    for (int64_t v = 0; v < n; ++v) marked[(size_t)v] = (int)(rnd() % 100) < mark_pct;
                    if (dead_pct >= 0) for (int64_t v = 0; v < n; ++v) dead[(size_t)v] = (int)(rnd() % 100) < dead_pct;
                    std::vector<uint32_t> live((size_t)((n + 31) / 32) + 1, 0u);      // (a word of room: n = 0 still has an address)
                    for (int64_t v = 0; v < n; ++v) if (!marked[(size_t)v]) live[(size_t)(v >> 5)] |= 1u << (v & 31);
                    int64_t n_new;
                    std::vector<uint32_t> got;
                    std::vector<uint8_t> want;                  // naive: per new node, is it marked
                    if (dead_pct >= 0) {
                        const RemovePlan p = remove_plan(level.data(), dead.data(), n, n ? 0 : -1);
                        n_new = p.n;
                        got = renumber_live_mask(live.data(), n, p.new_id.data(), n_new);
                        for (int64_t v = 0; v < n; ++v) if (!dead[(size_t)v]) want.push_back(marked[(size_t)v]);
                    } else {
                        n_new = n + grow;
                        got = renumber_live_mask(live.data(), n, nullptr, n_new);
                        for (int64_t v = 0; v < n; ++v) want.push_back(marked[(size_t)v]);
                        for (int64_t v = 0; v < grow; ++v) want.push_back(0);
                    }
                    ++cases;
                    bool bad = (int64_t)want.size() != n_new || (int64_t)got.size() != (n_new + 31) / 32;
                    for (int64_t j = 0; !bad && j < (int64_t)got.size() * 32; ++j) {
                        const bool is_live = (got[(size_t)(j >> 5)] >> (j & 31)) & 1u;
                        bad = j < n_new ? is_live == (want[(size_t)j] != 0) : is_live;       // past n_new: clear
                    }
                    // marked_ids of the old mask: the marked nodes ascending, id_base added
                    const std::vector<int64_t> ids = marked_ids(live.data(), n, 1);
                    size_t at = 0;
                    for (int64_t v = 0; !bad && v < n; ++v)
                        if (marked[(size_t)v]) bad = at >= ids.size() || ids[at++] != v + 1;
                    bad = bad || at != ids.size();
                    if (bad) { ++differ; std::printf("differs: n=%lld mark=%d dead=%d grow=%lld\n", (long long)n, mark_pct, dead_pct, (long long)grow); }
                }
            }
        }
    }
    std::printf("mark plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
