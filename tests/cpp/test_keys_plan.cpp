// keys_position, renumber_keys and smallest_duplicate (ocaml-hnsw_amd/csrc/hnsw_keys_plan.h) against naive restatements: the lookup
// on sorted arrays of length 0, 1, 2 and 1000 that hold INT64_MIN and INT64_MAX, with queries below, between and above; the
// renumbering rule new_key_of[new_id[v]] = key_of[v] over a grid of n and removal sets, against "the survivors' keys in order".  A
// host program: tests/test_keys_api.py builds it with -fsanitize=address,undefined and runs it.
#include "../../ocaml-hnsw_amd/csrc/hnsw_keys_plan.h"
#include "../../ocaml-hnsw_amd/csrc/hnsw_remove_plan.h"

#include <algorithm>
#include <cstdio>
#include <set>

using namespace hnsw_host;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int64_t naive_position(const std::vector<int64_t> &s, int64_t key) {
    for (size_t i = 0; i < s.size(); ++i) if (s[i] == key) return (int64_t)i;
    return -1;
}

int main() {
    long cases = 0, differ = 0;
    // ---- the lookup ----
    for (int64_t n : {0, 1, 2, 1000}) {
        for (int with_ends : {0, 1}) {
            std::set<int64_t> pool;
            if (with_ends && n >= 1) pool.insert(INT64_MIN);
            if (with_ends && n >= 2) pool.insert(INT64_MAX);
            // keys that differ only above bit 32, only in the low word, around zero: what a truncation or an unsigned compare confuses
            for (int64_t x : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)7 + ((int64_t)1 << 32), (int64_t)7, (int64_t)8,
                              -((int64_t)1 << 32), INT64_MIN / 2, (int64_t)-7 - ((int64_t)1 << 32)})
                if ((int64_t)pool.size() < n) pool.insert(x);
            while ((int64_t)pool.size() < n) pool.insert((int64_t)rnd64());
            std::vector<int64_t> sorted(pool.begin(), pool.end());      // (std::set<int64_t>: ascending signed order)
            std::vector<int64_t> asked(sorted);                         // every stored key, the last element included ...
            for (int64_t s : sorted) {                                  // ... its neighbours: between two stored keys, or absent at the ends
                if (s != INT64_MIN) asked.push_back(s - 1);
                if (s != INT64_MAX) asked.push_back(s + 1);
            }
            for (int64_t x : {INT64_MIN, INT64_MAX, (int64_t)0, (int64_t)-1}) asked.push_back(x);       // below all, above all
            for (int i = 0; i < 200; ++i) asked.push_back((int64_t)rnd64());
            for (int64_t key : asked) {
                ++cases;
                const int64_t got = keys_position(sorted.data(), n, key), want = naive_position(sorted, key);
                if (got != want) { ++differ; std::printf("lookup differs: n=%lld key=%lld got %lld want %lld\n", (long long)n, (long long)key, (long long)got, (long long)want); }
            }
        }
    }
    // ---- the renumbering rule, and the duplicate that is named ----
    for (int64_t n : {0, 1, 2, 63, 64, 65, 517, 2003}) {
        for (int dead_pct : {0, 1, 50, 99, 100}) {
            std::vector<uint8_t> dead((size_t)n), level((size_t)n, 0);
            std::vector<int64_t> key_of((size_t)n);
            for (int64_t v = 0; v < n; ++v) {
                dead[(size_t)v] = (int)(rnd64() % 100) < dead_pct;
                key_of[(size_t)v] = (int64_t)rnd64();
            }
            const RemovePlan p = remove_plan(level.data(), dead.data(), n, n ? 0 : -1);
            std::vector<int64_t> want;
            for (int64_t v = 0; v < n; ++v) {
                // brute force: new(v) = v - |{d dead : d < v}|
                int64_t below = 0;
                for (int64_t u = 0; u < v; ++u) below += dead[(size_t)u];
                if (!dead[(size_t)v]) {
                    if (p.new_id[(size_t)v] != v - below) { ++differ; std::printf("new_id differs: n=%lld v=%lld\n", (long long)n, (long long)v); }
                    want.push_back(key_of[(size_t)v]);
                }
            }
            ++cases;
            const std::vector<int64_t> got = renumber_keys(key_of.data(), n, p.new_id.data(), p.n);
            if (got != want) { ++differ; std::printf("renumbering differs: n=%lld dead=%d\n", (long long)n, dead_pct); }
            // two duplicated keys planted: the smaller one is named, whatever their places
            if (n >= 4) {
                std::vector<int64_t> s(key_of);
                s[0] = s[(size_t)n - 1] = INT64_MAX - 1;
                s[1] = s[(size_t)n / 2 + 1] = INT64_MIN + 1;
                std::sort(s.begin(), s.end());
                int64_t dup = 0;
                ++cases;
                if (!smallest_duplicate(s.data(), n, &dup) || dup != INT64_MIN + 1) { ++differ; std::printf("duplicate differs: n=%lld\n", (long long)n); }
            }
            std::vector<int64_t> u(key_of);
            std::sort(u.begin(), u.end());
            int64_t none = 0;
            ++cases;
            if ((std::adjacent_find(u.begin(), u.end()) != u.end()) != smallest_duplicate(u.data(), n, &none)) { ++differ; std::printf("distinct differs: n=%lld\n", (long long)n); }
        }
    }
    std::printf("keys plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
