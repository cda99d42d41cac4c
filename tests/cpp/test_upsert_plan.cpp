// upsert_split, upsert_fill_new_id, upsert_fill_replaced and upsert_duplicate_key (ocaml-hnsw_amd/csrc/hnsw_upsert_plan.h) against naive
// restatements: the partition of a call into stored and new rows, the node counts and the first new position, the out_new_id /
// out_replaced fills (against remove_plan's numbering too: the removal half must agree with what the caller is told), the refusals
// (a node out of range, a node named twice, an absent key where that is refused) and the smallest duplicated key -- over the cases
// all stored, none stored, m == 0, every node replaced and random mixtures.  A host program: tests/test_upsert_api.py builds it with
// the host compiler, and once more with -fsanitize=address,undefined, and runs both.
#include "../../ocaml-hnsw_amd/csrc/hnsw_upsert_plan.h"
#include "../../ocaml-hnsw_amd/csrc/hnsw_remove_plan.h"

#include <cstdio>
#include <map>
#include <set>

using namespace hnsw_host;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd64() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static long cases = 0, differ = 0;
static void bad(const char *what, long long a, long long b) { ++differ; std::printf("%s differs: %lld %lld\n", what, a, b); }

// one call: nodes[i] in [-1, n_old), no node twice
static void check_call(const std::vector<int32_t> &nodes, int64_t n_old, int32_t base) {
    const int64_t m = (int64_t)nodes.size();
    ++cases;
    UpsertPlan p;
    int64_t where = -7;
    if (upsert_split(nodes.data(), m, n_old, true, p, &where) != UPSERT_OK) { bad("split refused", n_old, m); return; }
    // naive: the partition
    std::set<int64_t> P;
    std::vector<int64_t> in_order;
    for (int64_t i = 0; i < m; ++i) if (nodes[(size_t)i] >= 0) { P.insert(nodes[(size_t)i]); in_order.push_back(nodes[(size_t)i]); }
    if (p.n_old != n_old || p.n_replaced != (int64_t)P.size() || p.n_live != n_old - (int64_t)P.size() || p.n_final != n_old - (int64_t)P.size() + m)
        bad("counts", n_old, m);
    if (p.removed != in_order) bad("removed order", n_old, m);
    if ((int64_t)p.dead.size() != n_old || (int64_t)p.replaced.size() != m) { bad("sizes", n_old, m); return; }
    for (int64_t v = 0; v < n_old; ++v) if ((p.dead[(size_t)v] != 0) != (P.count(v) != 0)) bad("dead", n_old, v);
    // the fills, into buffers of exactly the documented size (the sanitizer watches the ends)
    std::vector<uint8_t> rep((size_t)m, 9);
    std::vector<int32_t> new_id((size_t)n_old, -99);
    upsert_fill_replaced(p, rep.data());
    upsert_fill_new_id(p, base, new_id.data());
    for (int64_t i = 0; i < m; ++i) if (rep[(size_t)i] != (nodes[(size_t)i] >= 0 ? 1 : 0)) bad("replaced", n_old, i);
    for (int64_t v = 0; v < n_old; ++v) {
        int64_t below = 0;
        for (int64_t u = 0; u < v; ++u) below += P.count(u);
        const int64_t want = P.count(v) ? base - 1 : base + v - below;
        if (new_id[(size_t)v] != want) bad("new_id", v, new_id[(size_t)v]);
    }
    // ... and remove_plan, which numbers the removal half, says the same
    std::vector<uint8_t> level((size_t)n_old, 0);
    const RemovePlan rp = remove_plan(level.data(), p.dead.data(), n_old, n_old ? 0 : -1);
    if (rp.n != p.n_live) bad("remove_plan n", rp.n, p.n_live);
    for (int64_t v = 0; v < n_old; ++v) if (rp.new_id[(size_t)v] + base != new_id[(size_t)v]) bad("remove_plan new_id", v, rp.new_id[(size_t)v]);
    // positions: row i of the call becomes node n_live + i, so the ids after the call are a permutation-free range
    if (p.n_live + m != p.n_final) bad("positions", p.n_live, p.n_final);
    // the call by id: the same list is accepted iff it names no absent node
    UpsertPlan q;
    const int rc = upsert_split(nodes.data(), m, n_old, false, q, &where);
    int64_t first_absent = -1;
    for (int64_t i = 0; i < m && first_absent < 0; ++i) if (nodes[(size_t)i] < 0) first_absent = i;
    if (first_absent < 0 ? rc != UPSERT_OK : (rc != UPSERT_OUT_OF_RANGE || where != first_absent)) bad("by id", rc, where);
}

int main() {
    // ---- the partition, counts, fills ----
    for (int64_t n_old : {0, 1, 2, 31, 32, 33, 300, 1001}) {
        for (int32_t base : {0, 1}) {
            check_call({}, n_old, base);                                                    // m == 0
            {   // none stored
                std::vector<int32_t> nodes(17, -1);
                check_call(nodes, n_old, base);
            }
            {   // all stored: every node replaced, in a shuffled order
                std::vector<int32_t> nodes((size_t)n_old);
                for (int64_t v = 0; v < n_old; ++v) nodes[(size_t)v] = (int32_t)v;
                for (int64_t v = n_old - 1; v > 0; --v) std::swap(nodes[(size_t)v], nodes[(size_t)(rnd64() % (uint64_t)(v + 1))]);
                check_call(nodes, n_old, base);
                // ... and every node replaced plus new rows between them
                std::vector<int32_t> more;
                for (int32_t v : nodes) { more.push_back(v); if (rnd64() % 3 == 0) more.push_back(-1); }
                check_call(more, n_old, base);
            }
            for (int pct : {1, 50, 99}) {   // mixtures: stored rows scattered through the call
                std::vector<int32_t> nodes;
                for (int64_t v = 0; v < n_old; ++v) if ((int)(rnd64() % 100) < pct) nodes.push_back((int32_t)v);
                for (int i = 0; i < 40; ++i) nodes.push_back(-1);
                for (int64_t v = (int64_t)nodes.size() - 1; v > 0; --v) std::swap(nodes[(size_t)v], nodes[(size_t)(rnd64() % (uint64_t)(v + 1))]);
                check_call(nodes, n_old, base);
            }
        }
    }
    // ---- refusals: out of range, twice ----
    {
        UpsertPlan p;
        int64_t where = -1;
        const int32_t twice[] = {4, -1, 9, 4, 9};
        ++cases;
        if (upsert_split(twice, 5, 10, true, p, &where) != UPSERT_TWICE || where != 3) bad("twice", where, 3);
        const int32_t range[] = {4, 10, 3};
        ++cases;
        if (upsert_split(range, 3, 10, true, p, &where) != UPSERT_OUT_OF_RANGE || where != 1) bad("range", where, 1);
        const int32_t neg[] = {4, -2};
        ++cases;
        if (upsert_split(neg, 2, 10, true, p, &where) != UPSERT_OUT_OF_RANGE || where != 1) bad("negative", where, 1);
        ++cases;
        if (upsert_split(range, 1, 0, false, p, &where) != UPSERT_OUT_OF_RANGE || where != 0) bad("empty index", where, 0);
    }
    // ---- the duplicated key that is named: the smallest, wherever the pairs lie ----
    for (int64_t m : {0, 1, 2, 3, 64, 1000}) {
        std::vector<int64_t> keys((size_t)m);
        std::set<int64_t> seen;
        for (int64_t i = 0; i < m; ++i) { int64_t k; do k = (int64_t)rnd64(); while (!seen.insert(k).second); keys[(size_t)i] = k; }
        int64_t dup = 5;
        ++cases;
        if (upsert_duplicate_key(keys.data(), m, &dup) || dup != 5) bad("distinct", m, dup);
        if (m >= 2) {
            std::vector<int64_t> k2(keys);
            k2[0] = k2[(size_t)m - 1] = INT64_MIN;                      // the smallest possible key, first and last row
            ++cases;
            if (!upsert_duplicate_key(k2.data(), m, &dup) || dup != INT64_MIN) bad("dup min", m, dup);
            if (k2 != std::vector<int64_t>([&] { std::vector<int64_t> k3(keys); k3[0] = k3[(size_t)m - 1] = INT64_MIN; return k3; }())) bad("keys changed", m, 0);
        }
        if (m >= 64) {
            std::vector<int64_t> k2(keys);
            k2[3] = k2[40] = INT64_MAX - 1;
            k2[7] = k2[(size_t)m / 2 + 1] = -((int64_t)1 << 40) - 5;     // the smaller pair lies between the larger pair's rows
            std::map<int64_t, int> count;
            for (int64_t k : k2) ++count[k];
            int64_t want = 0;
            for (const auto &kv : count) if (kv.second > 1) { want = kv.first; break; }      // (std::map: ascending signed order)
            ++cases;
            if (!upsert_duplicate_key(k2.data(), m, &dup) || dup != want) bad("dup smallest", dup, want);
        }
    }
    std::printf("upsert plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
