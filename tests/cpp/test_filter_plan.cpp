// filter_plan (ocaml-hnsw_amd/csrc/hnsw_filter_plan.h): the layout of the exact stage of hnsw_search_batch_filtered_each.  Over a
// grid of (queries, filters, tile, assignment) it checks what the masked scan and the scatter kernel rely on: every (filter,
// query) pair appears exactly once, every tile holds one filter's queries only, the rows ascend by (filter, query), a filter with
// queries gets fewer than T padding rows and one without gets no row, and the total is a multiple of T.  A host program: built
// and run by tests/test_filter_each_api.py under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../ocaml-hnsw_amd/csrc/hnsw_filter_plan.h"

#include <cstdio>
#include <map>
#include <random>

using hnsw_host::FilterRows;
using hnsw_host::filter_plan;
using Pairs = std::vector<std::pair<int32_t, int32_t>>;

static long cases = 0, bad = 0;

static void check(const Pairs &pairs, int n_filters, int T) {
    ++cases;
    const FilterRows r = filter_plan(pairs, T);
    bool ok = r.row_query.size() % (size_t)T == 0 && r.tile_filter.size() == r.row_query.size() / (size_t)T;
    std::map<int32_t, int32_t> filter_of;            // query -> filter (a query occurs once in the input)
    std::map<int32_t, size_t> group;                 // filter -> queries
    for (const auto &p : pairs) { filter_of[p.second] = p.first; ++group[p.first]; }
    std::map<int32_t, size_t> rows_of, pad_of;
    size_t seen = 0;
    int32_t last_f = -1, last_q = -1;
    for (size_t i = 0; ok && i < r.row_query.size(); ++i) {
        const int32_t f = r.tile_filter[i / (size_t)T], q = r.row_query[i];
        ok = f >= 0 && f < n_filters && f >= last_f;                         // tiles ascend by filter
        if (f != last_f) last_q = -1;
        last_f = f;
        ++rows_of[f];
        if (q < 0) { ++pad_of[f]; continue; }
        ok = ok && filter_of.count(q) && filter_of[q] == f && q > last_q;    // homogeneous tile; ascending, so no query twice
        last_q = q;
        ++seen;
    }
    ok = ok && seen == pairs.size() && rows_of.size() == group.size();       // every pair once; no rows for a filter without queries
    for (const auto &g : group) {
        const size_t rows = rows_of.count(g.first) ? rows_of[g.first] : 0, pad = pad_of.count(g.first) ? pad_of[g.first] : 0;
        ok = ok && rows == g.second + pad && pad < (size_t)T && rows % (size_t)T == 0;
    }
    // padding only at a group's end: a padding row is never followed by a query of the same filter
    for (size_t i = 0; ok && i + 1 < r.row_query.size(); ++i)
        if (r.row_query[i] < 0 && r.row_query[i + 1] >= 0) ok = r.tile_filter[i / (size_t)T] != r.tile_filter[(i + 1) / (size_t)T];
    if (!ok) {
        ++bad;
        if (bad <= 5) std::printf("FAIL m %zu filters %d T %d\n", pairs.size(), n_filters, T);
    }
}

int main() {
    std::mt19937 rng(12345);
    const int ms[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 300};
    for (int T : {4, 8})
        for (int m : ms)
            for (int L = 1; L <= 40; ++L) {
                std::vector<int32_t> queries((size_t)m);
                for (int i = 0; i < m; ++i) queries[(size_t)i] = 3 * i + 1;      // (query numbers need not be dense)
                std::shuffle(queries.begin(), queries.end(), rng);
                Pairs p((size_t)m);
                // uniformly random
                for (int i = 0; i < m; ++i) p[(size_t)i] = {(int32_t)(rng() % (unsigned)L), queries[(size_t)i]};
                check(p, L, T);
                // all in one filter: the first, the last
                for (int f : {0, L - 1}) {
                    for (int i = 0; i < m; ++i) p[(size_t)i] = {f, queries[(size_t)i]};
                    check(p, L, T);
                }
                // one each, round robin: groups of about m / L, most filters empty when m < L
                for (int i = 0; i < m; ++i) p[(size_t)i] = {(int32_t)(i % L), queries[(size_t)i]};
                check(p, L, T);
                // only the odd filters, the even ones empty; skewed: half of the queries in the last filter
                for (int i = 0; i < m; ++i) p[(size_t)i] = {(int32_t)(L > 1 ? (2 * (rng() % (unsigned)(L / 2)) + 1) : 0), queries[(size_t)i]};
                check(p, L, T);
                for (int i = 0; i < m; ++i) p[(size_t)i] = {(int32_t)(rng() % 2 ? L - 1 : rng() % (unsigned)L), queries[(size_t)i]};
                check(p, L, T);
                // groups of exactly T - 1, T and T + 1 queries in turn
                for (int i = 0, f = 0, left = T - 1, size = T - 1; i < m; ++i) {
                    p[(size_t)i] = {(int32_t)(f % L), queries[(size_t)i]};
                    if (--left == 0) { ++f; size = size == T + 1 ? T - 1 : size + 1; left = size; if (f >= L) { f = L - 1; left = m; } }
                }
                check(p, L, T);
            }
    std::printf("filter plan ok: %ld cases, %ld differ\n", cases, bad);
    return bad ? 1 : 0;
}
