// hnsw_by_id_plan.h against a naive restatement: the drop-self rule on one row (self at 0, in the middle, at k, absent, twice, among
// fill entries; k = 1 and k = 1023), the limits of (ef', k'), and the chunk bounds of hnsw_knn_graph.  A host program: built with the
// host compiler under -fsanitize=address,undefined by tests/test_by_id_api.py.
#include "../../ocaml-hnsw_amd/csrc/hnsw_by_id_plan.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hnsw_host;

static long cases = 0, differ = 0;
#define EXPECT(c) do { ++cases; if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++differ; } } while (0)

// the definition, naively: copy the k + 1 entries, erase the first one equal to self among them, or the last one; keep k
static void naive(const std::vector<int32_t> &ids, const std::vector<float> &dist, int32_t self, std::vector<int32_t> &oi, std::vector<float> &od) {
    oi = ids; od = dist;
    size_t p = ids.size() - 1;
    for (size_t j = 0; j < ids.size(); ++j) if (ids[j] == self) { p = j; break; }
    oi.erase(oi.begin() + (long)p);
    od.erase(od.begin() + (long)p);
}

static void check_row(const std::vector<int32_t> &ids, int32_t self, int32_t want_p) {
    const int32_t k = (int32_t)ids.size() - 1;
    std::vector<float> dist(ids.size());
    for (size_t j = 0; j < ids.size(); ++j) dist[j] = ids[j] < 0 ? __builtin_nanf("") : 0.5f * (float)j;
    // exactly k entries each: the sanitizer sees a write past the row's end
    std::vector<int32_t> oi((size_t)k), wi;
    std::vector<float> od((size_t)k), wd;
    drop_self_row(ids.data(), dist.data(), k, self, oi.data(), od.data());
    naive(ids, dist, self, wi, wd);
    EXPECT(drop_self_position(ids.data(), k, self) == want_p);
    EXPECT(oi == wi);
    EXPECT(std::memcmp(od.data(), wd.data(), sizeof(float) * (size_t)k) == 0);        // (NaN fills: compared as bits)
    std::vector<int32_t> only((size_t)k);
    drop_self_row(ids.data(), nullptr, k, self, only.data(), nullptr);                  // (no distances wanted)
    EXPECT(only == wi);
}

int main() {
    // self at 0, in the middle, at k, absent, twice (the first one wins), among fill entries
    check_row({7, 1, 2, 3, 4}, 7, 0);
    check_row({1, 2, 7, 3, 4}, 7, 2);
    check_row({1, 2, 3, 4, 7}, 7, 4);
    check_row({1, 2, 3, 4, 5}, 7, 4);
    check_row({1, 7, 3, 7, 5}, 7, 1);
    check_row({7, 3, -1, -1, -1}, 7, 0);
    check_row({3, 7, -1, -1, -1}, 7, 1);
    check_row({3, 4, -1, -1, -1}, 7, 4);              // absent from a short row: the last fill goes, the row stays as it was
    check_row({-1, -1, -1}, 0, 2);                    // nothing found at all
    check_row({0, -1, -1}, -1, 1);                    // a self equal to the fill id is still "the first equal entry"
    // k = 1
    check_row({7, 9}, 7, 0);
    check_row({9, 7}, 7, 1);
    check_row({9, 8}, 7, 1);
    // k = 1023: every position of self, and absent
    {
        std::vector<int32_t> row(1024);
        for (int j = 0; j < 1024; ++j) row[(size_t)j] = 5000 + j;
        for (int p : {0, 1, 63, 64, 65, 511, 1022, 1023}) check_row(row, 5000 + p, p);
        check_row(row, 4, 1023);
        row[700] = row[100];
        check_row(row, row[100], 100);
    }
    // the source of every output entry: below p itself, from p on the next one
    for (int p = 0; p <= 5; ++p)
        for (int j = 0; j < 5; ++j) EXPECT(drop_self_source(j, p) == (j < p ? j : j + 1));

    // the limits: k in 1 .. 1023, and no k + 1 is formed beyond them
    EXPECT(!drop_self_k_ok(0) && !drop_self_k_ok(-1) && drop_self_k_ok(1) && drop_self_k_ok(1023) && !drop_self_k_ok(1024));
    EXPECT(!drop_self_k_ok(INT32_MAX) && !drop_self_k_ok(INT32_MIN));
    EXPECT(BY_ID_MAX_WIDTH == 1024);
    for (int k : {1, 10, 100, 1023}) {
        EXPECT(drop_self_inner_k(k) == k + 1);
        for (int ef : {1, k - 1, k, k + 1, k + 2, 1024})
            if (ef >= 1) EXPECT(drop_self_inner_ef(ef, k) == (ef > k + 1 ? ef : k + 1) && drop_self_inner_ef(ef, k) >= drop_self_inner_k(k));
    }
    EXPECT(drop_self_inner_ef(10, 10) == 11 && drop_self_inner_ef(16, 10) == 16 && drop_self_inner_ef(1024, 1023) == 1024);

    // the chunks of the graph call: n = 0, 1, chunk - 1, chunk, chunk + 1 (and several chunks) cover [0, n) once, in order
    for (int64_t chunk : {(int64_t)1, (int64_t)3, (int64_t)500, GRAPH_CHUNK_ROWS})
        for (int64_t n : {(int64_t)0, (int64_t)1, chunk - 1, chunk, chunk + 1, 4 * chunk + 3}) {
            if (n < 0) continue;
            const int64_t c = graph_chunks(n, chunk);
            EXPECT(c == (n + chunk - 1) / chunk);
            int64_t next = 0;
            for (int64_t i = 0; i < c; ++i) {
                int64_t first = -1, rows = -1;
                graph_chunk(n, chunk, i, &first, &rows);
                EXPECT(first == next && rows >= 1 && rows <= chunk && (rows == chunk || i == c - 1));
                next = first + rows;
            }
            EXPECT(next == n);
        }
    EXPECT(graph_chunks(0, 500) == 0 && graph_chunks(2003, 500) == 5 && graph_chunks(2003, 2003) == 1 && graph_chunks(2003, 2004) == 1);
    {
        int64_t first, rows;
        graph_chunk(2003, 500, 4, &first, &rows);
        EXPECT(first == 2000 && rows == 3);
    }
    std::printf("by-id plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
