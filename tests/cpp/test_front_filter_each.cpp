// Hnsw::Filter::by_label / bits and Hnsw::Ohnsw::knn_filtered_each (the C++ mirror of hnsw_filter_create_by_label,
// hnsw_filter_bits and hnsw_search_batch_filtered_each) on the chain of tests/cpp/test_front_filter.cpp: each query's row of the
// per-query call against knn_filtered under that query's filter.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const float vals[6] = {0, 1, 2, 3, 5, 3};          // node 5 duplicates node 3
    // a chain 0 - 1 - 2 - 3 - 4, node 5 hanging off node 3
    int32_t deg0[6] = {1, 2, 2, 3, 1, 1};
    int32_t nbr0[18] = {1, -1, -1,  0, 2, -1,  1, 3, -1,  2, 4, 5,  3, -1, -1,  3, -1, -1};
    hnsw_index_desc d{};
    d.vectors = vals; d.n = 6; d.d = 1; d.row_stride = 1; d.metric = HNSW_METRIC_L2; d.id_base = 0;
    d.max_degree0 = 3; d.max_degree = 1; d.max_layer = 0; d.entry_point = 0; d.deg0 = deg0; d.nbr0 = nbr0; d.upper = nullptr;
    auto g = Hnsw::Hgraph::create(d);

    // label 0: nodes 1, 3, 5; label 1: nodes 0, 4; label 2: node 2 alone; label 3: nobody
    const std::vector<int32_t> labels{1, 0, 2, 0, 1, 0};
    auto fs = Hnsw::Filter::by_label(g, labels, 4);
    EXPECT(fs.size() == 4);
    EXPECT(fs[0].count() == 3 && fs[1].count() == 2 && fs[2].count() == 1 && fs[3].count() == 0);
    const uint32_t want_bits[4] = {0x2Au, 0x11u, 0x04u, 0x00u};
    for (int l = 0; l < 4; ++l) {
        const auto b = fs[(size_t)l].bits();
        EXPECT(b.size() == 1 && b[0] == want_bits[l]);
    }
    // a filter made from a mask gives its bits back too
    Hnsw::Filter some(g, std::vector<bool>{false, true, false, true, false, true});
    EXPECT(some.bits() == fs[0].bits());

    // six queries, every filter in use, not grouped by filter; k = 2, ef = 2: ladder stages and the exact stage in one call
    const float q[6] = {4.5f, 0.f, 2.2f, 3.f, 1.f, 4.5f};
    const std::vector<int32_t> which{0, 1, 2, 0, 3, 1};
    const Hnsw::Mat batch{q, 6, 1};
    const auto r = Hnsw::Ohnsw::knn_filtered_each(g, fs, which, 2, batch, 2);
    EXPECT(r.ids.size() == 12 && r.dist.size() == 12 && r.stage.size() == 6);
    for (size_t l = 0; l < 4; ++l) {
        const auto ref = Hnsw::Ohnsw::knn_filtered(g, fs[l], 2, batch, 2);
        for (size_t i = 0; i < 6; ++i) {
            if ((size_t)which[i] != l) continue;
            EXPECT(r.ids[2 * i] == ref.ids[2 * i] && r.ids[2 * i + 1] == ref.ids[2 * i + 1]);
            EXPECT(std::memcmp(&r.dist[2 * i], &ref.dist[2 * i], 8) == 0);
            EXPECT(r.stage[i] == ref.stage[i]);
        }
    }
    // what those rows are: query 0 under {1, 3, 5}: the tie 3 / 5 lowest id first; query 2 under {2}: one real entry and the fill
    EXPECT(r.ids[0] == 3 && r.ids[1] == 5 && r.dist[0] == 1.5f && r.dist[1] == 1.5f);
    EXPECT(r.ids[4] == 2 && r.ids[5] == -1 && std::isnan(r.dist[5]) && r.stage[2] == Hnsw::Ohnsw::Filtered::exact_stage);
    EXPECT(r.ids[8] == -1 && r.ids[9] == -1 && r.stage[4] == Hnsw::Ohnsw::Filtered::exact_stage);      // nobody carries label 3
    EXPECT(r.ids[10] == 4 && r.ids[11] == 0 && r.dist[10] == 0.5f && r.dist[11] == 4.5f);

    bool threw = false;
    try { Hnsw::Filter::by_label(g, std::vector<int32_t>{0, 0, 0, 0, 0, 4}, 4); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // a label past n_labels - 1
    threw = false;
    try { Hnsw::Ohnsw::knn_filtered_each(g, fs, std::vector<int32_t>{0, 1, 2, 0, 4, 1}, 2, batch, 2); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // a position past the table
    threw = false;
    try { Hnsw::Ohnsw::knn_filtered_each(g, fs, std::vector<int32_t>{0, 1}, 2, batch, 2); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // one position per query
    if (fails) return 1;
    std::printf("filter-each front-end ok\n");
    return 0;
}
