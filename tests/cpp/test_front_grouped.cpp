// Hnsw::Labels and Hnsw::Ohnsw::knn_grouped / brute_force_grouped (the C++ mirror of hnsw_labels_*, hnsw_search_batch_grouped and
// hnsw_brute_force_batch_grouped) on the chain of tests/cpp/test_front_filter_each.cpp: one small grouped call and one exact call.
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
    Hnsw::Labels l(g, labels, 4);
    const auto info = l.info();
    EXPECT(info.n_labels == 4 && info.n_labelled == 6 && info.n_groups == 3);
    EXPECT(l.get() == labels);

    // the exact call: per label its nearest node (the tie 3 / 5 of label 0: the lower id), the three groups ascending, then the fill
    const float q[2] = {4.5f, 0.2f};
    const Hnsw::Mat batch{q, 2, 1};
    const auto x = Hnsw::Ohnsw::brute_force_grouped(g, l, 4, batch);
    EXPECT(x.ids.size() == 8 && x.dist.size() == 8 && x.labels.size() == 8);
    EXPECT(x.ids[0] == 4 && x.ids[1] == 3 && x.ids[2] == 2 && x.ids[3] == -1);
    EXPECT(x.labels[0] == 1 && x.labels[1] == 0 && x.labels[2] == 2 && x.labels[3] == -1);
    EXPECT(x.dist[0] == 0.5f && x.dist[1] == 1.5f && x.dist[2] == 2.5f && std::isnan(x.dist[3]));
    EXPECT(x.ids[4] == 0 && x.ids[5] == 1 && x.ids[6] == 2 && x.ids[7] == -1);
    EXPECT(x.labels[4] == 1 && x.labels[5] == 0 && x.labels[6] == 2 && x.labels[7] == -1);

    // the grouped search, k = 3 of three groups with W = the whole graph: stage 0, the exact call's rows
    const auto r = Hnsw::Ohnsw::knn_grouped(g, l, 3, batch, 6);
    EXPECT(r.ids.size() == 6 && r.stage.size() == 2 && r.stage[0] == 0 && r.stage[1] == 0);
    for (size_t i = 0; i < 2; ++i)
        for (size_t j = 0; j < 3; ++j) {
            EXPECT(r.ids[3 * i + j] == x.ids[4 * i + j] && r.labels[3 * i + j] == x.labels[4 * i + j]);
            EXPECT(std::memcmp(&r.dist[3 * i + j], &x.dist[4 * i + j], 4) == 0);
        }
    // k = 4 > n_groups: no walk, the exact stage and its fill
    const auto r4 = Hnsw::Ohnsw::knn_grouped(g, l, 4, batch, 6);
    EXPECT(r4.stage[0] == Hnsw::Ohnsw::Grouped::exact_stage && r4.stage[1] == Hnsw::Ohnsw::Grouped::exact_stage);
    EXPECT(r4.ids == x.ids && r4.labels == x.labels && std::memcmp(r4.dist.data(), x.dist.data(), 32) == 0);
    // under a filter that allows nodes 1, 4, 5 only: label 0 is represented by node 5 for the first query
    Hnsw::Filter f(g, std::vector<bool>{false, true, false, false, true, true});
    const auto xf = Hnsw::Ohnsw::brute_force_grouped(g, l, 2, batch, &f);
    EXPECT(xf.ids[0] == 4 && xf.ids[1] == 5 && xf.labels[0] == 1 && xf.labels[1] == 0);

    bool threw = false;
    try { Hnsw::Labels bad(g, std::vector<int32_t>{0, 0, 0, 0, 0, 4}, 4); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // a label past n_labels - 1
    threw = false;
    try { Hnsw::Ohnsw::knn_grouped(g, l, 3, batch, 2); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // k > ef
    if (fails) return 1;
    std::printf("grouped front-end ok\n");
    return 0;
}
