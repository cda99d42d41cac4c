// Hnsw::Filter and Hnsw::Ohnsw::knn_filtered (the C++ mirror of hnsw_filter_* / hnsw_search_batch_filtered) on the reference's
// five-node example values (lib/ohnsw.ml:617-643: values [0;1;2;3;5], |a-b| distance == L2 at d = 1), linked as a chain.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>

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
    const float q[2] = {4.5f, 0.f};

    // everything allowed: the plain search
    Hnsw::Filter all(g, std::vector<bool>(6, true));
    EXPECT(all.count() == 6);
    auto r = Hnsw::Ohnsw::knn_filtered(g, all, 2, Hnsw::Mat{q, 2, 1}, 6);
    EXPECT(r.ids.size() == 4 && r.dist.size() == 4 && r.stage.size() == 2);
    EXPECT(r.ids[0] == 4 && r.ids[1] == 3 && r.dist[0] == 0.5f && r.dist[1] == 1.5f);
    EXPECT(r.ids[2] == 0 && r.ids[3] == 1 && r.dist[2] == 0.f && r.dist[3] == 1.f);
    EXPECT(r.stage[0] == 0 && r.stage[1] == 0);

    // nodes 1, 3 and 5, W of two: query 0 is served once W has doubled, the tie 3 / 5 lowest id first
    Hnsw::Filter some(g, std::vector<bool>{false, true, false, true, false, true});
    EXPECT(some.count() == 3);
    r = Hnsw::Ohnsw::knn_filtered(g, some, 2, Hnsw::Mat{q, 2, 1}, 2);
    EXPECT(r.ids[0] == 3 && r.ids[1] == 5 && r.dist[0] == 1.5f && r.dist[1] == 1.5f);
    EXPECT(r.ids[2] == 1 && r.ids[3] == 3 && r.dist[2] == 1.f && r.dist[3] == 3.f);
    EXPECT(r.stage[0] >= 1 && r.stage[1] >= 1);

    // one allowed node and k = 2: the exact stage, one real entry and the fill; the packed-word constructor, garbage past n
    const uint32_t word = 0xFFFFFFC0u | (1u << 2);
    Hnsw::Filter one(g, &word, 6);
    EXPECT(one.count() == 1);
    r = Hnsw::Ohnsw::knn_filtered(g, one, 2, Hnsw::Mat{q, 2, 1}, 4);
    EXPECT(r.ids[0] == 2 && r.dist[0] == 2.5f && r.ids[1] == -1 && std::isnan(r.dist[1]));
    EXPECT(r.ids[2] == 2 && r.dist[2] == 2.f && r.ids[3] == -1 && std::isnan(r.dist[3]));
    EXPECT(r.stage[0] == Hnsw::Ohnsw::Filtered::exact_stage && r.stage[1] == Hnsw::Ohnsw::Filtered::exact_stage);

    bool threw = false;
    try { Hnsw::Filter bad(g, std::vector<bool>(5, true)); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // n_bits != n
    threw = false;
    try { Hnsw::Ohnsw::knn_filtered(g, all, 3, Hnsw::Mat{q, 2, 1}, 2); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // k > ef
    if (fails) return 1;
    std::printf("filter front-end ok\n");
    return 0;
}
