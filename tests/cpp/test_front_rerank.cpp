// Hnsw::Ohnsw::rerank (the C++ mirror of hnsw_rerank_batch) on the reference's five-node example values
// (lib/ohnsw.ml:617-643: values [0;1;2;3;5], |a-b| distance == L2 at d = 1), on an index without edges.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const float vals[6] = {0, 1, 2, 3, 5, 3};          // node 5 duplicates node 3
    int32_t deg0[6] = {0, 0, 0, 0, 0, 0}, nbr0[6] = {-1, -1, -1, -1, -1, -1};
    hnsw_index_desc d{};
    d.vectors = vals; d.n = 6; d.d = 1; d.row_stride = 1; d.metric = HNSW_METRIC_L2; d.id_base = 0;
    d.max_degree0 = 1; d.max_degree = 1; d.max_layer = 0; d.entry_point = 0; d.deg0 = deg0; d.nbr0 = nbr0; d.upper = nullptr;
    auto g = Hnsw::Hgraph::create(d);
    const float q[2] = {4.5f, 0.f};
    // query 0: candidates 5, 0, 4, 3 -> 4 (0.5), then the tie 3 / 5 (1.5) lowest id first; query 1: one real candidate
    const int32_t cand[2][4] = {{5, 0, 4, 3}, {-1, 2, -1, -1}};
    auto r = Hnsw::Ohnsw::rerank(g, 3, Hnsw::Mat{q, 2, 1}, &cand[0][0], 4);
    EXPECT(r.first.size() == 6 && r.second.size() == 6);
    EXPECT(r.first[0] == 4 && r.first[1] == 3 && r.first[2] == 5);
    EXPECT(r.second[0] == 0.5f && r.second[1] == 1.5f && r.second[2] == 1.5f);
    EXPECT(r.first[3] == 2 && r.second[3] == 2.f);
    EXPECT(r.first[4] == -1 && r.first[5] == -1 && std::isnan(r.second[4]) && std::isnan(r.second[5]));
    bool threw = false;
    try { Hnsw::Ohnsw::rerank(g, 5, Hnsw::Mat{q, 2, 1}, &cand[0][0], 4); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // k > cand_stride
    if (fails) return 1;
    std::printf("rerank front-end ok\n");
    return 0;
}
