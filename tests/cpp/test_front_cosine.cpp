// HNSW_METRIC_COSINE through the C++ front: Hnsw::normalise, Hnsw::Ohnsw::rows and the searches of a six-node COSINE index over
// axis-aligned vectors, where the normaliser is exact (a power-of-two length, one non-zero value) and every expected number can
// be written down by hand.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    // nodes 0..4 along +x, +y, +z, -x, -y with lengths 2, 4, 8, 0.5, 16; node 5 is the zero vector
    const float vals[6][3] = {{2, 0, 0}, {0, 4, 0}, {0, 0, 8}, {-0.5f, 0, 0}, {0, -16, 0}, {0, 0, 0}};
    const float unit[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {0, 0, 0}};
    const float lens[6] = {2, 4, 8, 0.5f, 16, 0};
    const Hnsw::Mat X{&vals[0][0], 6, 3};

    std::vector<float> norms;
    const std::vector<float> nx = Hnsw::normalise(X, 0, &norms);
    EXPECT(nx.size() == 18 && norms.size() == 6);
    for (int i = 0; i < 6; ++i) {
        EXPECT(norms[(size_t)i] == lens[i]);
        for (int j = 0; j < 3; ++j) EXPECT(nx[(size_t)(3 * i + j)] == unit[i][j]);
    }
    EXPECT(Hnsw::normalise(X).size() == 18);

    // every node linked to every other one
    int32_t deg0[6], nbr0[6][5];
    for (int i = 0; i < 6; ++i) {
        deg0[i] = 5;
        for (int j = 0, s = 0; j < 6; ++j) if (j != i) nbr0[i][s++] = j;
    }
    hnsw_index_desc d{};
    d.vectors = &vals[0][0]; d.n = 6; d.d = 3; d.row_stride = 3; d.metric = HNSW_METRIC_COSINE; d.id_base = 0;
    d.max_degree0 = 5; d.max_degree = 1; d.max_layer = 0; d.entry_point = 2; d.deg0 = deg0; d.nbr0 = &nbr0[0][0]; d.upper = nullptr;
    auto g = Hnsw::Hgraph::create(d);
    hnsw_index_info inf{};
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.metric == HNSW_METRIC_COSINE && inf.metric == 2 && inf.n == 6 && inf.d == 3);

    // the index holds N(X)
    const std::vector<float> all = Hnsw::Ohnsw::rows(g);
    EXPECT(all.size() == 18);
    for (int i = 0; i < 18; ++i) EXPECT(all[(size_t)i] == (&unit[0][0])[i]);
    const std::vector<float> two = Hnsw::Ohnsw::rows(g, {4, 0});
    EXPECT(two.size() == 6 && two[1] == -1.f && two[0] == 0.f && two[2] == 0.f && two[3] == 1.f && two[4] == 0.f && two[5] == 0.f);
    bool threw = false;
    try { Hnsw::Ohnsw::rows(g, {6}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    // queries of any length: (0, -3, 0) is node 4's direction, opposite to node 1, at right angles to the rest; the zero query is at
    // distance 1 from everything
    const float q[2][3] = {{0, -3, 0}, {0, 0, 0}};
    auto nn = Hnsw::Ohnsw::knn(g, 1, q[0]);
    EXPECT(nn.size() == 1 && nn[0].node == 4 && nn[0].distance_to_target == 0.f);
    auto bf = Hnsw::Ohnsw::brute_force_knn(g, 6, Hnsw::Mat{&q[0][0], 2, 3});
    const int want_ids[6] = {4, 0, 2, 3, 5, 1};
    const float want_dist[6] = {0, 1, 1, 1, 1, 2};
    for (int i = 0; i < 6; ++i) {
        EXPECT(bf.first[(size_t)i] == want_ids[i] && bf.second[(size_t)i] == want_dist[i]);
        EXPECT(bf.first[(size_t)(6 + i)] == i && bf.second[(size_t)(6 + i)] == 1.f);
    }
    const int32_t ids[3] = {1, 4, 5};
    auto dist = Hnsw::Ohnsw::distance_l2(g, Hnsw::Mat{&q[0][0], 1, 3}, ids, 3);
    EXPECT(dist.size() == 3 && dist[0] == 2.f && dist[1] == 0.f && dist[2] == 1.f);

    // a data row with an infinity refuses the whole index
    float bad[6][3];
    for (int i = 0; i < 18; ++i) (&bad[0][0])[i] = (&vals[0][0])[i];
    bad[3][1] = std::numeric_limits<float>::infinity();
    d.vectors = &bad[0][0];
    threw = false;
    try { Hnsw::Hgraph::create(d); } catch (const std::invalid_argument &e) { threw = std::string(e.what()).find("row 3") != std::string::npos; }
    EXPECT(threw);

    if (fails) return 1;
    std::printf("cosine front-end ok\n");
    return 0;
}
