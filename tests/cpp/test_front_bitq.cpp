// Option "bit_query_bits" through the C++ front: Hnsw::bit_query_codes (the 4-bit query codes) and a search of the six-node L2 index
// of test_front_bits.cpp with the option on, where every code and the expected answer can be written down by hand.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const float vals[6][3] = {{2, 0, 0}, {0, 4, 0}, {0, 0, 8}, {-0.5f, 0, 0}, {0, -16, 0}, {0, 0, 0}};
    int32_t deg0[6], nbr0[6][5];
    for (int i = 0; i < 6; ++i) {
        deg0[i] = 5;
        for (int j = 0, s = 0; j < 6; ++j) if (j != i) nbr0[i][s++] = j;
    }
    hnsw_index_desc d{};
    d.vectors = &vals[0][0]; d.n = 6; d.d = 3; d.row_stride = 3; d.metric = HNSW_METRIC_L2; d.id_base = 0;
    d.max_degree0 = 5; d.max_degree = 1; d.max_layer = 0; d.entry_point = 2; d.deg0 = deg0; d.nbr0 = &nbr0[0][0]; d.upper = nullptr;
    auto g = Hnsw::Hgraph::create(d);

    // bit_rows off: no thresholds to quantise against, whatever bit_query_bits says; the option itself is accepted and does nothing
    const std::vector<float> Q = {7, 2.5f, -0.5f,   3, 0, 0,   0, 0, 0,   -1, 0.25f, 0.125f};
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_query_bits", 4));
    bool threw = false;
    try { Hnsw::bit_query_codes(g, Q); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    hnsw_index_info inf{};
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.row_format != Hnsw::Rows::BITS);
    const float q[3] = {3, 0, 0};
    auto nn = Hnsw::Ohnsw::knn(g, 1, q);
    EXPECT(nn.size() == 1 && nn[0].node == 0 && nn[0].distance_to_target == 1.f);

    // mode 2 (thresholds +0): y = q, a = max |y|, r = 7 / a, v = rint(y * r) half-to-even
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_rows", 2));
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.row_format == Hnsw::Rows::BITS);                       // the same rows: no format of its own
    const int64_t bytes_on = inf.device_bytes;
    std::vector<int8_t> v = Hnsw::bit_query_codes(g, Q);
    const int8_t want[12] = {7, 2, 0,   7, 0, 0,   0, 0, 0,   -7, 2, 1};   // 2.5 -> 2 and -0.5 -> -0 (ties to even); 1.75 -> 2, 0.875 -> 1
    EXPECT(v.size() == 12);
    for (size_t i = 0; i < 12 && i < v.size(); ++i) EXPECT(v[i] == want[i]);

    // (3, 0, 0): codes (7, 0, 0); <v, s> = 7 for node 0 (bits 001), -7 for every other node; the answer carries the exact L2
    // distance over the float32 rows
    nn = Hnsw::Ohnsw::knn(g, 1, q);
    EXPECT(nn.size() == 1 && nn[0].node == 0 && nn[0].distance_to_target == 1.f);
    // (-1, -1, 5): codes (-1, -1, 7); node 2 (bits 100): 1 + 1 + 7 = 9
    const float q2[3] = {-1, -1, 5};
    nn = Hnsw::Ohnsw::knn(g, 1, q2);
    EXPECT(nn.size() == 1 && nn[0].node == 2 && nn[0].distance_to_target == std::sqrt(1.f + 1.f + 9.f));

    // the codes do not depend on the option being on; bad values; nothing was allocated for it
    EXPECT(hnsw_index_set_option(g.handle(), "bit_query_bits", 1) == HNSW_ERR_BAD_ARG);
    EXPECT(hnsw_index_set_option(g.handle(), "bit_query_bits", 8) == HNSW_ERR_BAD_ARG);
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_query_bits", 0));
    std::vector<int8_t> again = Hnsw::bit_query_codes(g, Q);
    EXPECT(again == v);
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.row_format == Hnsw::Rows::BITS && inf.device_bytes == bytes_on);
    nn = Hnsw::Ohnsw::knn(g, 1, q);
    EXPECT(nn.size() == 1 && nn[0].node == 0 && nn[0].distance_to_target == 1.f);

    if (fails) return 1;
    std::printf("bitq front-end ok\n");
    return 0;
}
