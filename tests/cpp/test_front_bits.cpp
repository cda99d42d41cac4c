// Option "bit_rows" through the C++ front: Hnsw::bits (thresholds and codes), Hnsw::Rows::BITS and a search of a six-node L2 index
// over axis-aligned vectors, where every bit, every column mean and every expected distance can be written down by hand.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

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
    hnsw_index_info inf{};
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    const int rows0 = inf.row_format;
    const int64_t bytes0 = inf.device_bytes;
    EXPECT(rows0 != Hnsw::Rows::BITS && Hnsw::Rows::BITS == 7);

    // off: no copy to show
    bool threw = false;
    try { Hnsw::bits(g); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    // mode 2: sign bits, thresholds +0; equality gives 0
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_rows", 2));
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.row_format == Hnsw::Rows::BITS);
    EXPECT(inf.device_bytes == bytes0 + 6 * 64 + 4 * 512);           // n * 64 * NW + the threshold table, NW = 1
    int64_t rb = 0;
    Hnsw::check(hnsw_index_row_bytes(g.handle(), &rb));
    EXPECT(rb == 1);
    Hnsw::Bits b = Hnsw::bits(g);
    EXPECT(b.words == 1 && b.t.size() == 3 && b.codes.size() == 6);
    const uint32_t sign[6] = {1u, 2u, 4u, 0u, 0u, 0u};
    for (int i = 0; i < 6; ++i) EXPECT(b.codes[(size_t)i] == sign[i]);
    for (int j = 0; j < 3; ++j) EXPECT(b.t[(size_t)j] == 0.f);

    // (3, 0, 0): bits 001, Hamming distance 0 to node 0 alone; the answer carries the exact L2 distance over the float32 rows
    const float q[3] = {3, 0, 0};
    auto nn = Hnsw::Ohnsw::knn(g, 1, q);
    EXPECT(nn.size() == 1 && nn[0].node == 0 && nn[0].distance_to_target == 1.f);

    // mode 1: thresholds at the column means 1.5 / 6, -12 / 6, 8 / 6
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_rows", 1));
    b = Hnsw::bits(g);
    EXPECT(b.t[0] == 0.25f && b.t[1] == -2.f && b.t[2] == (float)(8.0 / 6.0));
    const uint32_t mean[6] = {3u, 2u, 6u, 2u, 0u, 2u};
    for (int i = 0; i < 6; ++i) EXPECT(b.codes[(size_t)i] == mean[i]);
    nn = Hnsw::Ohnsw::knn(g, 1, q);                                   // bits 011: node 0 again
    EXPECT(nn.size() == 1 && nn[0].node == 0 && nn[0].distance_to_target == 1.f);

    // a bad value, and the options it excludes
    EXPECT(hnsw_index_set_option(g.handle(), "bit_rows", 3) == HNSW_ERR_BAD_ARG);
    EXPECT(hnsw_index_set_option(g.handle(), "sq8_rows", 1) == HNSW_ERR_BAD_ARG);
    EXPECT(hnsw_index_set_option(g.handle(), "half_rows", 1) == HNSW_ERR_BAD_ARG);

    // 0: the previous rows and the previous bytes
    Hnsw::check(hnsw_index_set_option(g.handle(), "bit_rows", 0));
    Hnsw::check(hnsw_index_get_info(g.handle(), &inf));
    EXPECT(inf.row_format == rows0 && inf.device_bytes == bytes0);
    threw = false;
    try { Hnsw::bits(g); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    if (fails) return 1;
    std::printf("bits front-end ok\n");
    return 0;
}
