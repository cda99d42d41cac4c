// Hnsw::Ohnsw::remove (the C++ mirror of hnsw_index_remove) on the reference's five-node example values (lib/ohnsw.ml:617-643:
// values [0;1;2;3;5], |a-b| distance == L2 at d = 1), linked as a chain 0 - 1 - 2 - 3 - 4: the middle node leaves, its two
// neighbours propose each other (each is nearer to the other than to its own live neighbour), offer and agree.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cstdio>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const float vals[5] = {0, 1, 2, 3, 5};
    int32_t deg0[5] = {1, 2, 2, 2, 1};
    int32_t nbr0[15] = {1, -1, -1,  0, 2, -1,  1, 3, -1,  2, 4, -1,  3, -1, -1};
    hnsw_index_desc d{};
    d.vectors = vals; d.n = 5; d.d = 1; d.row_stride = 1; d.metric = HNSW_METRIC_L2; d.id_base = 0;
    d.max_degree0 = 3; d.max_degree = 1; d.max_layer = 0; d.entry_point = 0; d.deg0 = deg0; d.nbr0 = nbr0; d.upper = nullptr;
    auto g = Hnsw::Hgraph::create(d);

    bool threw = false;
    try { Hnsw::Ohnsw::remove(g, {2, 2}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // a duplicate id
    threw = false;
    try { Hnsw::Ohnsw::remove(g, {5}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // an id out of range
    hnsw_index_info inf{};
    EXPECT(hnsw_index_get_info(g.handle(), &inf) == HNSW_OK && inf.n == 5);

    const std::vector<int32_t> new_id = Hnsw::Ohnsw::remove(g, {2});
    EXPECT((new_id == std::vector<int32_t>{0, 1, -1, 2, 3}));
    EXPECT(hnsw_index_get_info(g.handle(), &inf) == HNSW_OK && inf.n == 4 && inf.entry_point == 0 && inf.max_layer == 0);
    int32_t deg[4] = {0, 0, 0, 0}, nbr[12];
    EXPECT(hnsw_index_export_layer0(g.handle(), deg, nbr) == HNSW_OK);
    const int32_t want_deg[4] = {1, 2, 2, 1};
    const int32_t want_nbr[12] = {1, -1, -1,  0, 2, -1,  3, 1, -1,  2, -1, -1};      // old node 3: its live link first, the new one after it
    for (int i = 0; i < 4; ++i) EXPECT(deg[i] == want_deg[i]);
    for (int i = 0; i < 12; ++i) EXPECT(nbr[i] == want_nbr[i]);

    // the repaired chain is searched end to end: the old node 3 (value 3) is now node 2
    const float q[1] = {2.9f};
    const auto r = Hnsw::Ohnsw::knn(g, 2, q);
    EXPECT(r.size() == 2 && r[0].node == 2 && r[1].node == 1);

    // everything leaves: the empty index
    const std::vector<int32_t> none = Hnsw::Ohnsw::remove(g, {0, 1, 2, 3});
    EXPECT((none == std::vector<int32_t>{-1, -1, -1, -1}));
    EXPECT(hnsw_index_get_info(g.handle(), &inf) == HNSW_OK && inf.n == 0);
    if (fails) return 1;
    std::printf("remove front-end ok\n");
    return 0;
}
