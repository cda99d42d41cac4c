// Hnsw::Ohnsw::mark_deleted / unmark_deleted / deleted_count / compact and the Filter overloads of range_search / brute_force_range
// (the C++ mirror of hnsw_index_mark_deleted ... and of the _filtered range calls) on the reference's five-node example values
// (lib/ohnsw.ml:617-643: values [0;1;2;3;5], |a-b| distance == L2 at d = 1), linked as a chain 0 - 1 - 2 - 3 - 4.
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
    const float q[1] = {2.1f};
    const Hnsw::Mat Q{q, 1, 1};

    // an allow-mask and a radius together: nodes 1, 2, 3 are within 1.5 of 2.1; the filter leaves node 2 out
    {
        Hnsw::Filter f(g, std::vector<bool>{true, true, false, true, true});
        const auto h = Hnsw::Ohnsw::range_search(g, f, 1.5f, Q, 4).fetch();
        EXPECT(h.lims[1] == 2 && h.ids[0] == 3 && h.ids[1] == 1);
        const auto all = Hnsw::Ohnsw::range_search(g, 1.5f, Q, 4).fetch();
        EXPECT(all.lims[1] == 3 && all.ids[0] == 2 && h.stage[0] == all.stage[0] && h.nhops[0] == all.nhops[0]);
        const auto b = Hnsw::Ohnsw::brute_force_range(g, f, 1.5f, Q).fetch();
        EXPECT(b.lims[1] == 2 && b.ids[0] == 3 && b.ids[1] == 1 && b.ndist[0] == 4 && b.stage[0] == Hnsw::RangeResult::exact_stage);
    }

    bool threw = false;
    try { Hnsw::Ohnsw::mark_deleted(g, {2, 2}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // a duplicate id
    threw = false;
    try { Hnsw::Ohnsw::mark_deleted(g, {5}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // an id out of range
    EXPECT(Hnsw::Ohnsw::deleted_count(g) == 0);

    // node 2 is marked: it stays in the graph (the walk from 0 reaches 3 through it) and is never returned
    Hnsw::Ohnsw::mark_deleted(g, {2});
    EXPECT(Hnsw::Ohnsw::deleted_count(g) == 1);
    EXPECT((Hnsw::Ohnsw::deleted_mask(g) == std::vector<bool>{false, false, true, false, false}));
    auto r = Hnsw::Ohnsw::knn(g, 2, q);
    EXPECT(r.size() == 2 && r[0].node == 3 && r[1].node == 1);
    const auto bf = Hnsw::Ohnsw::brute_force_knn(g, 5, Q);
    EXPECT(bf.first[0] == 3 && bf.first[1] == 1 && bf.first[2] == 0 && bf.first[3] == 4 && bf.first[4] == -1);
    {
        const auto h = Hnsw::Ohnsw::range_search(g, 1.5f, Q, 4).fetch();
        EXPECT(h.lims[1] == 2 && h.ids[0] == 3 && h.ids[1] == 1);
        Hnsw::Filter f(g, std::vector<bool>{false, true, true, true, false});        // made under the mark: ANDed with the live nodes
        EXPECT(f.count() == 2);
    }
    hnsw_index_info inf{};
    EXPECT(hnsw_index_get_info(g.handle(), &inf) == HNSW_OK && inf.n == 5);      // n stays the stored count

    // unmarked again: the plain answer
    Hnsw::Ohnsw::unmark_deleted(g, {2});
    EXPECT(Hnsw::Ohnsw::deleted_count(g) == 0);
    r = Hnsw::Ohnsw::knn(g, 2, q);
    EXPECT(r.size() == 2 && r[0].node == 2 && r[1].node == 3);

    // compact = remove of the marked nodes
    Hnsw::Ohnsw::mark_deleted(g, {2});
    const std::vector<int32_t> new_id = Hnsw::Ohnsw::compact(g);
    EXPECT((new_id == std::vector<int32_t>{0, 1, -1, 2, 3}));
    EXPECT(Hnsw::Ohnsw::deleted_count(g) == 0);
    EXPECT(hnsw_index_get_info(g.handle(), &inf) == HNSW_OK && inf.n == 4);
    r = Hnsw::Ohnsw::knn(g, 2, q);
    EXPECT(r.size() == 2 && r[0].node == 2 && r[1].node == 1);                    // old node 3 is node 2 now
    EXPECT((Hnsw::Ohnsw::compact(g) == std::vector<int32_t>{0, 1, 2, 3}));        // nothing marked: the identity
    if (fails) return 1;
    std::printf("soft delete front-end ok\n");
    return 0;
}
