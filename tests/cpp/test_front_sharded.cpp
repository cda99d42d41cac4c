// Hnsw::Sharded and Hnsw::merge_lists (the C++ mirror of hnsw_sharded_* and hnsw_merge_lists) on the reference's five-node example
// values (lib/ohnsw.ml:617-643: values [0;1;2;3;5], |a-b| distance == L2 at d = 1), cut into two shards of unequal size on one
// device: rows {0, 1, 2} linked 0 - 1 - 2 and rows {3, 5} linked 0 - 1, each with LOCAL ids.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const float a_vals[3] = {0, 1, 2}, b_vals[2] = {3, 5};
    int32_t a_deg[3] = {1, 2, 1}, a_nbr[6] = {1, -1, 0, 2, 1, -1};
    int32_t b_deg[2] = {1, 1}, b_nbr[4] = {1, -1, 0, -1};
    hnsw_index_desc a{}, b{};
    a.vectors = a_vals; a.n = 3; a.d = 1; a.row_stride = 1; a.metric = HNSW_METRIC_L2; a.id_base = 0;
    a.max_degree0 = 2; a.max_degree = 1; a.max_layer = 0; a.entry_point = 0; a.deg0 = a_deg; a.nbr0 = a_nbr; a.upper = nullptr;
    b = a;
    b.vectors = b_vals; b.n = 2; b.deg0 = b_deg; b.nbr0 = b_nbr;
    auto s = Hnsw::Sharded::create({&a, &b}, {0, 0});
    EXPECT(s.num_shards() == 2);
    EXPECT(s.shard(0).second == 0 && s.shard(1).second == 3);                     // the running sum of the shards' n
    const auto inf = s.info();
    EXPECT(inf.n == 5 && inf.d == 1 && inf.metric == HNSW_METRIC_L2 && inf.id_base == 0 && inf.device_bytes > 0);

    const float q[1] = {2.1f};
    const Hnsw::Mat Q{q, 1, 1};
    const auto r = s.knn_batch(Q, 3, 3);                                           // 2 (0.1), 3 (0.9), 1 (1.1): global ids
    EXPECT(r.first[0] == 2 && r.first[1] == 3 && r.first[2] == 1);
    EXPECT(r.second[0] < r.second[1] && r.second[1] < r.second[2]);
    const auto bf = s.brute_force_knn(6, Q);                                       // all five rows, then the fill
    EXPECT(bf.first[0] == 2 && bf.first[1] == 3 && bf.first[2] == 1 && bf.first[3] == 0 && bf.first[4] == 4 && bf.first[5] == -1);
    EXPECT(std::isnan(bf.second[5]));

    // a borrowed shard is not grown on its own; an option reaches every shard
    hnsw_build_params bp{};
    bp.num_connections = 2; bp.num_nodes_search_construction = 4; bp.metric = HNSW_METRIC_L2;
    const float more[1] = {7};
    EXPECT(hnsw_index_insert(s.shard(1).first, more, 1, 1, &bp) == HNSW_ERR_BAD_ARG);
    s.set_option("refine", 4);
    bool threw = false;
    try { s.set_option("refine", 5000); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { s.knn_batch(Q, 3, 3, HNSW_FILL_BA, HNSW_SEM_FUNCTOR_NEAREST_K); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    // the merge alone: two lists of two, equal distances across the lists go by global id, the padding is skipped
    const auto m = Hnsw::merge_lists({0, 1, 0, -1}, {1.f, 2.f, 1.f, 0.f}, {0, 10}, 1, 2, 4, 0, HNSW_FILL_BA);
    EXPECT(m.first[0] == 0 && m.first[1] == 10 && m.first[2] == 1 && m.first[3] == -1);
    EXPECT(m.second[0] == 1.f && m.second[1] == 1.f && m.second[2] == 2.f && std::isinf(m.second[3]));
    if (fails) return 1;
    std::printf("sharded front-end ok\n");
    return 0;
}
