// Hnsw::ShardedFilter, Hnsw::Sharded::knn_filtered / range_search / brute_force_range, Hnsw::ShardedRangeResult and
// Hnsw::merge_segments (the C++ mirror of hnsw_sharded_filter_*, hnsw_sharded_search_batch_filtered, hnsw_sharded_range_* and
// hnsw_merge_segments) on the five-node example of test_front_sharded.cpp: values [0;1;2;3;5] at d = 1, cut into the shards
// {0, 1, 2} and {3, 5} on one device, so the shard bound (global row 3) is no multiple of 32.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>
#include <memory>

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
    auto s = std::make_unique<Hnsw::Sharded>(Hnsw::Sharded::create({&a, &b}, {0, 0}));
    const float q[1] = {2.1f};                                                     // distances: 2.1, 1.1, 0.1 | 0.9, 2.9
    const Hnsw::Mat Q{q, 1, 1};

    // a filter over the global rows: row 1 is out; shard 0's part is {1, 0, 1}, shard 1's {1, 1}
    Hnsw::ShardedFilter f(*s, {true, false, true, true, true});
    EXPECT(f.count() == 4);
    int64_t c0 = 0, c1 = 0;
    EXPECT(hnsw_filter_count(f.part(0), &c0) == HNSW_OK && c0 == 2);
    EXPECT(hnsw_filter_count(f.part(1), &c1) == HNSW_OK && c1 == 2);
    uint32_t w0[2] = {0, 0}, w1[2] = {0, 0};
    EXPECT(hnsw_filter_bits(f.part(0), w0) == HNSW_OK && w0[0] == 5u);
    EXPECT(hnsw_filter_bits(f.part(1), w1) == HNSW_OK && w1[0] == 3u);

    // filtered k-NN: 2 (0.1), 3 (0.9), 0 (2.1); both parts allow fewer than k = 3 nodes, so both shards took their exact stage
    const auto r = s->knn_filtered(f, Q, 3, 3);
    EXPECT(r.ids[0] == 2 && r.ids[1] == 3 && r.ids[2] == 0);
    EXPECT(r.dist[0] < r.dist[1] && r.dist[1] < r.dist[2]);
    EXPECT(r.stage[0] == Hnsw::Sharded::Filtered::exact_stage);
    const auto r5 = s->knn_filtered(f, Q, 5, 5, HNSW_FILL_BA);                     // four allowed rows, then the fill
    EXPECT(r5.ids[3] == 4 && r5.ids[4] == -1 && std::isinf(r5.dist[4]));

    // range search, exact and graph form: rows 2 (0.1) and 3 (0.9) lie within 1.0, one in each shard
    for (int form = 0; form < 2; ++form) {
        const auto h = (form ? s->range_search(1.0f, Q, 4) : s->brute_force_range(1.0f, Q)).fetch();
        EXPECT(h.lims.size() == 2 && h.lims[0] == 0 && h.lims[1] == 2);
        EXPECT(h.ids.size() == 2 && h.ids[0] == 2 && h.ids[1] == 3 && h.dist[0] < h.dist[1] && h.dist[1] <= 1.0f);
        EXPECT(h.ndist[0] > 0);
    }
    Hnsw::ShardedFilter no2(*s, {true, true, false, true, true});
    const auto hf = s->brute_force_range(1.0f, Q, &no2).fetch();                   // under a mask without row 2
    EXPECT(hf.lims[1] == 1 && hf.ids[0] == 3);
    EXPECT(hf.stage[0] == Hnsw::ShardedRangeResult::exact_stage);
    const auto none = s->brute_force_range(0.01f, Q);                              // nothing in range: a valid empty result
    EXPECT(none.nq() == 1 && none.total() == 0);

    // a filter of another Sharded is refused; so is the functor's nearest-k rule
    auto t = Hnsw::Sharded::create({&a, &b}, {0, 0});
    Hnsw::ShardedFilter other(t, {true, true, true, true, true});
    bool threw = false;
    try { s->knn_filtered(other, Q, 3, 3); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { s->brute_force_range(1.0f, Q, &other); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { s->knn_filtered(f, Q, 3, 3, HNSW_FILL_OHNSW, HNSW_SEM_FUNCTOR_NEAREST_K); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::ShardedFilter bad(*s, {true, true}); } catch (const std::invalid_argument &) { threw = true; }     // n_bits is not n
    EXPECT(threw);

    // a result outlives its sharded index
    auto kept = s->brute_force_range(3.0f, Q);
    { Hnsw::ShardedFilter gone(std::move(f)); }
    { Hnsw::ShardedFilter gone(std::move(no2)); }
    s.reset();
    const auto hk = kept.fetch();
    EXPECT(hk.ids.size() == 5 && hk.ids[0] == 2 && hk.ids[1] == 3 && hk.ids[2] == 1 && hk.ids[3] == 0 && hk.ids[4] == 4);

    // the segment merge alone: equal distances across the lists go by global id, an empty segment in between
    const auto m = Hnsw::merge_segments({{0, 2, 2}, {0, 1, 2}}, {{0, 1}, {0, 3}}, {{1.f, 2.f}, {1.f, -1.f}}, {0, 10}).fetch();
    EXPECT(m.lims[0] == 0 && m.lims[1] == 3 && m.lims[2] == 4);
    EXPECT(m.ids[0] == 0 && m.ids[1] == 10 && m.ids[2] == 1 && m.ids[3] == 13);
    EXPECT(m.dist[0] == 1.f && m.dist[1] == 1.f && m.dist[2] == 2.f && m.dist[3] == -1.f);
    EXPECT(m.ndist[0] == 0 && m.stage[1] == 0);
    threw = false;
    try { Hnsw::merge_segments({{0, 1}}, {{0}}, {{1.f}}, {0, 0}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    if (fails) return 1;
    std::printf("sharded query front-end ok\n");
    return 0;
}
