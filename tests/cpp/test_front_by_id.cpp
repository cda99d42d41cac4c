// Hnsw::Ohnsw::knn_by_id / knn_by_key / brute_force_by_id / knn_graph (the C++ mirror of hnsw_search_batch_by_id ... hnsw_knn_graph)
// on 300 vectors built on the device: the search by id against the plain search over rows(ids), the drop-self rule restated on the
// host, keys, the exact form, the graph, and the refusals.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the definition on one batch: rows [nq][k + 1] with the first entry equal to self (or the last one) removed
static void drop_self(const std::vector<int32_t> &ri, const std::vector<float> &rd, const std::vector<int32_t> &self, int k,
                      std::vector<int32_t> &oi, std::vector<float> &od) {
    oi.clear(); od.clear();
    for (size_t q = 0; q < self.size(); ++q) {
        int p = k;
        for (int j = 0; j <= k; ++j) if (ri[q * (size_t)(k + 1) + (size_t)j] == self[q]) { p = j; break; }
        for (int j = 0; j <= k; ++j) if (j != p) { oi.push_back(ri[q * (size_t)(k + 1) + (size_t)j]); od.push_back(rd[q * (size_t)(k + 1) + (size_t)j]); }
    }
}
static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0;
}

int main() {
    const int n = 300, d = 8, k = 4, ef = 16;
    std::vector<float> X((size_t)n * d);
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (float &x : X) x = next();
    auto g = Hnsw::Ohnsw::build_batch_bigarray(Hnsw::Mat{X.data(), n, d}, 8, 40, 1);

    const std::vector<int32_t> ids{0, 299, 17, 150, 17, 64};
    const std::vector<float> Q = Hnsw::Ohnsw::rows(g, std::vector<int64_t>(ids.begin(), ids.end()));
    const Hnsw::Mat batch{Q.data(), (int64_t)ids.size(), d};

    // exclude_self = false: the plain search over the stored rows
    std::vector<int32_t> pi, wi;
    std::vector<float> pd, wd;
    Hnsw::detail::search(g, batch, ef, k, HNSW_FILL_OHNSW, pi, pd);
    const auto keep = Hnsw::Ohnsw::knn_by_id(g, k, ids, ef, false);
    EXPECT(keep.first == pi && same_bits(keep.second, pd));
    // exclude_self: that search k + 1 wide with self removed
    Hnsw::detail::search(g, batch, ef, k + 1, HNSW_FILL_OHNSW, pi, pd);
    drop_self(pi, pd, ids, k, wi, wd);
    const auto drop = Hnsw::Ohnsw::knn_by_id(g, k, ids, ef);
    EXPECT(drop.first == wi && same_bits(drop.second, wd));
    for (size_t q = 0; q < ids.size(); ++q) for (int j = 0; j < k; ++j) EXPECT(drop.first[q * k + (size_t)j] != ids[q]);
    // ef == k (the default): the inner call runs with ef' = k + 1
    Hnsw::detail::search(g, batch, k + 1, k + 1, HNSW_FILL_OHNSW, pi, pd);
    drop_self(pi, pd, ids, k, wi, wd);
    const auto tight = Hnsw::Ohnsw::knn_by_id(g, k, ids);
    EXPECT(tight.first == wi && same_bits(tight.second, wd));

    // the exact form against brute_force_knn over the rows
    const auto scan = Hnsw::Ohnsw::brute_force_knn(g, k + 1, batch);
    drop_self(scan.first, scan.second, ids, k, wi, wd);
    const auto exact = Hnsw::Ohnsw::brute_force_by_id(g, k, ids);
    EXPECT(exact.first == wi && same_bits(exact.second, wd));

    // the graph: every node's row of the one call
    std::vector<int32_t> everyone((size_t)n);
    for (int v = 0; v < n; ++v) everyone[(size_t)v] = v;
    const auto all = Hnsw::Ohnsw::knn_by_id(g, k, everyone, ef);
    Hnsw::check(hnsw_index_set_option(g.handle(), "graph_chunk_rows", 77));
    const auto graph = Hnsw::Ohnsw::knn_graph(g, k, ef);
    EXPECT(graph.first == all.first && same_bits(graph.second, all.second));
    const auto xgraph = Hnsw::Ohnsw::knn_graph(g, k, 0, true);
    const auto xall = Hnsw::Ohnsw::brute_force_by_id(g, k, everyone);
    EXPECT(xgraph.first == xall.first && same_bits(xgraph.second, xall.second));

    // keys: the by-id rows through keys_of, the same distance bits; an absent key and a handle without keys are refused
    bool threw = false;
    try { Hnsw::Ohnsw::knn_by_key(g, k, std::vector<int64_t>{5}, ef); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    std::vector<int64_t> keys((size_t)n);
    for (int v = 0; v < n; ++v) keys[(size_t)v] = (v % 2 ? -1 : 1) * ((int64_t)(v / 2 + 1) << 32) + (v % 7);
    keys[0] = INT64_MIN; keys[299] = INT64_MAX;
    Hnsw::Ohnsw::set_keys(g, keys);
    std::vector<int64_t> qk;
    for (int32_t v : ids) qk.push_back(keys[(size_t)v]);
    const auto keyed = Hnsw::Ohnsw::knn_by_key(g, k, qk, ef, true, -5);
    EXPECT(keyed.first == Hnsw::Ohnsw::keys_of(g, drop.first, -5) && same_bits(keyed.second, drop.second));
    threw = false;
    try { Hnsw::Ohnsw::knn_by_key(g, k, std::vector<int64_t>{keys[3], 12345}, ef); } catch (const std::invalid_argument &e) {
        threw = std::strstr(e.what(), "keys[1]=12345") != nullptr;
    }
    EXPECT(threw);

    // an id out of range is refused naming the first by position
    threw = false;
    try { Hnsw::Ohnsw::knn_by_id(g, k, std::vector<int32_t>{5, 300, -1}, ef); } catch (const std::invalid_argument &e) {
        threw = std::strstr(e.what(), "ids[1]=300") != nullptr;
    }
    EXPECT(threw);
    EXPECT(Hnsw::Ohnsw::knn_by_id(g, k, std::vector<int32_t>{}, ef).first.empty());

    if (fails) return 1;
    std::printf("by-id front-end ok\n");
    return 0;
}
