// Hnsw::Ohnsw::set_keys / keys_of / find_keys / knn_keyed / remove_keys / insert_keyed and Hnsw::Filter::by_keys (the C++ mirror of
// hnsw_index_set_keys ... hnsw_filter_create_by_keys) on 300 vectors built on the device: set, find, a keyed search against the plain
// one, removal by key, a keyed insert.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const int n = 300, d = 8, nq = 5, k = 4;
    std::vector<float> X((size_t)n * d), Q((size_t)nq * d);
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (float &x : X) x = next();
    for (float &x : Q) x = next();
    auto g = Hnsw::Ohnsw::build_batch_bigarray(Hnsw::Mat{X.data(), n, d}, 8, 40, 1);
    EXPECT(!Hnsw::Ohnsw::keys_info(g).first);

    // keys that a 32-bit truncation or an unsigned compare confuses: negative, the extremes, pairs 2^32 apart
    std::vector<int64_t> keys((size_t)n);
    for (int v = 0; v < n; ++v) keys[(size_t)v] = (v % 2 ? -1 : 1) * ((int64_t)(v / 2 + 1) << 32) + (v % 7);
    keys[0] = INT64_MIN; keys[1] = INT64_MAX; keys[2] = -1; keys[3] = 0;
    Hnsw::Ohnsw::set_keys(g, keys);
    const auto info = Hnsw::Ohnsw::keys_info(g);
    EXPECT(info.first && info.second == (int64_t)n * 20);
    EXPECT(Hnsw::Ohnsw::keys_of(g) == keys);
    const auto some = Hnsw::Ohnsw::keys_of(g, std::vector<int32_t>{1, 299, -1, 300, 0}, 77);
    EXPECT(some == (std::vector<int64_t>{INT64_MAX, keys[299], 77, 77, INT64_MIN}));
    const auto found = Hnsw::Ohnsw::find_keys(g, std::vector<int64_t>{keys[299], INT64_MIN, 12345, keys[17], keys[17]});
    EXPECT(found == (std::vector<int64_t>{299, 0, -1, 17, 17}));

    // a duplicate is refused naming the smallest duplicated key, and the keys stay
    std::vector<int64_t> twice(keys);
    twice[200] = twice[10];
    twice[250] = twice[5];
    bool threw = false;
    try { Hnsw::Ohnsw::set_keys(g, twice); } catch (const std::invalid_argument &e) {
        threw = std::strstr(e.what(), std::to_string(std::min(keys[10], keys[5])).c_str()) != nullptr;
    }
    EXPECT(threw);
    EXPECT(Hnsw::Ohnsw::keys_of(g) == keys);

    // the keyed search: the plain call's rows through keys_of, the same distance bits
    const Hnsw::Mat batch{Q.data(), nq, d};
    std::vector<int32_t> plain_ids;
    std::vector<float> plain_dist;
    Hnsw::detail::search(g, batch, 16, k, HNSW_FILL_OHNSW, plain_ids, plain_dist);
    const auto keyed = Hnsw::Ohnsw::knn_keyed(g, k, batch, 16);
    EXPECT(keyed.keys == Hnsw::Ohnsw::keys_of(g, plain_ids));
    EXPECT(std::memcmp(keyed.dist.data(), plain_dist.data(), sizeof(float) * nq * k) == 0);
    for (uint32_t st : keyed.stage) EXPECT(st == 0);
    // ... under a filter by keys that allows three nodes: those three, then the missing key
    const std::vector<int64_t> three{keys[7], keys[100], keys[299], keys[100]};
    {
        auto f = Hnsw::Filter::by_keys(g, three);
        EXPECT(f.count() == 3);
        const auto fk = Hnsw::Ohnsw::knn_keyed(g, k, batch, 16, &f, -5);
        for (int q = 0; q < nq; ++q) {
            int seen = 0;
            for (int j = 0; j < 3; ++j) for (int t = 0; t < 3; ++t) seen += fk.keys[(size_t)(q * k + j)] == three[(size_t)t];
            EXPECT(seen == 3 && fk.keys[(size_t)(q * k + 3)] == -5 && std::isnan(fk.dist[(size_t)(q * k + 3)]));
        }
    }

    // removal by key: the nodes of those keys leave, the other keys keep their order
    const std::vector<int64_t> gone{keys[299], keys[0], keys[150]};
    const auto new_id = Hnsw::Ohnsw::remove_keys(g, gone);
    EXPECT(new_id.size() == (size_t)n && new_id[0] == -1 && new_id[150] == -1 && new_id[299] == -1 && new_id[1] == 0 && new_id[298] == 296);
    std::vector<int64_t> left;
    for (int v = 0; v < n; ++v) if (v != 0 && v != 150 && v != 299) left.push_back(keys[(size_t)v]);
    EXPECT(Hnsw::Ohnsw::keys_of(g) == left);
    EXPECT(Hnsw::Ohnsw::find_keys(g, std::vector<int64_t>{keys[1], keys[0], keys[298]}) == (std::vector<int64_t>{0, -1, 296}));
    threw = false;
    try { Hnsw::Ohnsw::remove_keys(g, std::vector<int64_t>{keys[5], keys[0]}); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // keys[0] is gone: nothing is removed
    EXPECT(Hnsw::Ohnsw::keys_of(g) == left);

    // a keyed insert puts a removed key back; the plain insert is refused now
    threw = false;
    try { Hnsw::Ohnsw::insert(g, Hnsw::Mat{X.data(), 1, d}, 8, 40, 1); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::insert_keyed(g, Hnsw::Mat{X.data(), 2, d}, std::vector<int64_t>{keys[0], keys[5]}, 8, 40, 1); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);                                      // keys[5] is stored
    EXPECT(Hnsw::Ohnsw::insert_keyed(g, Hnsw::Mat{X.data(), 2, d}, std::vector<int64_t>{keys[0], keys[150]}, 8, 40, 1) == n - 3);
    EXPECT(Hnsw::Ohnsw::find_keys(g, std::vector<int64_t>{keys[0], keys[150]}) == (std::vector<int64_t>{n - 3, n - 2}));

    Hnsw::Ohnsw::clear_keys(g);
    EXPECT(!Hnsw::Ohnsw::keys_info(g).first);
    if (fails) return 1;
    std::printf("keys front-end ok\n");
    return 0;
}
