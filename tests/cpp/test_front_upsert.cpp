// Hnsw::Ohnsw::upsert_keyed / update (the C++ mirror of hnsw_index_upsert_keyed / hnsw_index_update) on 300 vectors built on the
// device: a mixed call against remove_keys + insert_keyed on a twin, the outputs, a refused call that leaves the index as it was,
// the call by id on a twin without keys.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"

#include <cstdio>
#include <cstring>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const int n = 300, d = 8, nq = 5, k = 4, m = 6;
    std::vector<float> X((size_t)n * d), Q((size_t)nq * d), Y((size_t)m * d);
    uint32_t s = 4321u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (float &x : X) x = next();
    for (float &x : Q) x = next();
    for (float &x : Y) x = next();
    const Hnsw::Mat data{X.data(), n, d}, batch{Q.data(), nq, d}, fresh{Y.data(), m, d};
    auto a = Hnsw::Ohnsw::build_batch_bigarray(data, 8, 40, 1);
    auto b = Hnsw::Ohnsw::build_batch_bigarray(data, 8, 40, 1);
    std::vector<int64_t> keys((size_t)n);
    for (int v = 0; v < n; ++v) keys[(size_t)v] = (v % 2 ? -1 : 1) * ((int64_t)(v / 2 + 1) << 32) + (v % 7);
    Hnsw::Ohnsw::set_keys(a, keys);
    Hnsw::Ohnsw::set_keys(b, keys);

    // four stored keys and two new ones, scattered
    const std::vector<int64_t> call{keys[299], 5, keys[0], keys[150], -6, keys[17]};
    const auto up = Hnsw::Ohnsw::upsert_keyed(a, fresh, call, 8, 40, 1);
    EXPECT(up.replaced == (std::vector<uint8_t>{1, 0, 1, 1, 0, 1}));
    const auto new_id = Hnsw::Ohnsw::remove_keys(b, std::vector<int64_t>{keys[299], keys[0], keys[150], keys[17]});
    EXPECT(up.new_id == new_id);
    EXPECT(Hnsw::Ohnsw::insert_keyed(b, fresh, call, 8, 40, 1) == n - 4);
    EXPECT(Hnsw::Ohnsw::find_keys(a, call) == (std::vector<int64_t>{n - 4, n - 3, n - 2, n - 1, n, n + 1}));
    EXPECT(Hnsw::Ohnsw::keys_of(a) == Hnsw::Ohnsw::keys_of(b));
    EXPECT(Hnsw::Ohnsw::rows(a) == Hnsw::Ohnsw::rows(b));
    const auto ka = Hnsw::Ohnsw::knn_keyed(a, k, batch, 16), kb = Hnsw::Ohnsw::knn_keyed(b, k, batch, 16);
    EXPECT(ka.keys == kb.keys);
    EXPECT(std::memcmp(ka.dist.data(), kb.dist.data(), sizeof(float) * nq * k) == 0);

    // a key twice in the call: refused naming it, the index as it was
    bool threw = false;
    try { Hnsw::Ohnsw::upsert_keyed(a, Hnsw::Mat{Y.data(), 3, d}, std::vector<int64_t>{keys[5], 99, keys[5]}, 8, 40, 1); } catch (const std::invalid_argument &e) {
        threw = std::strstr(e.what(), std::to_string(keys[5]).c_str()) != nullptr;
    }
    EXPECT(threw);
    EXPECT(Hnsw::Ohnsw::keys_of(a) == Hnsw::Ohnsw::keys_of(b));
    // update() is refused on the keyed handle ...
    threw = false;
    try { Hnsw::Ohnsw::update(a, std::vector<int64_t>{3}, Hnsw::Mat{Y.data(), 1, d}, 8, 40, 1); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    // ... and on twins without keys it is remove + insert
    Hnsw::Ohnsw::clear_keys(a);
    Hnsw::Ohnsw::clear_keys(b);
    const std::vector<int64_t> ids{7, 200, 8};
    const auto moved = Hnsw::Ohnsw::update(a, ids, Hnsw::Mat{Y.data(), 3, d}, 8, 40, 1);
    EXPECT(moved == Hnsw::Ohnsw::remove(b, ids));
    Hnsw::Ohnsw::insert(b, Hnsw::Mat{Y.data(), 3, d}, 8, 40, 1);
    EXPECT(Hnsw::Ohnsw::rows(a) == Hnsw::Ohnsw::rows(b));
    std::vector<int32_t> ia, ib;
    std::vector<float> da, db;
    Hnsw::detail::search(a, batch, 16, k, HNSW_FILL_OHNSW, ia, da);
    Hnsw::detail::search(b, batch, 16, k, HNSW_FILL_OHNSW, ib, db);
    EXPECT(ia == ib && std::memcmp(da.data(), db.data(), sizeof(float) * nq * k) == 0);
    if (fails) return 1;
    std::printf("upsert front-end ok\n");
    return 0;
}
