// Hnsw::Cursor, Hnsw::Ohnsw::knn_after / brute_force_after (the C++ mirror of hnsw_search_batch_after / hnsw_brute_force_batch_after)
// on 300 vectors built on the device: the pages of the exact form, concatenated, against the order (ord(distance), id) over
// distance_l2; the graph form's first page against the plain search; its pages disjoint and ascending; a filter; the refusals.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"
#include "../../ocaml-hnsw_amd/csrc/hnsw_after_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    const int n = 300, d = 8, k = 7, ef = 16, nq = 5;
    std::vector<float> X((size_t)n * d), Q((size_t)nq * d);
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (float &x : X) x = next();
    for (float &x : Q) x = next();
    auto g = Hnsw::Ohnsw::build_batch_bigarray(Hnsw::Mat{X.data(), n, d}, 8, 40, 1);
    const Hnsw::Mat batch{Q.data(), nq, d};

    // the paged order from public calls: D over every (query, node) pair, sorted by (ord(D), id)
    std::vector<int32_t> everyone((size_t)nq * n);
    for (int q = 0; q < nq; ++q) for (int v = 0; v < n; ++v) everyone[(size_t)q * n + v] = v;
    const std::vector<float> D = Hnsw::Ohnsw::distance_l2(g, batch, everyone.data(), n);
    std::vector<std::vector<uint64_t>> order((size_t)nq);
    for (int q = 0; q < nq; ++q) {
        for (int v = 0; v < n; ++v) order[(size_t)q].push_back(hnsw_after::word(D[(size_t)q * n + v], (uint32_t)v));
        std::sort(order[(size_t)q].begin(), order[(size_t)q].end());
    }

    // the exact form: pages until every row is short; their concatenation is the order, bit for bit
    std::vector<std::vector<uint64_t>> got((size_t)nq);
    std::vector<Hnsw::Cursor> cur;
    for (int page = 0; page < n / k + 2; ++page) {
        const Hnsw::Ohnsw::Paged p = Hnsw::Ohnsw::brute_force_after(g, k, batch, cur);
        bool all_short = true;
        for (int q = 0; q < nq; ++q) {
            int real = 0;
            for (int j = 0; j < k; ++j) {
                const int32_t id = p.ids[(size_t)q * k + j];
                if (id < 0) { EXPECT(std::isnan(p.dist[(size_t)q * k + j])); continue; }
                EXPECT(real == j);      // the real entries come first
                got[(size_t)q].push_back(hnsw_after::word(p.dist[(size_t)q * k + j], (uint32_t)id));
                ++real;
            }
            const Hnsw::Cursor before = cur.empty() ? Hnsw::Cursor::start() : cur[(size_t)q];
            if (real) EXPECT(p.next[(size_t)q].id == p.ids[(size_t)q * k + real - 1] &&
                             std::memcmp(&p.next[(size_t)q].dist, &p.dist[(size_t)q * k + real - 1], 4) == 0);
            else EXPECT(p.next[(size_t)q].id == before.id && std::memcmp(&p.next[(size_t)q].dist, &before.dist, 4) == 0);
            all_short = all_short && real < k;
        }
        cur = p.next;
        if (all_short) break;
    }
    for (int q = 0; q < nq; ++q) EXPECT(got[(size_t)q] == order[(size_t)q]);

    // the graph form: page 0 from the start cursor is the plain search's row (distinct distances), later pages are disjoint and ascending
    std::vector<int32_t> pi;
    std::vector<float> pd;
    Hnsw::detail::search(g, batch, ef, k, HNSW_FILL_OHNSW, pi, pd);
    Hnsw::Ohnsw::Paged p0 = Hnsw::Ohnsw::knn_after(g, k, batch, {}, ef);
    EXPECT(p0.ids == pi && std::memcmp(p0.dist.data(), pd.data(), pd.size() * 4) == 0);
    for (int q = 0; q < nq; ++q) EXPECT(p0.stage[(size_t)q] == 0u);
    std::vector<std::set<int32_t>> seen((size_t)nq);
    std::vector<uint64_t> last((size_t)nq, 0);
    Hnsw::Ohnsw::Paged p = p0;
    for (int page = 0; page < 5; ++page) {
        for (int q = 0; q < nq; ++q) for (int j = 0; j < k; ++j) {
            const int32_t id = p.ids[(size_t)q * k + j];
            EXPECT(id >= 0 && seen[(size_t)q].insert(id).second);
            const uint64_t w = hnsw_after::word(p.dist[(size_t)q * k + j], (uint32_t)id);
            EXPECT(w > last[(size_t)q]);
            last[(size_t)q] = w;
        }
        p = Hnsw::Ohnsw::knn_after(g, k, batch, p.next, ef);
    }

    // a filter that allows three nodes: the exact stage, a short row, every id allowed
    std::vector<bool> allow((size_t)n, false);
    allow[3] = allow[100] = allow[299] = true;
    Hnsw::Filter f(g, allow);
    const Hnsw::Ohnsw::Paged pf = Hnsw::Ohnsw::knn_after(g, k, batch, {}, ef, &f);
    for (int q = 0; q < nq; ++q) {
        EXPECT(pf.stage[(size_t)q] == Hnsw::Ohnsw::Paged::exact_stage);
        for (int j = 0; j < k; ++j) {
            const int32_t id = pf.ids[(size_t)q * k + j];
            EXPECT(j < 3 ? (id == 3 || id == 100 || id == 299) : id == -1);
        }
    }

    // refused: a NaN cursor, a cursor count that is not nq, k > ef
    bool threw = false;
    try { Hnsw::Ohnsw::knn_after(g, k, batch, std::vector<Hnsw::Cursor>((size_t)nq, Hnsw::Cursor(NAN, 0)), ef); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::brute_force_after(g, k, batch, std::vector<Hnsw::Cursor>(2)); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::knn_after(g, k, batch, {}, k - 1); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    if (fails) return 1;
    std::printf("paged front-end ok\n");
    return 0;
}
