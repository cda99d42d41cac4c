// Hnsw::Ohnsw::diversify / knn_diverse / brute_force_diverse (the C++ mirror of hnsw_diversify_batch, hnsw_search_batch_diverse and
// hnsw_brute_force_batch_diverse) on 300 vectors built on the device: the operator against the selection rule of
// hnsw_diverse_plan.h over r and D from distance_l2 and rank from rerank; lambda = 1 against rerank; the two searches against their
// inner call followed by the operator; a filter; the refusals.
#include "../../ocaml-hnsw_amd/host/hnsw_front.hpp"
#include "../../ocaml-hnsw_amd/csrc/hnsw_diverse_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

int main() {
    const int n = 300, d = 8, k = 7, ef = 32, pool = 24, nq = 5, stride = 40;
    std::vector<float> X((size_t)n * d), Q((size_t)nq * d);
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (float &x : X) x = next();
    for (int v = 0; v < 10; ++v) std::memcpy(&X[(size_t)(200 + v) * d], &X[(size_t)v * d], d * sizeof(float));     // duplicates to push down the row
    for (float &x : Q) x = next();
    auto g = Hnsw::Ohnsw::build_batch_bigarray(Hnsw::Mat{X.data(), n, d}, 8, 40, 1);
    const Hnsw::Mat batch{Q.data(), nq, d};

    // candidates: 40 distinct nodes per query, a few entries padding
    std::vector<int32_t> cand((size_t)nq * stride);
    for (int q = 0; q < nq; ++q) for (int j = 0; j < stride; ++j) cand[(size_t)q * stride + j] = (j % 9 == 4) ? -1 : (q * 37 + j * 7) % n;

    // the operator against the rule over plain numbers: rank and r from rerank, D from distance_l2 with the stored rows as queries
    const auto ranked = Hnsw::Ohnsw::rerank(g, stride, batch, cand.data(), stride);
    for (float lambda : {0.f, 0.25f, 0.5f, 1.f}) {
        const Hnsw::Ohnsw::Diverse got = Hnsw::Ohnsw::diversify(g, k, batch, cand.data(), stride, lambda);
        for (int q = 0; q < nq; ++q) {
            std::vector<int32_t> nodes;
            std::vector<float> r;
            for (int j = 0; j < stride && ranked.first[(size_t)q * stride + j] >= 0; ++j) {
                nodes.push_back(ranked.first[(size_t)q * stride + j]);
                r.push_back(ranked.second[(size_t)q * stride + j]);
            }
            const int c = (int)nodes.size();
            std::vector<float> rows((size_t)c * d);
            for (int i = 0; i < c; ++i) std::memcpy(&rows[(size_t)i * d], &X[(size_t)nodes[(size_t)i] * d], d * sizeof(float));
            std::vector<int32_t> all((size_t)c * c);
            for (int i = 0; i < c; ++i) for (int j = 0; j < c; ++j) all[(size_t)i * c + j] = nodes[(size_t)j];
            const std::vector<float> D = Hnsw::Ohnsw::distance_l2(g, Hnsw::Mat{rows.data(), c, d}, all.data(), c);
            std::vector<int> pick((size_t)c);
            std::vector<float> div((size_t)c), m((size_t)c);
            const int picks = hnsw_diverse::select(r.data(), D.data(), c, k, lambda, pick.data(), div.data(), m.data());
            EXPECT(picks == k);
            for (int j = 0; j < picks; ++j) {
                EXPECT(got.ids[(size_t)q * k + j] == nodes[(size_t)pick[(size_t)j]]);
                EXPECT(std::memcmp(&got.dist[(size_t)q * k + j], &r[(size_t)pick[(size_t)j]], 4) == 0);
                EXPECT(std::memcmp(&got.div[(size_t)q * k + j], &div[(size_t)j], 4) == 0);
            }
            EXPECT(std::isinf(got.div[(size_t)q * k]));
        }
        if (lambda == 1.f) {
            const auto rr = Hnsw::Ohnsw::rerank(g, k, batch, cand.data(), stride);
            EXPECT(got.ids == rr.first && same_bits(got.dist, rr.second));
        }
    }

    // the searches: the inner call at k := pool, then the operator over its id rows
    std::vector<int32_t> pi;
    std::vector<float> pd;
    Hnsw::detail::search(g, batch, ef, pool, HNSW_FILL_OHNSW, pi, pd);
    const Hnsw::Ohnsw::Diverse want = Hnsw::Ohnsw::diversify(g, k, batch, pi.data(), pool, 0.25f);
    const Hnsw::Ohnsw::Diverse got = Hnsw::Ohnsw::knn_diverse(g, k, batch, pool, 0.25f, ef);
    EXPECT(got.ids == want.ids && same_bits(got.dist, want.dist) && same_bits(got.div, want.div));
    for (int q = 0; q < nq; ++q) EXPECT(got.status[(size_t)q] == 0u);

    const auto scan = Hnsw::Ohnsw::brute_force_knn(g, pool, batch);
    const Hnsw::Ohnsw::Diverse bwant = Hnsw::Ohnsw::diversify(g, k, batch, scan.first.data(), pool, 0.5f);
    const Hnsw::Ohnsw::Diverse bgot = Hnsw::Ohnsw::brute_force_diverse(g, k, batch, pool, 0.5f);
    EXPECT(bgot.ids == bwant.ids && same_bits(bgot.dist, bwant.dist) && same_bits(bgot.div, bwant.div));

    // a filter that allows three nodes: a short row, every id allowed, the rest filled
    std::vector<bool> allow((size_t)n, false);
    allow[3] = allow[100] = allow[299] = true;
    Hnsw::Filter f(g, allow);
    const Hnsw::Ohnsw::Diverse pf = Hnsw::Ohnsw::knn_diverse(g, k, batch, pool, 0.5f, ef, &f);
    for (int q = 0; q < nq; ++q) for (int j = 0; j < k; ++j) {
        const int32_t id = pf.ids[(size_t)q * k + j];
        EXPECT(j < 3 ? (id == 3 || id == 100 || id == 299) : (id == -1 && std::isnan(pf.dist[(size_t)q * k + j]) && std::isnan(pf.div[(size_t)q * k + j])));
    }

    // refused: lambda outside [0, 1] or NaN, pool > ef, pool < k, k > cand_stride
    bool threw = false;
    try { Hnsw::Ohnsw::diversify(g, k, batch, cand.data(), stride, 1.5f); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::knn_diverse(g, k, batch, pool, NAN, ef); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::knn_diverse(g, k, batch, ef + 1, 0.5f, ef); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::brute_force_diverse(g, k, batch, k - 1, 0.5f); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { Hnsw::Ohnsw::diversify(g, stride + 1, batch, cand.data(), stride, 0.5f); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);

    if (fails) return 1;
    std::printf("diverse front-end ok\n");
    return 0;
}
