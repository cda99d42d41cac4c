// The arithmetic of the diversified searches that is plain numbers (ocaml-hnsw_amd/csrc/hnsw_diverse_plan.h) against its definitions:
//   check_args   every refusal of the operator's plain numbers, with its code, and what passes;
//   mu_of, score three rounded float32 operations: against the same expression evaluated in double and rounded after every step
//                (a fused multiply-add would round once and differ on the cases chosen here);
//   score_word   ascending words = ascending g as IEEE values, -0 and +0 one word;
//   pick_word    (g, rank) ascending, the slot recoverable;
//   slots_for, lds_bytes  powers of two from 64 on; 20 bytes a slot and 256;
//   select       the greedy rule against a naive restatement (floats compared with <, ties by rank) over random and heavily tied
//                inputs, lambda in {0, 0.25, 0.5, 1}, k from 1 to c.
// A host program: built with the host compiler, and a second time under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../ocaml-hnsw_amd/csrc/hnsw_diverse_plan.h"

#include <cfloat>
#include <cstdio>
#include <vector>

using namespace hnsw_diverse;

static long cases = 0, differ = 0;
#define CHECK(c) do { ++cases; if (!(c)) { if (differ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++differ; } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// g with every step rounded by hand: the products and the difference in double (exact for float operands: 48 and 49 bits),
// each rounded to float on its own
static float score_by_hand(float lambda, float mu, float r, float m) {
    volatile float a = (float)((double)lambda * (double)r);
    volatile float b = (float)((double)mu * (double)m);
    return (float)((double)a - (double)b);
}

// the rule again, naively: floats compared as floats, the first candidate in rank order among the smallest g
static int naive_select(const std::vector<float> &r, const std::vector<float> &D, int c, int k, float lambda, std::vector<int> &pick,
                        std::vector<float> &div) {
    const float mu = 1.0f - lambda;
    std::vector<char> done((size_t)c, 0);
    pick.clear(); div.clear();
    for (int j = 0; j < k && j < c; ++j) {
        int best = -1;
        float best_g = 0.f, best_m = 0.f;
        if (j == 0) { best = 0; best_m = INFINITY; }
        else for (int v = 0; v < c; ++v) {
            if (done[(size_t)v]) continue;
            float m = INFINITY;
            for (int s : pick) m = D[(size_t)s * c + v] < m ? D[(size_t)s * c + v] : m;
            const float g = score_by_hand(lambda, mu, r[(size_t)v], m);
            if (best < 0 || g < best_g) { best = v; best_g = g; best_m = m; }
        }
        pick.push_back(best); div.push_back(best_m);
        done[(size_t)best] = 1;
    }
    return (int)pick.size();
}

int main() {
    const char *why = nullptr;
    // ---- check_args
    CHECK(check_args(1, 8, 3, HNSW_FILL_OHNSW, 0.5f, &why) == HNSW_OK && why == nullptr);
    CHECK(check_args(0, 1, 1, HNSW_FILL_BA, 0.0f, &why) == HNSW_OK);
    CHECK(check_args(5, 1024, 1024, HNSW_FILL_BA, 1.0f, &why) == HNSW_OK);
    CHECK(check_args(1, 0, 1, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, -3, 1, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 1025, 1, 0, 0.5f, &why) == HNSW_ERR_UNSUPPORTED && why);
    CHECK(check_args(1, 8, 0, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 9, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 2, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, -1, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 0, NAN, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 0, -0.1f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 0, 1.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 0, INFINITY, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(1, 8, 3, 0, -0.0f, &why) == HNSW_OK);                     // -0 is 0
    CHECK(check_args(-1, 8, 3, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(check_args(0x80000000LL, 8, 3, 0, 0.5f, &why) == HNSW_ERR_BAD_ARG && why);
    CHECK(lambda_ok(0.f) && lambda_ok(1.f) && !lambda_ok(bits_float(0x3F800001u)) && !lambda_ok(bits_float(0x80000001u)));

    // ---- mu and g: three rounded operations
    CHECK(float_bits(mu_of(0.25f)) == float_bits(0.75f) && mu_of(1.f) == 0.f && mu_of(0.f) == 1.f);
    CHECK(float_bits(mu_of(0.1f)) == float_bits((float)(1.0 - (double)0.1f)));
    long fused_would_differ = 0;
    for (int i = 0; i < 300000; ++i) {
        const float lambda = (float)(rnd() % 1025u) / 1024.0f * (rnd() & 1u ? 1.0f : 0.999f);
        const float r = bits_float(0x3F000000u + (rnd() & 0x01FFFFFFu)), m = bits_float(0x3F000000u + (rnd() & 0x01FFFFFFu));
        const float mu = mu_of(lambda);
        const float g = score(lambda, mu, r, m), h = score_by_hand(lambda, mu, r, m);
        CHECK(float_bits(g) == float_bits(h));
        fused_would_differ += float_bits(std::fmaf(lambda, r, -(mu * m))) != float_bits(h);
    }
    CHECK(fused_would_differ > 1000);           // (the sweep can tell the two apart)
    // negative relevances and pair distances (inner product), zeros, infinities
    for (float r : {-2.5f, -0.f, 0.f, 1.f, 3.25f, FLT_MAX}) for (float m : {-1.5f, -0.f, 0.f, 0.75f, INFINITY}) for (float l : {0.f, 0.25f, 0.5f, 1.f}) {
        const float g = score(l, mu_of(l), r, m), h = score_by_hand(l, mu_of(l), r, m);
        CHECK(float_bits(g) == float_bits(h) || (g != g && h != h));
    }

    // ---- score_word: ascending words = ascending values, the two zeros one word
    std::vector<float> sweep;
    sweep.push_back(-INFINITY);
    for (uint32_t b = 0xFF7FFFFFu; b > 0x80000000u; b -= (b - 0x80000000u > 40000u ? 39989u : 1u)) sweep.push_back(bits_float(b));
    sweep.push_back(0.f);
    for (uint32_t b = 1u; b < 0x7F800000u; b += (0x7F800000u - b > 40000u && b > 64u ? 39989u : 1u)) sweep.push_back(bits_float(b));
    sweep.push_back(INFINITY);
    for (size_t i = 0; i + 1 < sweep.size(); ++i) CHECK(score_word(sweep[i]) < score_word(sweep[i + 1]));
    CHECK(score_word(-0.f) == score_word(0.f));
    // (the word a -0 kept apart would take stays unused)
    CHECK(score_word(bits_float(0x80000001u)) + 2u == score_word(0.f) && score_word(0.f) + 1u == score_word(bits_float(1u)));

    // ---- pick_word: (g, rank) ascending, the slot along
    for (int i = 0; i < 100000; ++i) {
        const float g1 = bits_float(0x3F800000u + rnd() % 3u) * (rnd() & 1u ? 1.f : -1.f), g2 = bits_float(0x3F800000u + rnd() % 3u) * (rnd() & 1u ? 1.f : -1.f);
        const uint32_t r1 = rnd() % 1024u, r2 = rnd() % 1024u, s1 = rnd() % 1024u, s2 = rnd() % 1024u;
        const uint64_t w1 = pick_word(g1, r1, s1), w2 = pick_word(g2, r2, s2);
        if (r1 != r2 || g1 != g2) CHECK((w1 < w2) == (g1 < g2 || (g1 == g2 && r1 < r2)));
        CHECK((w1 & 0xFFFFu) == s1 && ((w1 >> 16) & 0xFFFFu) == r1);
    }
    CHECK(pick_word(-0.f, 5, 9) == pick_word(0.f, 5, 9));

    // ---- the LDS of a wave
    CHECK(slots_for(1) == 64 && slots_for(64) == 64 && slots_for(65) == 128 && slots_for(200) == 256 && slots_for(1024) == 1024);
    for (int c = 1; c <= 1024; ++c) { const int s = slots_for(c); CHECK(s >= c && s >= 64 && (s & (s - 1)) == 0 && (s == 64 || s / 2 < c)); }
    CHECK(lds_bytes(64) == 64 * 20 + 256 && lds_bytes(1024) == 20736 && lds_bytes(1024) <= 160 * 1024 / 7);

    // ---- select against the naive rule
    std::vector<int> pick((size_t)MAX_CAND), npick;
    std::vector<float> div((size_t)MAX_CAND), m((size_t)MAX_CAND), ndiv;
    for (int trial = 0; trial < 400; ++trial) {
        const int c = trial < 8 ? trial + 1 : 1 + (int)(rnd() % 40u);
        const bool tied = trial & 1;                     // small integers: many equal r, D and g
        std::vector<float> r((size_t)c), D((size_t)c * c);
        for (int v = 0; v < c; ++v) r[(size_t)v] = tied ? (float)(rnd() % 3u) : (float)(rnd() & 0xFFFFu) / 4096.f - (trial % 3 ? 0.f : 4.f);
        for (int v = 1; v < c; ++v) if (r[(size_t)v] < r[(size_t)v - 1]) { const float t = r[(size_t)v]; r[(size_t)v] = r[(size_t)v - 1]; r[(size_t)v - 1] = t; v = 0; }   // rank order: ascending r
        for (int s = 0; s < c; ++s) for (int v = 0; v <= s; ++v)
            D[(size_t)s * c + v] = D[(size_t)v * c + s] = s == v ? 0.f : tied ? (float)(rnd() % 3u) : (float)(rnd() & 0xFFFFu) / 4096.f;
        for (float lambda : {0.f, 0.25f, 0.5f, 1.f}) for (int k : {1, 2, (c + 1) / 2, c, c + 3}) {
            if (k < 1 || k > MAX_CAND) continue;
            const int got = select(r.data(), D.data(), c, k, lambda, pick.data(), div.data(), m.data());
            const int want = naive_select(r, D, c, k, lambda, npick, ndiv);
            CHECK(got == want && got == (k < c ? k : c));
            for (int j = 0; j < got && j < want; ++j) CHECK(pick[(size_t)j] == npick[(size_t)j] && float_bits(div[(size_t)j]) == float_bits(ndiv[(size_t)j]));
            if (lambda == 1.f) for (int j = 0; j < got; ++j) CHECK(pick[(size_t)j] == j);      // lambda = 1: rank order
        }
    }

    std::printf("diverse plan %s: %ld cases, %ld differ\n", differ ? "FAILED" : "ok", cases, differ);
    return differ ? 1 : 0;
}
