// hnsw_diverse_plan.h -- the arithmetic of the diversified searches (hnsw_diversify_batch and the two searches over it,
// hnsw_diverse.hip) that is plain numbers: what the operator refuses of its arguments, mu, the score g of a candidate and its word in
// the argmin, the LDS of a wave, and the selection rule itself over given relevances r, pair distances D and ranks.  Host and device
// share these functions, so that a host program can check what the kernel computes (tests/cpp/test_diverse_plan.cpp, plainly and
// under AddressSanitizer and UBSan).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "hnsw_mi355x.h"

#if defined(__HIPCC__)
#define HNSW_DIVERSE_HD __host__ __device__ inline
#else
#define HNSW_DIVERSE_HD inline
#endif
// g is three rounded operations: no compiler may contract them into a fused multiply-add
#if defined(__GNUC__) && !defined(__clang__)
#define HNSW_DIVERSE_NO_FMA __attribute__((optimize("fp-contract=off")))
#else
#define HNSW_DIVERSE_NO_FMA
#endif

namespace hnsw_diverse {

constexpr int MAX_CAND = 1024;           // candidates per row, as hnsw_rerank_batch

HNSW_DIVERSE_HD uint32_t float_bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
HNSW_DIVERSE_HD float bits_float(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

// lambda weighs relevance against diversity: a number in [0, 1] (a NaN is in no interval)
HNSW_DIVERSE_HD bool lambda_ok(float lambda) { return lambda >= 0.0f && lambda <= 1.0f; }

// What the operator refuses of its plain numbers, in this order, before it looks at the handle and the arrays.  *why: a printf
// format taking (cand_stride, k) as two ints.
inline int check_args(int64_t nq, int32_t cand_stride, int32_t k, int32_t fill, float lambda, const char **why) {
    *why = nullptr;
    if (cand_stride < 1) { *why = "cand_stride must be >= 1 (cand_stride=%d)"; return HNSW_ERR_BAD_ARG; }
    if (cand_stride > MAX_CAND) { *why = "cand_stride=%d > 1024 not supported"; return HNSW_ERR_UNSUPPORTED; }
    if (k < 1 || k > cand_stride) { *why = "k must be in 1..cand_stride (cand_stride=%d k=%d)"; return HNSW_ERR_BAD_ARG; }
    if (fill != HNSW_FILL_OHNSW && fill != HNSW_FILL_BA) { *why = "bad fill"; return HNSW_ERR_BAD_ARG; }
    if (!lambda_ok(lambda)) { *why = "lambda must lie in [0, 1] and not be NaN"; return HNSW_ERR_BAD_ARG; }
    if (nq < 0 || nq > 0x7FFFFFFFLL) { *why = "nq out of range"; return HNSW_ERR_BAD_ARG; }
    return HNSW_OK;
}

// mu = fl(1 - lambda), once, in float32
HNSW_DIVERSE_HD float mu_of(float lambda) { return 1.0f - lambda; }

// g(v) = fl( fl(lambda * r) - fl(mu * m) ): two products and one difference, each rounded (numpy: lambda * r - mu * m on float32 arrays)
HNSW_DIVERSE_HD HNSW_DIVERSE_NO_FMA float score(float lambda, float mu, float r, float m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = lambda * r;
    const float b = mu * m;
    return a - b;
}

// g as an ordered 32-bit word: -0 folded into +0 (they compare equal as IEEE values), then the sign flipped, a negative value's other
// bits too -- ascending words = ascending g
HNSW_DIVERSE_HD uint32_t score_word(float g) {
    const uint32_t b = g == 0.0f ? 0u : float_bits(g);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// ... and the word of a candidate in a round's argmin: (g, rank) ascending, with the slot the candidate sits in (below 1024, as the
// rank) along for the winner's removal
HNSW_DIVERSE_HD uint64_t pick_word(float g, uint32_t rank, uint32_t slot) { return ((uint64_t)score_word(g) << 32) | (rank << 16) | slot; }

// the candidate slots of a wave: the power of two at or above cand_stride, 64 at least (the bitonic network's size)
HNSW_DIVERSE_HD int slots_for(int cand_stride) {
    int cap = 64;
    while (cap < cand_stride) cap <<= 1;
    return cap;
}
// LDS per wave: 20 bytes per slot -- the sort's 8-byte words, which then hold rank and m of the candidates still to pick, beside ids,
// relevance keys and the round's pair keys -- plus the evaluation's 64 scratch words: 1.5 KB at 64 candidates, 20.25 KB at 1024
HNSW_DIVERSE_HD size_t lds_bytes(int cap) { return (size_t)cap * 20 + 64 * 4; }

// The selection rule over plain numbers: c candidates in rank order, r[v] their relevance, D[s * c + v] the pair distance, picks
// min(k, c) of them.  pick[j]: the rank of pick j; div[j]: m at the moment of its selection (+inf for pick 1).  m: c floats of scratch.
// Returns the number of picks.
inline int select(const float *r, const float *D, int c, int k, float lambda, int *pick, float *div, float *m) {
    const float mu = mu_of(lambda);
    const int picks = k < c ? k : c;
    if (picks < 1) return 0;
    uint8_t done[MAX_CAND] = {0};
    for (int v = 0; v < c; ++v) m[v] = INFINITY;
    pick[0] = 0; div[0] = INFINITY;
    done[0] = 1;
    for (int j = 1; j < picks; ++j) {
        const int s = pick[j - 1];
        int best = -1;
        uint64_t best_word = 0;
        for (int v = 0; v < c; ++v) {
            if (done[v]) continue;
            const float dv = D[(size_t)s * c + v];
            if (dv < m[v]) m[v] = dv;
            const uint64_t w = pick_word(score(lambda, mu, r[v], m[v]), (uint32_t)v, (uint32_t)v);
            if (best < 0 || w < best_word) { best = v; best_word = w; }
        }
        pick[j] = best; div[j] = m[best];
        done[best] = 1;
    }
    return picks;
}

} // namespace hnsw_diverse
