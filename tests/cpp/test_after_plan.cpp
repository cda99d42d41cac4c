// The arithmetic of the paged searches that is plain numbers (ocaml-hnsw_amd/csrc/hnsw_after_plan.h) against its definitions:
//   ord        strictly monotone over a sweep of floats, with -inf, negative values, -0, +0, subnormals, +inf and a positive NaN;
//   is_after   a naive tuple compare, and cursor_word: word(D, v) > cursor_word(c) exactly when v is after c;
//   next_cursor the last real entry of a row, the input cursor when it has none;
//   l2_key_hi  hi(D) = max{s : sqrtf(s) <= D}: the neighbouring floats of the answer through sqrtf, for more than 10^5 values of D with
//              0, the smallest subnormal, FLT_MAX and +inf among them.
// A host program: built with the host compiler, and a second time under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../ocaml-hnsw_amd/csrc/hnsw_after_plan.h"

#include <cfloat>
#include <climits>
#include <cstdio>
#include <tuple>
#include <vector>

using namespace hnsw_after;

static long cases = 0, differ = 0;
#define CHECK(c) do { ++cases; if (!(c)) { if (differ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++differ; } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

int main() {
    // ---- ord: an ascending sweep of floats (by value; -0 before +0; the NaN last) has strictly ascending images
    std::vector<float> sweep;
    sweep.push_back(-INFINITY);
    for (uint32_t b = 0xFF7FFFFFu; b > 0x80000000u; b -= (b - 0x80000000u > 40000u ? 39989u : 1u)) sweep.push_back(bits_float(b));   // -FLT_MAX .. -subnormal
    sweep.push_back(bits_float(0x80000000u));   // -0
    sweep.push_back(0.f);
    for (uint32_t b = 1u; b < 0x7F800000u; b += (0x7F800000u - b > 40000u && b > 64u ? 39989u : 1u)) sweep.push_back(bits_float(b));    // subnormals .. FLT_MAX
    sweep.push_back(INFINITY);
    sweep.push_back(bits_float(0x7FC00000u));   // a positive NaN: above +inf
    for (size_t i = 0; i + 1 < sweep.size(); ++i) {
        CHECK(ord(sweep[i]) < ord(sweep[i + 1]));
        CHECK(float_bits(ord_inverse(ord(sweep[i]))) == float_bits(sweep[i]));
    }
    CHECK(ord(-0.f) + 1u == ord(0.f));
    CHECK(ord(bits_float(1u)) == ord(0.f) + 1u);
    CHECK(ord(FLT_MAX) + 1u == ord(INFINITY));

    // ---- is_after against the tuple compare, cursor_word against is_after
    const float dists[] = {-INFINITY, -2.5f, -0.f, 0.f, bits_float(1u), 1.f, bits_float(0x3F800001u), 3.25f, FLT_MAX, INFINITY};
    const int32_t cids[] = {INT32_MIN, INT32_MIN + 1, -2, -1, 0, 1, 2, 5, 6, 7, 1000, INT32_MAX - 1, INT32_MAX};
    const int64_t nodes[] = {0, 1, 4, 5, 6, 999, 1000, 2147483646ll, 2147483647ll};
    for (int32_t id_base : {0, 1}) for (float cd : dists) for (int32_t ci : cids) {
        const uint64_t lo = cursor_word(cd, ci, id_base);
        for (float D : dists) for (int64_t v : nodes) {
            const bool naive = std::make_tuple(ord(D), v + id_base) > std::make_tuple(ord(cd), (int64_t)ci);
            CHECK(is_after(D, v, id_base, cd, ci) == naive);
            CHECK((word(D, (uint32_t)v) > lo) == naive);
        }
    }
    for (int i = 0; i < 200000; ++i) {      // random pairs close to one another
        const float cd = bits_float((rnd() % 5u) + 0x3F800000u), D = bits_float((rnd() % 5u) + 0x3F800000u);
        const int32_t ci = (int32_t)(rnd() % 7u) - 2, id_base = (int32_t)(rnd() & 1u);
        const int64_t v = rnd() % 6u;
        const bool naive = std::make_tuple(ord(D), v + id_base) > std::make_tuple(ord(cd), (int64_t)ci);
        CHECK(is_after(D, v, id_base, cd, ci) == naive);
        CHECK((word(D, (uint32_t)v) > cursor_word(cd, ci, id_base)) == naive);
    }
    // the start cursor is before every node, whatever its distance
    CHECK(word(-INFINITY, 0u) > cursor_word(-INFINITY, INT32_MIN, 0));
    CHECK(word(-INFINITY, 0u) > cursor_word(-INFINITY, INT32_MIN, 1));

    // ---- next_cursor
    {
        const int32_t ids[] = {7, 3, -1, -1};
        const float d[] = {1.f, 2.f, NAN, NAN};
        float nd; int32_t ni;
        next_cursor(ids, d, 4, 0, 0.5f, 9, &nd, &ni);
        CHECK(nd == 2.f && ni == 3);
        next_cursor(ids, d, 1, 0, 0.5f, 9, &nd, &ni);
        CHECK(nd == 1.f && ni == 7);
        next_cursor(ids + 2, d + 2, 2, 0, 0.5f, 9, &nd, &ni);
        CHECK(nd == 0.5f && ni == 9);
        const int32_t one[] = {1, 0};          // id_base 1: id 0 is fill
        next_cursor(one, d, 2, 1, 0.5f, 9, &nd, &ni);
        CHECK(nd == 1.f && ni == 1);
        next_cursor(one, d, 0, 1, 0.5f, 9, &nd, &ni);
        CHECK(nd == 0.5f && ni == 9);
    }

    // ---- l2_key_hi against its definition
    auto check_hi = [](float D) {
        const int64_t hi = l2_key_hi(D);
        if (D < 0.f) { CHECK(hi == -1); return; }
        CHECK(hi >= 0 && hi <= 0x7F800000ll);
        if (hi < 0 || hi > 0x7F800000ll) return;
        CHECK(sqrtf(bits_float((uint32_t)hi)) <= D);                                 // hi is in the set ...
        if (hi < 0x7F800000ll) CHECK(sqrtf(bits_float((uint32_t)hi + 1u)) > D);      // ... and its successor is not (sqrtf is monotone)
    };
    for (float D : {0.f, -0.f, bits_float(1u), bits_float(2u), FLT_MIN, 1.f, FLT_MAX, (float)INFINITY, -1.f, -INFINITY, 1.8446743e19f, 1.8446744e19f, 1.8446745e19f})
        check_hi(D);
    CHECK(l2_key_hi(0.f) == 0 && l2_key_hi(-0.f) == 0 && l2_key_hi(bits_float(1u)) == 0);
    CHECK(l2_key_hi(INFINITY) == 0x7F800000ll && l2_key_hi(FLT_MAX) == 0x7F7FFFFFll);
    long n_hi = 0;
    for (uint32_t b = 0u; b <= 0x7F800000u; b += 16411u) { check_hi(bits_float(b)); ++n_hi; }        // a stride over every binade
    for (uint32_t b = 0u; b < 5000u; ++b) { check_hi(bits_float(b)); check_hi(bits_float(0x7F800000u - b)); n_hi += 2; }
    for (int i = 0; i < 60000; ++i) {       // the distances a search returns: square roots of sums
        const float s = bits_float(0x30000000u + rnd() % 0x20000000u);
        const float D = sqrtf(s);
        check_hi(D); ++n_hi;
        CHECK(l2_key_hi(D) >= (int64_t)float_bits(s));       // the sum D came from is not above hi(D)
    }
    CHECK(n_hi >= 100000);

    std::printf("after plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
