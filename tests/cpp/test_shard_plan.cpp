// shard_lo, cut_mask, SegPlan and check_lims (ocaml-hnsw_amd/csrc/hnsw_shard_plan.h) against a naive restatement: the partition
// bounds in 128-bit arithmetic, the cut mask bit by bit into a buffer of exactly the words it may write, the segment plan against
// a running sum.  A host program: tests/test_sharded_api.py builds it with -fsanitize=address,undefined and runs it.
#include "../../ocaml-hnsw_amd/csrc/hnsw_shard_plan.h"

#include <algorithm>
#include <cstdio>
#include <memory>
#include <vector>

using namespace hnsw_host;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static long cases = 0, differ = 0;
static void expect(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0) {
    ++cases;
    if (!ok) { ++differ; std::printf("differs: %s (%lld, %lld, %lld)\n", what, a, b, c); }
}

static void test_shard_lo() {
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)7, (int64_t)64, (int64_t)1000, ((int64_t)1 << 40) + 3}) {
        for (int G : {1, 2, 3, 4, 5, 6, 7, 8, 64}) {
            expect(shard_lo(n, 0, G) == 0, "lo(0) = 0", n, G);
            expect(shard_lo(n, G, G) == n, "lo(G) = n", n, G);
            int64_t least = n, most = 0;
            for (int g = 0; g < G; ++g) {
                const int64_t lo = shard_lo(n, g, G), hi = shard_lo(n, g + 1, G);
                expect(lo <= hi, "monotone", n, G, g);
                expect(lo == (int64_t)(((__int128)n * g) / G), "(n * g) / G in 128 bits", n, G, g);
                least = std::min(least, hi - lo);
                most = std::max(most, hi - lo);
            }
            expect(most - least <= 1, "sizes differ by at most 1", n, G);
        }
    }
}

// one part [lo, lo + n) of `bits` (n_bits bits): the output buffer has exactly max(words, 1) words on the heap, so a store past it is
// an AddressSanitizer report; the source has exactly ceil(n_bits / 32) words (one for n_bits = 0: an address), so is a load past it
static void cut_one(const std::vector<uint8_t> &bit, int64_t lo, int64_t n) {
    const int64_t n_bits = (int64_t)bit.size(), src_words = (n_bits + 31) / 32, words = (n + 31) / 32;
    std::unique_ptr<uint32_t[]> src(new uint32_t[(size_t)std::max<int64_t>(src_words, 1)]());
    for (int64_t v = 0; v < n_bits; ++v) if (bit[(size_t)v]) src[(size_t)(v >> 5)] |= 1u << (v & 31);
    std::unique_ptr<uint32_t[]> out(new uint32_t[(size_t)std::max<int64_t>(words, 1)]);
    for (int64_t w = 0; w < std::max<int64_t>(words, 1); ++w) out[(size_t)w] = 0xDEADBEEFu;
    cut_mask(src.get(), n_bits, lo, n, out.get());
    bool ok = true;
    for (int64_t j = 0; ok && j < std::max<int64_t>(words, 1) * 32; ++j) {
        const bool got = (out[(size_t)(j >> 5)] >> (j & 31)) & 1u;
        ok = got == (j < n ? bit[(size_t)(lo + j)] != 0 : false);        // past n: clear
    }
    expect(ok, "cut_mask", n_bits, lo, n);
}

static void test_cut_mask() {
    for (int64_t n_bits : {0, 1, 31, 32, 33, 63, 64, 65, 1000}) {
        for (int fillv : {0, 1, 2, 3}) {                                  // zeros, ones, two random masks
            std::vector<uint8_t> bit((size_t)n_bits);
            for (auto &b : bit) b = fillv == 0 ? 0 : fillv == 1 ? 1 : (uint8_t)(rnd() & 1u);
            for (int G = 1; G <= 5; ++G)
                for (int g = 0; g < G; ++g) cut_one(bit, shard_lo(n_bits, g, G), shard_lo(n_bits, g + 1, G) - shard_lo(n_bits, g, G));
            // hand-made bounds: an empty part (at the start, inside, at the end), a part that starts at bit 31, parts that end on the
            // last bit
            for (int64_t at : {(int64_t)0, n_bits / 2, n_bits}) cut_one(bit, at, 0);
            if (n_bits >= 31) {
                cut_one(bit, 31, n_bits - 31);
                cut_one(bit, 31, std::min<int64_t>(n_bits - 31, 33));
                cut_one(bit, 31, std::min<int64_t>(n_bits - 31, 1));
            }
            for (int64_t len : {(int64_t)1, (int64_t)32, (int64_t)33}) if (len <= n_bits) cut_one(bit, n_bits - len, len);
        }
    }
}

static void test_seg_plan() {
    const int64_t M = SEG_ENTRIES;
    expect(M == 0x7FFFFFFFLL, "SEG_ENTRIES is 2^31 - 1");
    // accepted: totals with zeros; the bases are the exclusive sum
    for (int n_lists : {1, 2, 5, 64}) {
        SegPlan p;
        int64_t sum = 0, longest = 0;
        bool ok = true;
        for (int g = 0; g < n_lists; ++g) {
            const int64_t t = (g % 3 == 1) ? 0 : (int64_t)(rnd() % 100000), first = 1000 * (int64_t)g;
            ok = ok && p.add(t, first) == SEG_OK && p.base[g] == sum && p.total[g] == t && p.first_row[g] == first;
            sum += t;
            longest = std::max(longest, t);
        }
        expect(ok && p.n_lists == n_lists && p.sum == sum && p.longest == longest && p.close() == SEG_OK, "an accepted plan", n_lists);
    }
    {   // one list at exactly 2^31 - 1, alone
        SegPlan p;
        expect(p.add(M, 0) == SEG_OK && p.close() == SEG_OK && p.sum == M && p.longest == M && p.base[0] == 0, "one list of 2^31 - 1 entries");
    }
    for (int bad : {0, 1, 3}) {   // a list above 2^31 - 1: refused at that list, the plan as it was before it
        SegPlan p;
        int refused_at = -1;
        for (int g = 0; g < 4 && refused_at < 0; ++g)
            if (p.add(g == bad ? M + 1 : 10, g) != SEG_OK) refused_at = g;
        expect(refused_at == bad && p.n_lists == bad && p.sum == 10 * (int64_t)bad, "a list above 2^31 - 1", bad, refused_at);
    }
    {   // a sum above 2^31 - 1 of lists that fit
        SegPlan p;
        expect(p.add(M, 0) == SEG_OK && p.add(0, 5) == SEG_OK && p.add(1, 9) == SEG_OK && p.close() == SEG_SUM_TOO_LONG && p.sum == M + 1 &&
                   p.base[2] == M,
               "a sum above 2^31 - 1");
        SegPlan q;
        expect(q.add(M - 1, 0) == SEG_OK && q.add(1, 1) == SEG_OK && q.close() == SEG_OK, "a sum of exactly 2^31 - 1");
    }
}

static void test_check_lims() {
    int64_t at = -1;
    const int64_t good[] = {0, 0, 3, 3, 9}, start[] = {1, 1, 3}, down[] = {0, 4, 4, 2, 9}, none[] = {0}, none_bad[] = {7};
    expect(check_lims(good, 4, &at) == LIMS_OK, "lims accepted");
    expect(check_lims(none, 0, &at) == LIMS_OK, "lims of no query accepted");
    expect(check_lims(start, 2, &at) == LIMS_START, "lims not starting at 0");
    expect(check_lims(none_bad, 0, &at) == LIMS_START, "lims of no query not starting at 0");
    expect(check_lims(down, 4, &at) == LIMS_DECREASE && at == 2, "a decreasing step", at);
}

int main() {
    test_shard_lo();
    test_cut_mask();
    test_seg_plan();
    test_check_lims();
    std::printf("shard plan ok: %ld cases, %ld differ\n", cases, differ);
    return differ ? 1 : 0;
}
