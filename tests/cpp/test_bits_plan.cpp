// walk_query_words (ocaml-hnsw_amd/csrc/hnsw_bits_plan.h) against what the kernels do with a query row of the bit-row walks, for
// every d in 1..1024: the writer's words (bit_pack_kernel / bit_query_planes_kernel: per 64 dimensions one ballot = two words, per
// plane) and the reader's (load_query_bits / load_query_planes: lane l16 of step i) are replayed on a host matrix of three rows
// with that stride, every word written exactly once per row and none outside it.  Host arithmetic only: build with
// -fsanitize=address,undefined and run (tests/test_bit_query_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_bits_plan.h"

#include <cstdio>
#include <vector>

int main() {
    using namespace hnsw_host;
    int cases = 0, bad = 0;
    const int64_t nq = 3;
    for (int d = 1; d <= 1024; ++d)
        for (int planes = 0; planes < 2; ++planes) {
            const int nw = bit_words(d), units = 8 * nw, np = planes ? 4 : 1;
            const int64_t stride = walk_query_words(d, planes != 0), used = (int64_t)np * 16 * nw;
            bool ok = nw == (d + 511) / 512 && stride >= used && stride % 16 == 0;
            if (planes) ok = ok && stride == 64 * nw;            // exactly the planes
            else ok = ok && stride == padded_stride(d) && stride >= d && stride < d + 16;
            std::vector<uint32_t> m((size_t)(nq * stride), 0u);  // (exactly nq rows: a word past the last row is the sanitizer's)
            for (int64_t q = 0; q < nq; ++q) {
                for (int p = 0; p < np; ++p)
                    for (int u = 0; u < units; ++u)
                        for (int h = 0; h < 2; ++h) {            // the writer: the ballot's low and high word
                            const int64_t w = (int64_t)2 * units * p + 2 * u + h;
                            ok = ok && w < stride;
                            m[(size_t)(q * stride + w)] += 1u;
                        }
                for (int p = 0; p < np; ++p)
                    for (int i = 0; i < nw; ++i)
                        for (int l16 = 0; l16 < 16; ++l16) {     // the reader: plane p, step i, lane l16
                            const int64_t w = (int64_t)p * 16 * nw + i * 16 + l16;
                            ok = ok && w < stride && m[(size_t)(q * stride + w)] == 1u;
                        }
            }
            // the bits of dimension i: bit i % 32 of word i / 32 of its plane, inside the plane
            ok = ok && (d - 1) / 32 < 16 * nw;
            ++cases;
            if (!ok) { ++bad; std::printf("d %d planes %d: stride %lld\n", d, planes, (long long)stride); }
        }
    // the trap: a narrow row's planes do not fit its padded float stride
    if (!(walk_query_words(20, true) == 64 && padded_stride(20) == 32 && walk_query_words(20, false) == 32)) ++bad;
    if (!(walk_query_words(1024, true) == 128 && walk_query_words(513, true) == 128 && walk_query_words(512, true) == 64)) ++bad;
    std::printf("bits plan ok: %d cases, %d differ\n", cases, bad);
    return bad ? 1 : 0;
}
