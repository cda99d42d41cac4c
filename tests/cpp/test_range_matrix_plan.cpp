// hnsw_scan_matrix_plan.h, the range scan's part (hnsw_range_matrix.hip): LDS and waves, eligibility, and the range rule: with the bound made
// from khi, the largest key in range, no pair whose chain key is at most khi is ever dropped.  Host arithmetic only: build with
// -fsanitize=address,undefined and run (tests/test_range_matrix_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_scan_matrix_plan.h"

#include <cstdio>
#include <initializer_list>
#include <random>
#include <vector>
using namespace hnsw_host;

static uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
static float flt(uint32_t b) { return __builtin_bit_cast(float, b); }
// dist_to_key, key_to_dist and range_key_bounds (hnsw_device.hip.h, hnsw_scan_device.hip.h), restated
static uint32_t dist_to_key(int metric, float acc) {
    const uint32_t b = bits(1.0f - acc);
    return metric == 0 ? bits(acc) : (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static float key_to_dist(int metric, uint32_t key) {
    return metric == 0 ? (float)std::sqrt((double)flt(key)) : flt((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}
static void range_key_bounds(int metric, float radius, uint32_t &lo, uint32_t &hi) {
    uint32_t a = metric == 0 ? 0u : 0x007FFFFFu, b = metric == 0 ? 0x7F800000u : 0xFF800000u;
    lo = a;
    if (!(key_to_dist(metric, a) <= radius)) { lo = 1u; hi = 0u; return; }
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1) + 1u;
        if (key_to_dist(metric, mid) <= radius) a = mid; else b = mid - 1u;
    }
    hi = a;
}
// the float scan's sum of (row, query): one fmaf chain per lane of a 16-lane group over its float4 chunks, then the reduce16 tree
static float chain(int metric, const float *x, const float *q, int d) {
    float p[16];
    for (int l = 0; l < 16; ++l) {
        p[l] = 0.f;
        for (int e = 0; e < d; ++e) {
            if (e / 4 % 16 != l) continue;
            const float dx = x[e] - q[e];
            p[l] = metric == 0 ? __builtin_fmaf(dx, dx, p[l]) : __builtin_fmaf(x[e], q[e], p[l]);
        }
    }
    for (int s = 8; s >= 1; s >>= 1) for (int j = 0; j < s; ++j) p[j] += p[j + s];
    return p[0];
}
// a stand-in for the matrix unit: every product rounded, pairwise fp32 sums
static float pairwise(const float *x, const float *q, int lo, int hi) {
    return hi - lo == 1 ? x[lo] * q[lo] : pairwise(x, q, lo, (lo + hi) / 2) + pairwise(x, q, (lo + hi) / 2, hi);
}
static float norm(const float *x, int d) { float s = 0.f; for (int i = 0; i < d; ++i) s = __builtin_fmaf(x[i], x[i], s); return s; }

int main() {
    int bad = 0, cases = 0;
    auto expect = [&](bool ok, const char *what) { ++cases; if (!ok) { ++bad; std::printf("FAILED: %s\n", what); } };
    for (int nch : {1, 2, 4, 8}) {      // the budget the kernel asserts
        const int w = range_matrix_waves(nch);
        expect(w == (scan_matrix_piece(nch) == 64 ? 8 : 4) && RANGE_MATRIX_WAVE_BYTES == 32 * RANGE_MATRIX_BUF * 4 + 256 && RANGE_MATRIX_BUF >= 64 &&
                   range_matrix_lds_bytes(nch) == scan_matrix_tile_bytes(nch) + w * RANGE_MATRIX_WAVE_BYTES && range_matrix_lds_bytes(nch) <= 160 * 1024 &&
                   range_matrix_lds_bytes(nch) < scan_matrix_lds_bytes(nch), "waves; LDS within 160 KB and below the k-scan's");
        for (int64_t v : {1ll, 8ll, 9ll, 1024ll}) expect(range_matrix_slab_groups(v, nch) * w >= v && (range_matrix_slab_groups(v, nch) - 1) * w < v, "slab groups");
    }
    expect(scan_matrix_eligible(1, false, 1, false) && scan_matrix_eligible(1, false, 512, false) && !scan_matrix_eligible(1, true, 128, false) &&
               !scan_matrix_eligible(0, false, 128, false) && !scan_matrix_eligible(1, false, 516, false), "eligibility: the k-scan's rule, byte handles keep the float range kernels");
    for (float r : {0.f, 0.5f, 3.25f, 1e30f, INFINITY})        // the threshold is the float khi, the last key in range, was made from
        for (int m : {0, 1}) {
            uint32_t lo, hi;
            range_key_bounds(m, r, lo, hi);
            const float t = range_matrix_threshold(m, hi);
            expect(hi >= lo && (m == 0 ? bits(t) == hi : t == key_to_dist(1, hi)) && key_to_dist(m, hi) <= r && (hi == (m ? 0xFF800000u : 0x7F800000u) || !(key_to_dist(m, hi + 1) <= r)), "threshold of khi");
        }
    { uint32_t lo, hi; range_key_bounds(0, -1.f, lo, hi); expect(hi < lo, "a negative L2 radius has no key"); }
    // the rule.  kind 0: Gaussian, 1: shifted far from the origin, 2: tiny values (squares near the subnormals), 3: rows that are the
    // query plus a perturbation of a few ulps (keys on and beside the boundary)
    std::mt19937 rng(11);
    std::normal_distribution<float> gauss;
    const int N = 160, NQ = 6;
    long dropped[2] = {}, kept_needed = 0, on_edge = 0;
    for (int d : {3, 100, 512})
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<float> X((size_t)N * d), Q((size_t)NQ * d);
            for (float &v : Q) v = (gauss(rng) + (kind == 1 ? 100.f : 0.f)) * (kind == 2 ? 1e-18f : 1.f);
            for (int r = 0; r < N; ++r)
                for (int i = 0; i < d; ++i) {
                    float &v = X[(size_t)r * d + i];
                    v = (gauss(rng) + (kind == 1 ? 100.f : 0.f)) * (kind == 2 ? 1e-18f : 1.f);
                    if (kind == 3) v = Q[(size_t)(r % NQ) * d + i] * (1.f + 0x1p-22f * (float)(int)(rng() % 5));
                }
            const float eps = scan_matrix_eps(d);
            for (int metric = 0; metric < 2; ++metric)
                for (int qi = 0; qi < NQ; ++qi) {
                    const float *q = &Q[(size_t)qi * d];
                    const float qt = scan_matrix_query_term(metric, norm(q, d), eps);
                    std::vector<uint32_t> key(N);
                    std::vector<float> val(N);
                    for (int r = 0; r < N; ++r) {
                        const float *x = &X[(size_t)r * d];
                        key[r] = dist_to_key(metric, chain(metric, x, q, d));
                        val[r] = scan_matrix_value(metric, scan_matrix_row_term(metric, norm(x, d), eps), pairwise(x, q, 0, d));
                    }
                    for (int tr = 0; tr < N; tr += 5)           // radii: a row's own distance (a pair on the edge) and the float below it
                        for (float radius : {key_to_dist(metric, key[tr]), std::nextafter(key_to_dist(metric, key[tr]), -INFINITY)}) {
                            uint32_t lo, hi;
                            range_key_bounds(metric, radius, lo, hi);
                            if (hi < lo) continue;
                            on_edge += key[tr] == hi;
                            const float b = scan_matrix_bound(metric, range_matrix_threshold(metric, hi), qt);
                            for (int r = 0; r < N; ++r) {
                                const bool keeps = scan_matrix_survives(val[r], b);
                                if (key[r] <= hi) { ++kept_needed; expect(keeps, "a pair whose key is in range was dropped"); }
                                else if (!keeps) ++dropped[metric];
                            }
                        }
                }
        }
    expect(kept_needed > 0 && on_edge > 0 && dropped[0] > 0 && dropped[1] > 0, "pairs sit on the edge, and the screen drops pairs: it is no rule that keeps everything");
    std::printf("range matrix plan %s: %d cases, %d failed\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
