// hnsw_scan_matrix_plan.h (option "scan_matrix"): eligibility, LDS, grid and scratch, and the screening rule: no pair whose chain key is at
// most a threshold key is ever dropped.  Host arithmetic only: build with -fsanitize=address,undefined and run (tests/test_scan_matrix_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_scan_matrix_plan.h"

#include <cstdio>
#include <initializer_list>
#include <random>
#include <vector>
using namespace hnsw_host;

// the float scan's sum of (row, query): lane l16 of a 16-lane group on the float4 chunks l16, l16 + 16, ..., one fmaf chain per lane,
// then the tree p[j] += p[j + 8], p[j + 4], p[j + 2], p[j + 1] (hnsw_scan_device.hip.h, reduce16)
static float chain(int metric, const float *x, const float *q, int d) {
    const int nch = scan_matrix_nch(d);
    float p[16];
    for (int l = 0; l < 16; ++l) {
        p[l] = 0.f;
        for (int e = 0; e < 64 * nch; ++e) {        // the lane's elements in order: chunk 16 i + l is elements 64 i + 4 l ..
            if (e / 4 % 16 != l || e >= d) continue;
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
    expect(scan_matrix_eligible(1, false, 128, false) && scan_matrix_eligible(1, false, 1, false) && scan_matrix_eligible(1, false, 512, false), "on, d 1, 128, 512");
    expect(!scan_matrix_eligible(0, false, 128, false) && !scan_matrix_eligible(2, false, 128, false) && !scan_matrix_eligible(1, true, 128, false), "off, no switch value, byte precedence");
    expect(!scan_matrix_eligible(1, false, 513, false) && !scan_matrix_eligible(1, false, 0, false) && !scan_matrix_eligible(1, false, 128, true), "d out of range, per-query filters");
    for (int d = 1; d <= SCAN_MATRIX_MAX_D; ++d) {
        const int nch = scan_matrix_nch(d), w = scan_matrix_waves(nch);
        expect(scan_matrix_width(nch) >= d && scan_matrix_width(nch) < 2 * d + 64 && scan_matrix_width(nch) % scan_matrix_piece(nch) == 0 &&
                   (scan_matrix_pitch(nch) * 4) % 16 == 0 && (scan_matrix_pitch(nch) / 4) % 2 == 1, "row width; pitch float4 aligned, an odd number of bank quads");
        expect((w == 4 || w == 8) && scan_matrix_lds_bytes(nch) <= SCAN_MATRIX_LDS_MAX && scan_matrix_lds_bytes(nch) == scan_matrix_tile_bytes(nch) + w * SCAN_MATRIX_WAVE_BYTES &&
                   scan_matrix_tile_bytes(nch) % 16 == 0 && scan_matrix_eps(d) > 0.f && scan_matrix_eps(d) < 0x1p-11f && (d == 1 || scan_matrix_eps(d) > scan_matrix_eps(d - 1)), "LDS within 160 KB; margin");
    }
    for (int64_t v : {1ll, 31ll, 32ll, 33ll, 10000ll, 0x7FFFFFFFll})
        for (int nch : {1, 2, 4, 8})
            expect(scan_matrix_tiles(v) * SCAN_MATRIX_TILE >= v && (scan_matrix_tiles(v) - 1) * SCAN_MATRIX_TILE < v && scan_matrix_scratch(v) == 4 * v &&
                       scan_matrix_slab_groups(v, nch) * scan_matrix_waves(nch) >= v && (scan_matrix_slab_groups(v, nch) - 1) * scan_matrix_waves(nch) < v, "grid and scratch");
    // the rule.  kind 0: Gaussian, 1: shifted far from the origin, 2: magnitudes mixed over 12 decades, 3: rows that are the query
    // plus a perturbation of a few ulps, 4: Gaussian with a row of 1e20 and one of 1e-25
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss;
    const int N = 192, NQ = 8;
    long dropped[2][5] = {}, kept_needed = 0;
    for (int d : {3, 100, 512})
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<float> X((size_t)N * d), Q((size_t)NQ * d);
            for (float &v : Q) v = gauss(rng) + (kind == 1 ? 100.f : 0.f);
            for (int r = 0; r < N; ++r)
                for (int i = 0; i < d; ++i) {
                    float v = gauss(rng);
                    if (kind == 1) v += 100.f;
                    if (kind == 2) v *= std::pow(10.f, (float)(int)(rng() % 13) - 6.f);
                    if (kind == 3) v = Q[(size_t)(r % NQ) * d + i] * (1.f + 0x1p-22f * (float)(int)(rng() % 5));
                    if (kind == 4 && r == 5) v *= 1e20f;
                    if (kind == 4 && r == 6) v *= 1e-25f;
                    X[(size_t)r * d + i] = v;
                }
            const float eps = scan_matrix_eps(d);
            for (int metric = 0; metric < 2; ++metric)
                for (int qi = 0; qi < NQ; ++qi) {
                    const float *q = &Q[(size_t)qi * d];
                    const float qt = scan_matrix_query_term(metric, norm(q, d), eps);
                    std::vector<float> key(N), val(N);
                    for (int r = 0; r < N; ++r) {
                        const float *x = &X[(size_t)r * d];
                        key[r] = metric == 0 ? chain(0, x, q, d) : 1.0f - chain(1, x, q, d);     // what the key orders by
                        val[r] = scan_matrix_value(metric, scan_matrix_row_term(metric, norm(x, d), eps), pairwise(x, q, 0, d));
                    }
                    for (int tr = 0; tr < N; tr += 7) {         // the k-th word's float: a row's own, every seventh row
                        const float b = scan_matrix_bound(metric, key[tr], qt);
                        for (int r = 0; r < N; ++r) {
                            const bool keeps = scan_matrix_survives(val[r], b);
                            if (!(key[r] > key[tr])) { ++kept_needed; expect(keeps, "a pair at or below the threshold was dropped"); }
                            else if (!keeps) ++dropped[metric][kind];
                        }
                    }
                }
        }
    expect(kept_needed > 0 && dropped[0][0] > 0 && dropped[1][0] > 0 && dropped[0][2] > 0, "the screen drops pairs on plain data: it is no rule that keeps everything");
    // failing towards "survives": NaN and infinite terms never drop a pair
    for (int m : {0, 1}) expect(scan_matrix_survives(scan_matrix_value(m, scan_matrix_row_term(m, INFINITY, 0x1p-10f), 1.f), m ? -5.f : 5.f), "an infinite row norm survives");
    expect(scan_matrix_survives(scan_matrix_value(0, 3.f, NAN), 1.f) && scan_matrix_survives(1e30f, scan_matrix_bound(0, 1.f, INFINITY)) &&
               scan_matrix_survives(1e30f, scan_matrix_bound(0, INFINITY, 1.f)) && !scan_matrix_survives(INFINITY, scan_matrix_bound(0, 1.f, 1.f)), "NaN sum, infinite query norm or threshold keep; an excluded row's +inf drops");
    std::printf("scan matrix plan %s: %d cases, %d failed\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
